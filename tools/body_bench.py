"""Time of the body-sensor updates of one tick on one GPU at the headline shape, by the two routes the library has:

  A   the route before viekf_batch_update_body: one viekf_batch_update per measurement (after a fused step: the unpack
      launch, the mirror launch, then a read-modify-write pass over the whole square of P per measurement)
  B   BatchVIEKF.update_body: one call (after a fused step: the unpack launch, then one pass over the lower triangle)

    python tools/body_bench.py [--batch 1024] [--features 50] [--reps 40] [--warmup 5] [--ticks 20] [--out profiles/body]

Workloads, what the reference's callbacks do per tick (src/vi_ekf_ros.cpp:172-199, :452-470):
  imu_tick            step_n(K = 1, M = 0), then [ACC, ATT]
  truth_tick          step_n(K = 1, M = 0), then [POS, ATT, VEL, ALT]
  imu_updates_only    [ACC, ATT] on a canonical P, no step between the ticks
  truth_updates_only  [POS, ATT, VEL, ALT] likewise
Three batches at the same state run every workload: A, a twin of A (the A/A pair: the spread a difference has to beat) and
B, interleaved window by window in the same process, with the order rotating.  A window is --ticks ticks between two device
events on the batches' stream; all arguments are device tensors.  Before a window every z is set to the model's prediction
at the filter's state (eval_h, untimed), so that nothing is gated; the share of accepted entries is reported.  Medians of
--reps windows after --warmup, per tick, min .. max beside them.

The fused route has to move, per filter, the lower triangle of the active block once in and once out, and the panel once
more on its way in: 8 (n (n + 1) + 16 n) bytes.  `fused_hbm_frac` is that over the time of a B call of the updates-only
workloads over the HBM peak bench.py's roofline uses -- the rate of the whole call, launch included, not a kernel's share.
Prints one JSON line and appends it to <out>/body_bench_run.jsonl."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # (bench.py's roofline: MI355X_MICROARCH.md, 8.0 TB/s spec)
ACC, ALT, ATT, POS, VEL = 0, 1, 2, 3, 4
ZDIM = {ACC: 2, ALT: 1, ATT: 4, POS: 3, VEL: 3}
RDIM = {ACC: 2, ALT: 1, ATT: 3, POS: 3, VEL: 3}
RVAR = {ACC: 1.0, ALT: 1.0, ATT: 0.1, POS: 1.0, VEL: 1.0}
WORKLOADS = (("imu_tick", True, (ACC, ATT)), ("truth_tick", True, (POS, ATT, VEL, ALT)),
             ("imu_updates_only", False, (ACC, ATT)), ("truth_updates_only", False, (POS, ATT, VEL, ALT)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, scene
    B, N = a.batch, a.features
    if v.device_count() < 1:
        raise SystemExit("body_bench needs a GPU: a timing taken anywhere else says nothing")
    L = capi.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sc = scene.make_scene(B, N, 2, seed=11)
    assert sc["params"]["use_drag_term"], "the deployment this measures uses the drag-term accelerometer update"
    Mw = min(N, 8)

    def make():
        g = v.BatchVIEKF(B, N, sc["params"])
        g.set_stream(stream.cuda_stream)
        for i in range(N):
            g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        for s in range(2):
            g.step(sc["u"][s], sc["dt"], np.ascontiguousarray(sc["z"][s][:, :Mw, :]), np.ascontiguousarray(sc["slot"][:, :Mw]), sc["R"])
        return g

    batches = {"A": make(), "A2": make(), "B": make()}
    u = torch.tensor(sc["u"][1][None], device=dev)                      # [1, B, 6]
    dt = torch.tensor(sc["dt"][None], device=dev)                       # [1, B]
    n = 16 + 3 * N
    fused_bytes = 8 * (n * (n + 1) + 16 * n) * B

    def inputs(g, types):
        """z [M][B][4] at the filter's own prediction, R [M][9], per-entry [B][zdim] views for route A, a result buffer"""
        M = len(types)
        z = np.zeros((M, B, 4))
        R = np.zeros((M, 9))
        for m, t in enumerate(types):
            z[m] = np.nan_to_num(g.eval_h(t))
            r = RDIM[t]
            R[m, :r * r] = (RVAR[t] * np.eye(r)).ravel()
        zd = torch.tensor(z, device=dev)
        za = [zd[m, :, :ZDIM[t]].contiguous() for m, t in enumerate(types)]
        return dict(z=zd, za=za, R=torch.tensor(R, device=dev), res=torch.full((M, B), -9, dtype=torch.int32, device=dev))

    def tick(name, g, step, types, x):
        if step:
            g.step_n(u, dt, None, None, None)
        if name == "B":
            _, route = g.update_body((list(types), [ZDIM[t] for t in types], [RDIM[t] for t in types], x["z"], x["R"]), result=x["res"])
            assert route == 1
        else:
            for m, t in enumerate(types):
                capi.check(L.viekf_batch_update(g._h, t, C.c_void_p(x["za"][m].data_ptr()), ZDIM[t], C.c_void_p(x["R"][m].data_ptr()), RDIM[t],
                                                0, None, None, C.c_void_p(x["res"][m].data_ptr()), capi.DEVICE))

    out = dict(tool="body_bench", batch=B, features=N, ticks_per_window=a.ticks, reps=a.reps, kernels=batches["B"].describe(),
               fused_bytes_per_call=fused_bytes, hbm_peak_gbs=HBM_PEAK_GBS)
    order = ["A", "B", "A2"]
    for wname, step, types in WORKLOADS:
        ms = {k: [] for k in batches}
        accepted = {k: [] for k in batches}
        for r in range(a.warmup + a.reps):
            order = order[1:] + order[:1]
            for k in order:
                g = batches[k]
                x = inputs(g, types)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.ticks):
                    tick(k, g, step, types, x)
                e1.record(stream)
                e1.synchronize()
                if r >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1) / a.ticks)
                    accepted[k].append(float((x["res"] == 0).double().mean().item()))

        def med(xs):
            xs = np.array(xs)
            return dict(ms=round(float(np.median(xs)), 5), ms_min=round(float(xs.min()), 5), ms_max=round(float(xs.max()), 5))

        A, A2, Bm = med(ms["A"]), med(ms["A2"]), med(ms["B"])
        w = dict(M=len(types), with_step=step, A=A, A_twin=A2, B=Bm, aa_spread=round(abs(A["ms"] - A2["ms"]) / A["ms"], 4),
                 B_over_A=round(Bm["ms"] / A["ms"], 4), accepted=dict((k, round(float(np.mean(vv)), 4)) for k, vv in accepted.items()))
        if not step:
            w["fused_hbm_gbs"] = round(fused_bytes / (Bm["ms"] * 1e-3) / 1e9, 1)
            w["fused_hbm_frac"] = round(fused_bytes / (Bm["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        out[wname] = w
    # the three batches took the same measurements: the same state at the end, to rounding
    xa, xb = batches["A"].get_state(), batches["B"].get_state()
    out["x_rel_diff_A_vs_B"] = float(np.abs(xa - xb).max() / np.abs(xa).max())
    print(json.dumps(out), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "body_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
