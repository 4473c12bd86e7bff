"""Time of the PIXEL_VEL updates of one camera frame on one GPU at the headline shape, against the yardstick the library had
before them:

  F   one viekf_batch_update(FEAT) per feature: rank-2 updates through k_update_generic, a kernel this model does not touch
  P   BatchVIEKF.update_pixel_vels: one call, the fused launch k_update_pixvels (route 1)
  P0  the same call on a batch held to route 0: M launches of k_update_pixvel, the definition of the results

    python tools/pixvel_bench.py [--batch 1024] [--features 50] [--reps 20] [--warmup 4] [--ticks 3] [--out profiles/pixvel]

Workloads:
  frame          step_n(K = 1, the frame's M = N FEAT updates: one fused launch, P left packed), then the N updates
  updates_only   the N updates on a canonical P, no step between the frames
Four batches at the same state run every workload: F, a twin of F (the F/F pair: the spread a difference has to beat), P
and P0, interleaved window by window in the same process, with the order rotating.  A window is --ticks frames between two device
events on the batches' stream; all arguments are device tensors.  Before a window every z is set to the model's prediction
at the filter's state (eval_h / eval_pixel_vel, untimed), so that nothing is gated; the share of accepted entries is reported.
Medians of --reps windows after --warmup, per frame, min .. max beside them.

The fused route has to move, per filter, the lower triangle of the active block once in and once out, the six body columns
and three columns per entry once more on their way in: 8 (n (n + 1) + 6 n + 3 M n) bytes.  `fused_hbm_frac` is that over the
time of a P call of updates_only over the HBM peak bench.py's roofline uses -- the rate of the whole call, launch included.
Prints one JSON line and appends it to <out>/pixvel_bench_run.jsonl."""
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
FEAT = 6
GYRO_VAR = 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixvel"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, scene
    N = a.features
    if v.device_count() < 1:
        raise SystemExit("pixvel_bench needs a GPU: a timing taken anywhere else says nothing")
    L = capi.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    n = 16 + 3 * N
    Mw = min(N, 8)
    B = a.batch
    sc = scene.make_scene(B, N, 2, seed=11)
    gyro_h = np.ascontiguousarray(sc["u"][1][:, 3:6])
    gyro = torch.tensor(gyro_h, device=dev)
    Rf = torch.tensor(np.ascontiguousarray(np.asarray(sc["R"], dtype=np.float64)), device=dev)      # FEAT: 2 x 2, symmetric
    Rp = torch.tensor(np.diag([400.0, 400.0]), device=dev)                                           # PIXEL_VEL: (20 px/s)^2

    def make():
        g = v.BatchVIEKF(B, N, sc["params"])
        g.set_stream(stream.cuda_stream)
        for i in range(N):
            g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        for s in range(2):
            g.step(sc["u"][s], sc["dt"], np.ascontiguousarray(sc["z"][s][:, :Mw, :]), np.ascontiguousarray(sc["slot"][:, :Mw]), sc["R"])
        return g

    def inputs(name, g):
        """every entry's z at the filter's own prediction, slots 0 .. N-1"""
        slot = np.tile(np.arange(N, dtype=np.int32), (B, 1))
        zf = np.ascontiguousarray(np.stack([g.eval_h(FEAT, np.full(B, m, np.int32))[:, :2] for m in range(N)], axis=1))
        x = dict(slot=torch.tensor(slot, device=dev), zf=torch.tensor(zf, device=dev), rf=torch.full((B, N), -9, dtype=torch.int32, device=dev))
        if name == "P":
            zp = np.stack([g.eval_pixel_vel(np.full(B, m, np.int32), gyro_h, jacobian=False)[0] for m in range(N)], axis=1)
            x["zp"] = torch.tensor(np.ascontiguousarray(zp), device=dev)
            x["res"] = torch.full((B, N), -9, dtype=torch.int32, device=dev)
        else:
            x["za"] = [x["zf"][:, m].contiguous() for m in range(N)]
            x["sa"] = [x["slot"][:, m].contiguous() for m in range(N)]
            x["ra"] = torch.full((N, B), -9, dtype=torch.int32, device=dev)
        return x

    def tick(name, g, x, step):
        if step is not None:
            g.step_n(step[0], step[1], x["zf"], x["slot"], Rf, result=x["rf"])
        if name == "P":
            _, route = g.update_pixel_vels(x["zp"], x["slot"], gyro, Rp, GYRO_VAR, None, 0, result=x["res"])
            routes.add(route)
        else:
            for m in range(N):
                capi.check(L.viekf_batch_update(g._h, FEAT, C.c_void_p(x["za"][m].data_ptr()), 2, C.c_void_p(Rf.data_ptr()), 2, 0,
                                                C.c_void_p(x["sa"][m].data_ptr()), None, C.c_void_p(x["ra"][m].data_ptr()), capi.DEVICE))

    def window(name, g, step):
        x = inputs(name, g)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.ticks):
            tick(name, g, x, step)
        e1.record(stream)
        e1.synchronize()
        res = x["res"] if name == "P" else x["ra"]
        return e0.elapsed_time(e1) / a.ticks, float((res == 0).double().mean().item())

    def med(xs):
        xs = np.array(xs)
        return dict(ms=round(float(np.median(xs)), 5), ms_min=round(float(xs.min()), 5), ms_max=round(float(xs.max()), 5))

    batches = {"F": make(), "F2": make(), "P": make(), "P0": make()}
    batches["P0"].pixel_vels_route(0)
    routes = set()
    u = torch.tensor(sc["u"][1][None], device=dev)                      # [1, B, 6]
    dt = torch.tensor(sc["dt"][None], device=dev)                       # [1, B]
    bytes_p = 8 * (n * (n + 1) + 6 * n + 3 * N * n) * B
    out = dict(tool="pixvel_bench", batch=B, features=N, M=N, ticks_per_window=a.ticks, reps=a.reps, kernels=batches["P"].describe(),
               lds_bytes=int(L.viekf_pixvels_lds_bytes(N, N)), fused_bytes_per_call=bytes_p, hbm_peak_gbs=HBM_PEAK_GBS)
    order = ["F", "P", "F2", "P0"]
    for wname, step in (("frame", (u, dt)), ("updates_only", None)):
        ms = {k: [] for k in batches}
        accepted = {k: [] for k in batches}
        for r in range(a.warmup + a.reps):
            order = order[1:] + order[:1]
            for k in order:
                routes.clear()
                t, acc = window("P" if k in ("P", "P0") else "F", batches[k], step)
                assert routes <= {1 if k == "P" else 0}, (k, routes)
                if r >= a.warmup:
                    ms[k].append(t)
                    accepted[k].append(acc)
        F, F2, P, P0 = med(ms["F"]), med(ms["F2"]), med(ms["P"]), med(ms["P0"])
        w = dict(with_step=step is not None, F=F, F_twin=F2, P=P, P0=P0, ff_spread=round(abs(F["ms"] - F2["ms"]) / F["ms"], 4),
                 P_over_F=round(P["ms"] / F["ms"], 4), P_over_P0=round(P["ms"] / P0["ms"], 4), accepted=dict((k, round(float(np.mean(vv)), 4)) for k, vv in accepted.items()))
        if step is None:
            w["fused_hbm_gbs"] = round(bytes_p / (P["ms"] * 1e-3) / 1e9, 1)
            w["fused_hbm_frac"] = round(bytes_p / (P["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        out[wname] = w
    xa, xb = batches["P"].get_state(), batches["P0"].get_state()
    out["x_bit_equal_P_vs_P0"] = bool(np.array_equal(xa, xb))
    print(json.dumps(out), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "pixvel_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
