"""Time of the DEPTH updates of one camera frame on one GPU at the headline shape, by the two routes the library has:

  A   the route before viekf_batch_update_depths: one viekf_batch_update(DEPTH) per feature (after a fused step: the unpack
      launch, the mirror launch, then a read-modify-write pass over the whole square of P per measurement)
  B   BatchVIEKF.update_depths: one call (after a fused step: the unpack launch, then one pass over the lower triangle)

    python tools/depth_bench.py [--batch 1024] [--features 50] [--reps 30] [--warmup 4] [--ticks 5] [--out profiles/depth]

Workloads:
  frame          step_n(K = 1, the frame's M = N FEAT updates: one fused launch, P left packed), then the N DEPTH updates
  depths_only    the N DEPTH updates on a canonical P, no step between the frames
Three batches at the same state run every workload: A, a twin of A (the A/A pair: the spread a difference has to beat) and
B, interleaved window by window in the same process, with the order rotating.  A window is --ticks frames between two device
events on the batches' stream; all arguments are device tensors.  Before a window every z is set to the model's prediction
at the filter's state (eval_h, untimed), so that nothing is gated; the share of accepted entries is reported.  Medians of
--reps windows after --warmup, per frame, min .. max beside them.

The fused route has to move, per filter, the lower triangle of the active block once in and once out and one column of it
per entry once more on its way in: 8 (n (n + 1) + M n) bytes.  `fused_hbm_frac` is that over the time of a B call of
depths_only over the HBM peak bench.py's roofline uses -- the rate of the whole call, launch included.

What bounds the launch is told apart with two sweeps of route B on a canonical P (same windows, B alone):
  by_batch   256 / 512 / 1024 / 2048 filters: 256 workgroups fill the device's compute units once, and at N = M = 50 two fit
             on a unit; a time that stays flat up to 512 and then grows with the batch is workgroups' latency hidden by
             occupancy until the units are full; one that grows in proportion from the start is a shared resource
  by_m       M = 1 / 10 / 25 / 50 at the headline batch: the chain's column work grows with M^2 / 2, the trailing pass's
             arithmetic with M, its traffic not at all
Prints one JSON line and appends it to <out>/depth_bench_run.jsonl."""
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
FEAT, DEPTH = 6, 8
R_DEPTH = 0.04 ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, scene
    N = a.features
    if v.device_count() < 1:
        raise SystemExit("depth_bench needs a GPU: a timing taken anywhere else says nothing")
    L = capi.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    n = 16 + 3 * N
    Mw = min(N, 8)

    def make(sc, B):
        g = v.BatchVIEKF(B, N, sc["params"])
        g.set_stream(stream.cuda_stream)
        for i in range(N):
            g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        for s in range(2):
            g.step(sc["u"][s], sc["dt"], np.ascontiguousarray(sc["z"][s][:, :Mw, :]), np.ascontiguousarray(sc["slot"][:, :Mw]), sc["R"])
        return g

    def inputs(g, B, M, feat):
        """depths [B][M] (and pixels [B][N][2]) at the filter's own prediction, slots 0 .. M-1, per-entry [B] views for route A"""
        slot = np.tile(np.arange(M, dtype=np.int32), (B, 1))
        z = np.stack([g.eval_h(DEPTH, np.full(B, m, np.int32))[:, 0] for m in range(M)], axis=1)
        x = dict(z=torch.tensor(z, device=dev), slot=torch.tensor(slot, device=dev), R=torch.full((1,), R_DEPTH, dtype=torch.float64, device=dev),
                 res=torch.full((B, M), -9, dtype=torch.int32, device=dev))
        x["za"] = [x["z"][:, m].contiguous() for m in range(M)]
        x["sa"] = [x["slot"][:, m].contiguous() for m in range(M)]
        x["ra"] = torch.full((M, B), -9, dtype=torch.int32, device=dev)
        if feat:
            zf = np.stack([g.eval_h(FEAT, np.full(B, m, np.int32))[:, :2] for m in range(N)], axis=1)
            x["zf"] = torch.tensor(np.ascontiguousarray(zf), device=dev)
            x["sf"] = torch.tensor(np.tile(np.arange(N, dtype=np.int32), (B, 1)), device=dev)
            x["rf"] = torch.full((B, N), -9, dtype=torch.int32, device=dev)
        return x

    def tick(name, g, M, x, step):
        if step is not None:
            g.step_n(step[0], step[1], x["zf"], x["sf"], step[2], result=x["rf"])
        if name == "B":
            _, route = g.update_depths(DEPTH, x["z"], x["slot"], x["R"], None, 0, result=x["res"])
            assert route == 1
        else:
            for m in range(M):
                capi.check(L.viekf_batch_update(g._h, DEPTH, C.c_void_p(x["za"][m].data_ptr()), 1, C.c_void_p(x["R"].data_ptr()), 1, 0,
                                                C.c_void_p(x["sa"][m].data_ptr()), None, C.c_void_p(x["ra"][m].data_ptr()), capi.DEVICE))

    def window(name, g, B, M, step):
        x = inputs(g, B, M, step is not None)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.ticks):
            tick(name, g, M, x, step)
        e1.record(stream)
        e1.synchronize()
        res = x["res"] if name == "B" else x["ra"]
        acc = dict(depth=float((res == 0).double().mean().item()))
        if step is not None:
            acc["feat"] = float((x["rf"] == 0).double().mean().item())
        return e0.elapsed_time(e1) / a.ticks, acc

    def med(xs):
        xs = np.array(xs)
        return dict(ms=round(float(np.median(xs)), 5), ms_min=round(float(xs.min()), 5), ms_max=round(float(xs.max()), 5))

    B = a.batch
    sc = scene.make_scene(B, N, 2, seed=11)
    batches = {"A": make(sc, B), "A2": make(sc, B), "B": make(sc, B)}
    gF = make(sc, B)                                                     # (the frame's FEAT half alone: a batch of its own)
    u = torch.tensor(sc["u"][1][None], device=dev)                      # [1, B, 6]
    dt = torch.tensor(sc["dt"][None], device=dev)                       # [1, B]
    Rf = torch.tensor(np.ascontiguousarray(np.asarray(sc["R"], dtype=np.float64)), device=dev)
    fused_bytes = 8 * (n * (n + 1) + N * n) * B
    out = dict(tool="depth_bench", batch=B, features=N, M=N, ticks_per_window=a.ticks, reps=a.reps, kernels=batches["B"].describe(),
               lds_bytes=int(L.viekf_depths_lds_bytes(N, N)), fused_bytes_per_call=fused_bytes, hbm_peak_gbs=HBM_PEAK_GBS)
    order = ["A", "B", "A2"]
    for wname, step in (("frame", (u, dt, Rf)), ("depths_only", None)):
        ms = {k: [] for k in batches}
        accepted = {k: [] for k in batches}
        for r in range(a.warmup + a.reps):
            order = order[1:] + order[:1]
            for k in order:
                t, acc = window(k, batches[k], B, N, step)
                if r >= a.warmup:
                    ms[k].append(t)
                    accepted[k].append(acc)
        A, A2, Bm = med(ms["A"]), med(ms["A2"]), med(ms["B"])
        w = dict(M=N, with_step=step is not None, A=A, A_twin=A2, B=Bm, aa_spread=round(abs(A["ms"] - A2["ms"]) / A["ms"], 4),
                 B_over_A=round(Bm["ms"] / A["ms"], 4),
                 accepted=dict((k, dict((kk, round(float(np.mean([d[kk] for d in vv])), 4)) for kk in vv[0])) for k, vv in accepted.items()))
        if step is None:
            w["fused_hbm_gbs"] = round(fused_bytes / (Bm["ms"] * 1e-3) / 1e9, 1)
            w["fused_hbm_frac"] = round(fused_bytes / (Bm["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        else:                                                            # the frame's FEAT half alone
            fe = []
            for r in range(a.warmup + a.reps):
                x = inputs(gF, B, N, True)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.ticks):
                    gF.step_n(u, dt, x["zf"], x["sf"], Rf, result=x["rf"])
                e1.record(stream)
                e1.synchronize()
                if r >= a.warmup:
                    fe.append(e0.elapsed_time(e1) / a.ticks)
            w["feat_half_alone"] = med(fe)
        out[wname] = w
    # the three batches took the same measurements: the same state at the end, to rounding
    xa, xb = batches["A"].get_state(), batches["B"].get_state()
    out["x_rel_diff_A_vs_B"] = float(np.abs(xa - xb).max() / np.abs(xa).max())
    gB = batches["B"]
    by_m = {}
    for M in (1, 10, 25, 50):
        if M > N:
            continue
        ts = [window("B", gB, B, M, None)[0] for r in range(a.warmup + a.reps)][a.warmup:]
        by_m[str(M)] = med(ts)
    out["by_m"] = by_m
    del batches, gB, gF
    by_batch = {}
    for nb in (256, 512, 1024, 2048):
        scb = scene.make_scene(nb, N, 2, seed=11)
        g = make(scb, nb)
        ts = [window("B", g, nb, N, None)[0] for r in range(a.warmup + a.reps)][a.warmup:]
        by_batch[str(nb)] = med(ts)
        del g
    out["by_batch"] = by_batch
    print(json.dumps(out), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "depth_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
