"""Time of the consistency diagnostics (include/viekf_diag.h) at the headline shape on one GPU, next to the only route to the
same numbers without them: the covariances to the host and numpy.

    python tools/diag_bench.py [--batch 1024] [--features 50] [--reps 50] [--warmup 5] [--host-reps 3] [--out profiles/diag]

Every timed call follows a headline step (propagate + N feature updates in the fused kernel), so the part of P above the
diagonal is stale, as it is for a user who asks between two frames.
  device   viekf_diag_consistency with device pointers (x_true, logdet, nees, whitened, info all on the device), timed with
           device events around each call on the batch's stream; the step before it is outside the timed interval.
  host     viekf_batch_get_state(P) to host memory -- which first mirrors the lower triangle up (require_P) -- then
           numpy.linalg.cholesky / solve over the batch and the sums, under the process's thread quota; timed with a host
           clock (the copy ends in a synchronise).  e comes from viekf_batch_boxminus and is not counted.
  copy     the bare device-to-host copy of P (a second get_state straight after: nothing left to mirror).
The HBM floor of the device route is one read of the lower triangles, batch * m (m + 1) / 2 * 8 bytes, at the measured
stream rate.  Prints one JSON line per leg and a summary line, and appends them to <out>/diag_bench_run.jsonl."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBS = 6.3      # measured stream rate of one MI355X (README), TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, diag, scene
    B, N = a.batch, a.features
    total = a.warmup + a.reps + 2 * a.host_reps + 2
    sc = scene.make_scene(B, N, total, seed=77)
    g = v.BatchVIEKF(B, N, sc["params"])
    for i in range(N):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    dev = torch.device("cuda", g.device)
    stream = torch.cuda.current_stream(dev)
    g.set_stream(stream.cuda_stream)
    L = diag._bind()
    n, nx, m = g.n, g.nx, 16 + 3 * N
    k = [0]

    def step():
        g.step(sc["u"][k[0]], sc["dt"], sc["z"][k[0]], sc["slot"], sc["R"])
        k[0] += 1

    step()
    x = g.get_state()
    x_true = x.copy()
    x_true[:, 0:3] += 0.01
    d_xt = torch.as_tensor(x_true).to(dev)
    d_ld = torch.empty(B, dtype=torch.float64, device=dev)
    d_ne = torch.empty((B, 4), dtype=torch.float64, device=dev)
    d_wh = torch.empty((B, n), dtype=torch.float64, device=dev)
    d_in = torch.empty(B, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    ms = []
    for r in range(a.warmup + a.reps):
        step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        capi.check(L.viekf_diag_consistency(g._h, p(d_xt), p(d_ld), p(d_ne), p(d_wh), p(d_in), capi.DEVICE))
        e1.record(stream)
        e1.synchronize()
        if r >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    dev_out = dict(logdet=d_ld.cpu().numpy(), nees=d_ne.cpu().numpy(), info=d_in.cpu().numpy())
    bytes_floor = B * m * (m + 1) // 2 * 8
    floor_ms = bytes_floor / (HBM_TBS * 1e12) * 1e3
    med = float(np.median(ms))
    lines = [dict(tool="diag_bench", leg="device", batch=B, features=N, m=m, reps=a.reps, ms=round(med, 4), ms_min=round(float(ms.min()), 4),
                  ms_max=round(float(ms.max()), 4), bytes_floor=int(bytes_floor), hbm_floor_ms=round(floor_ms, 4),
                  share_of_hbm_floor=round(floor_ms / med, 4), pd_failures=int((dev_out["info"] != 0).sum()))]
    print(json.dumps(lines[-1]), flush=True)

    # the route without the diagnostics: P to the host (mirror + copy), numpy on the process's threads
    LL = capi.lib()
    P = np.empty((B, n, n))
    e = np.empty((B, n))
    hp = lambda arr: C.c_void_p(arr.ctypes.data)
    t_route, t_get, t_copy, t_np = [], [], [], []
    host_out = None
    for r in range(a.host_reps):
        step()
        g.sync()
        xs = g.get_state()
        capi.check(LL.viekf_batch_boxminus(g._h, hp(x_true), hp(xs), hp(e), capi.HOST))
        t0 = time.perf_counter()
        capi.check(LL.viekf_batch_get_state(g._h, None, hp(P), None, capi.HOST))
        t1 = time.perf_counter()
        Lc = np.linalg.cholesky(P)              # (P column-major per filter: symmetric, the same matrix either way)
        logdet = 2.0 * np.log(np.diagonal(Lc, axis1=1, axis2=2)).sum(1)
        y = np.linalg.solve(Lc, e[:, :, None])[:, :, 0]
        y2 = y * y
        nees = np.stack([y2[:, :3].sum(1), y2[:, :9].sum(1), y2[:, :16].sum(1), y2.sum(1)], axis=1)
        t2 = time.perf_counter()
        capi.check(LL.viekf_batch_get_state(g._h, None, hp(P), None, capi.HOST))   # nothing left to mirror: the bare copy
        t3 = time.perf_counter()
        t_route.append((t2 - t0) * 1e3); t_get.append((t1 - t0) * 1e3); t_np.append((t2 - t1) * 1e3); t_copy.append((t3 - t2) * 1e3)
        host_out = dict(logdet=logdet, nees=nees)
    lines.append(dict(tool="diag_bench", leg="host", batch=B, features=N, reps=a.host_reps, threads=int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
                      ms=round(float(np.median(t_route)), 2), ms_get_state_P=round(float(np.median(t_get)), 2),
                      ms_numpy=round(float(np.median(t_np)), 2), ms_bare_copy_P=round(float(np.median(t_copy)), 2),
                      bytes_copied=int(B * n * n * 8)))
    print(json.dumps(lines[-1]), flush=True)
    # the two routes at the same state (the last step): they have to agree before their times are compared
    capi.check(L.viekf_diag_consistency(g._h, p(d_xt), p(d_ld), p(d_ne), p(d_wh), p(d_in), capi.DEVICE))
    g.sync()
    rel = float(np.abs(d_ne.cpu().numpy() / host_out["nees"] - 1.0).max())
    dld = float(np.abs(d_ld.cpu().numpy() - host_out["logdet"]).max())
    lines.append(dict(tool="diag_bench", summary=True, batch=B, features=N, device_ms=lines[0]["ms"], host_route_ms=lines[1]["ms"],
                      bare_copy_ms=lines[1]["ms_bare_copy_P"], speedup_vs_host_route=round(lines[1]["ms"] / lines[0]["ms"], 1),
                      share_of_hbm_floor=lines[0]["share_of_hbm_floor"], nees_max_rel_diff=rel, logdet_max_abs_diff=dld))
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "diag_bench_run.jsonl"), "a") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
