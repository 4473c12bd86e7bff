"""Time of the device-resident node graph (include/viekf_node.h) on one GPU at the headline shape, next to the only route
that existed before it for the same numbers: the intake's edges and the state copied to the host, the pose blocks of P
through viekf_batch_get_cov_block with a host pointer (which has P unpacked and mirrored first), and numpy with
oracle.seq_oracle.xform_mul / xform_adj per filter.

    python tools/node_bench.py [--batch 1024] [--features 50] [--reps 30] [--warmup 3] [--out profiles/node]
    python tools/node_bench.py --check-trace <kernel_trace.csv>

One BatchSimulator flies `batch` vehicles with use_keyframe_reset on (params/ekf.yaml); BatchVIEKF + FrameIntake + NodeGraph
take its frames on the device.  2 s of flight with a frame every 10 ticks come first, so that the timed frames have the
simulator's natural share of resets.  Every timed frame: ten ticks, step_n, intake (untimed), then
  node        device events on the batch's stream around NodeGraph.update(out, x_true) + NodeGraph.global_pose(), device
              tensors, sync=False.  P is in the form the intake's FEAT update left it in.
  host_route  host clock (the stream idle before) around did_reset.cpu(), edges.cpu(), get_state, viekf_batch_get_cov_block
              of rows and columns 0 .. 8 to the host (`copies`), then the numpy node algebra for every filter (`numpy`).
The two routes' poses and covariances are compared on every timed frame (max_abs_diff).  Medians of --reps after --warmup,
min .. max beside them.  Prints one JSON line and appends it to <out>/node_bench_run.jsonl.
The kernel sequence comes from a run of its own: rocprofv3 --kernel-trace --stats -- python tools/node_bench.py
--no-host-route --reps 5; --check-trace reads its kernel trace and fails if a conversion of P -- a launch of the fused step
kernel or k_mirror_upper -- lies between an intake's k_frame_finish and the k_node_global that follows it."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def check_trace(path):
    """every k_node_global of the trace: what ran since the k_frame_finish before it"""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    name = next(k for k in rows[0] if k.lower() == "kernel_name")
    start = next(k for k in rows[0] if k.lower() == "start_timestamp")
    rows.sort(key=lambda r: int(r[start]))
    end = next(k for k in rows[0] if k.lower() == "end_timestamp")
    names = [r[name] for r in rows]

    def short(m):
        return m.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]

    queries, bad, between, last = 0, [], {}, []
    for i, n in enumerate(names):
        if "k_node_global" not in n or "k_node_global_error" in n:
            continue
        j = i - 1
        while j >= 0 and "k_frame_finish" not in names[j]:
            j -= 1
        if j < 0:
            continue
        queries += 1
        k0 = max(k for k in range(j) if "k_frame_plan" in names[k]) if any("k_frame_plan" in m for m in names[:j]) else j
        last = [[short(names[k]), int(rows[k][end]) - int(rows[k][start])] for k in range(k0, i + 1)]
        for m in names[j + 1:i]:
            between[short(m)] = between.get(short(m), 0) + 1
            if "k_step_resident" in m or "k_step_tiles" in m or "k_mirror_upper" in m:
                bad.append(m)
    out = dict(tool="node_bench --check-trace", trace=os.path.basename(path), kernels=len(names), queries_after_an_intake=queries,
               kernels_between_intake_and_query=between, conversions_of_P_between=len(bad), last_frame_from_the_plan_ns=last)
    print(json.dumps(out), flush=True)
    if bad or not queries:
        raise SystemExit("a conversion of P lies between an intake and the global query" if bad else "no query in the trace")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host-route", action="store_true", help="the device leg only (for a kernel trace)")
    ap.add_argument("--check-trace", default=None, help="a rocprofv3 kernel trace (csv) to check instead of running")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node"))
    a = ap.parse_args()
    if a.check_trace:
        check_trace(a.check_trace)
        return
    import torch
    import vi_ekf_amd as v
    from oracle.seq_oracle import xform_adj, xform_mul
    from vi_ekf_amd import capi, sim as S
    B, N, K = a.batch, a.features, a.ticks
    if v.device_count() < 1:
        raise SystemExit("node_bench needs a GPU: a timing taken anywhere else says nothing")
    p = v.load_yaml(os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml"))
    pd = p.to_dict()
    assert pd["use_keyframe_reset"]
    rng = np.random.default_rng(7)
    bs = v.BatchSimulator(B, p, max_features=N, seed=np.arange(1, B + 1), radius=rng.uniform(0.35, 1.5, B), period=rng.uniform(6.0, 9.0, B))
    bs.set_landmarks(v.landmarks_like(S.Simulator(pd, seed=1)))
    dev = torch.device("cuda", bs.device)
    stream = torch.cuda.current_stream(dev)
    g = v.BatchVIEKF(B, N, p)
    g.set_stream(stream.cuda_stream)
    fi, ng = v.FrameIntake(g), v.NodeGraph(g)
    host = not a.no_host_route
    R_dev = torch.as_tensor(np.diag([10.0, 10.0])).to(dev)
    dt = torch.full((K, B), bs.dt, dtype=torch.float64, device=dev)
    hnode, hcov = np.tile(np.array([0.0, 0, 0, 1, 0, 0, 0]), (B, 1)), np.zeros((B, 6, 6))
    blk = np.empty((B, 81))
    idx = [0, 1, 2, 6, 7, 8]
    stat = dict(resets=[], diff=[])

    def host_nodes(dr, eg):
        """viekf_node_update in numpy (vi_ekf_kfr.cpp:147-150)"""
        for b in np.nonzero(dr)[0]:
            Cm = np.zeros((6, 6))
            Cm[:3, :3] = eg[b, 7:16].reshape(3, 3, order="F")
            Cm[5, 5] = eg[b, 16]
            A = xform_adj(hnode[b])
            hcov[b] += A.T @ Cm @ A
            hnode[b] = xform_mul(hnode[b], eg[b, :7])

    def frame(timed):
        u = bs.step(K, device=True)
        z, ids, cnt, dep, _ = bs.camera(N, device=True)
        g.step_n(u, dt, None, None, None)
        out = fi.intake(z, ids, R_dev)
        xt = bs.truth_state(fi.tracked(device=True)[0])
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ng.update(out, x_true=xt, sync=False)
        pose, cov = ng.global_pose(device=True, sync=False)
        e1.record(stream)
        e1.synchronize()
        ms_d = e0.elapsed_time(e1)
        ms_c = ms_n = float("nan")
        if host and not timed:                           # (the host's copy of the nodes keeps up, untimed)
            host_nodes(out["did_reset"].cpu().numpy(), out["edges"].cpu().numpy())
        if host and timed:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dr, eg = out["did_reset"].cpu().numpy(), out["edges"].cpu().numpy()
            x = g.get_state()
            capi.check(capi.lib().viekf_batch_get_cov_block(g._h, C.c_int32(0), C.c_int32(0), C.c_int32(9), C.c_int32(9),
                                                            C.c_void_p(blk.ctypes.data), C.c_int(capi.HOST)))
            t1 = time.perf_counter()
            host_nodes(dr, eg)
            hp, hc = np.empty((B, 7)), np.empty((B, 6, 6))
            for b in range(B):
                Cx = blk[b].reshape(9, 9, order="F")[np.ix_(idx, idx)]
                A = xform_adj(hnode[b])
                hp[b] = xform_mul(hnode[b], np.concatenate([x[b, 0:3], x[b, 6:10]]))
                hc[b] = hcov[b] + A.T @ Cx @ A
            t2 = time.perf_counter()
            ms_c, ms_n = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            stat["diff"].append(max(float(np.abs(pose.cpu().numpy() - hp).max()), float(np.abs(cov.cpu().numpy() - hc).max())))
        if timed:
            stat["resets"].append(float(out["did_reset"].double().mean().item()))
        return ms_d, ms_c, ms_n

    for _ in range(50):                                  # 2 s of flight with frames: the filters have begun to reset
        frame(False)
    legs = {"node": [], "copies": [], "numpy": []}
    for r in range(a.warmup + a.reps):
        d, c, n = frame(r >= a.warmup)
        if r >= a.warmup:
            legs["node"].append(d)
            legs["copies"].append(c)
            legs["numpy"].append(n)

    def med(x):
        x = np.array(x)
        return dict(ms=round(float(np.median(x)), 4), ms_min=round(float(x.min()), 4), ms_max=round(float(x.max()), 4))

    nd = med(legs["node"])
    ln = dict(tool="node_bench", batch=B, features=N, reps=a.reps, kernels=g.describe(), node_update_and_global_pose=nd,
              resets_per_filter_and_frame=round(float(np.mean(stat["resets"])), 4), resets_total=int(ng.get()["count"].sum()))
    if host:
        c, n = med(legs["copies"]), med(legs["numpy"])
        ln.update(host_route_copies=c, host_route_numpy=n, host_route_over_node=round((c["ms"] + n["ms"]) / nd["ms"], 1),
                  copies_over_node=round(c["ms"] / nd["ms"], 1), max_abs_diff=float(np.max(stat["diff"])))
    print(json.dumps(ln), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "node_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
