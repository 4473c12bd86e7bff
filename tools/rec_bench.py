"""Time of the device-resident flight recorder (include/viekf_rec.h) on one GPU at the headline shape, next to the only route
that existed before it for the same numbers: per frame viekf_node_global + viekf_node_global_error into host arrays (a
synchronisation per frame), then tests/rec_ref.py's numpy.

    python tools/rec_bench.py [--batch 1024] [--features 50] [--frames 256] [--reps 20] [--warmup 3] [--inner 5]
                              [--host-filters 32] [--out profiles/rec]

One BatchSimulator flies `batch` vehicles with use_keyframe_reset on (params/ekf.yaml); BatchVIEKF + FrameIntake + NodeGraph
take its frames on the device.  2 s of flight with a frame every 10 ticks come first.  Then `frames` frames fill a recorder
with 5 channels {node NEES, nees[0..3] of consistency}; on every one of them (ticks, step_n, camera, intake, node update,
global pose, global error, consistency: untimed) device events on the batch's stream around
  push             FlightRecorder.push with device tensors, sync=False
and the host clock (the stream idle before) around
  host_per_frame   NodeGraph.global_pose + global_error with host arrays: what a user of the parent commit pays per frame
Then, on the full recorder, device events around --inner calls each (the window divided by --inner), --warmup + --reps times:
  trajectory_none / _yaw / _se3   trajectory_error(delta = 1)
  pose_ensemble, channels
all with device tensors and sync=False, and the host clock around tests/rec_ref.py on the first --host-filters filters
(host_numpy_yaw: trajectory_error("yaw"), per filter in the numpy restatement, so the figure for the batch is that times
batch / host-filters; stated as measured, with the factor beside it), whose results are compared with the device's.
Bytes: what an evaluation must read at least -- passes x batch x frames x 112 for the trajectory call (3 passes with an
alignment, 2 without), batch x frames x 113 for the ensemble, 2 x frames x batch x channels x 8 for the channels -- over its
time, as a share of the 8 TB/s HBM rate (the arrays fit the caches: the share can pass what HBM alone would give).  Medians,
min .. max beside them.  Prints one JSON line and appends it to <out>/rec_bench_run.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-filters", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from tests import rec_ref as RR
    from vi_ekf_amd import sim as S
    B, N, K, T, CH = a.batch, a.features, a.ticks, a.frames, 5
    if v.device_count() < 1:
        raise SystemExit("rec_bench needs a GPU: a timing taken anywhere else says nothing")
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
    fr = v.FlightRecorder(g, T, CH)
    R_dev = torch.as_tensor(np.diag([10.0, 10.0])).to(dev)
    dt = torch.full((K, B), bs.dt, dtype=torch.float64, device=dev)

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n, out

    legs = {}

    def frame(record):
        u = bs.step(K, device=True)
        z, ids, cnt, dep, lmk = bs.camera(N, device=True)
        g.step_n(u, dt, None, None, None)
        out = fi.intake(z, ids, R_dev)
        xt = bs.truth_state(fi.tracked(device=True)[0])
        ng.update(out, x_true=xt)
        if not record:
            return
        pose, _ = ng.global_pose(device=True, cov=False)
        ge = ng.global_error(xt)
        diag = v.consistency(g, ng.relative_truth(xt))
        chan = torch.cat([ge["nees"][:, None], diag["nees"]], dim=1).contiguous()
        torch.cuda.synchronize(dev)
        ms, _ = window(lambda: fr.push(pose, xt, chan=chan, stamp=bs.t, sync=False), 1)
        legs.setdefault("push", []).append(ms)
        xt_h = xt.cpu().numpy()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ng.global_pose(cov=False)
        ng.global_error(xt_h)
        legs.setdefault("host_per_frame", []).append((time.perf_counter() - t0) * 1e3)

    for _ in range(50):                                      # 2 s of flight with frames
        frame(False)
    for _ in range(T):
        frame(True)
    assert fr.count == T
    lo = torch.as_tensor(np.array([1.64, 0.35, 4.17, 9.39, 1.0])).to(dev)
    hi = torch.as_tensor(np.array([12.59, 7.81, 16.92, 28.87, 1e3])).to(dev)
    calls = dict(trajectory_none=lambda: fr.trajectory_error("none", device=True, sync=False),
                 trajectory_yaw=lambda: fr.trajectory_error("yaw", device=True, sync=False),
                 trajectory_se3=lambda: fr.trajectory_error("se3", device=True, sync=False),
                 pose_ensemble=lambda: fr.pose_ensemble(device=True, sync=False),
                 channels=lambda: fr.channels(lo, hi, sync=False))
    last = {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            torch.cuda.synchronize(dev)
            ms, last[k] = window(fn, a.inner)
            if r >= a.warmup:
                legs.setdefault(k, []).append(ms)

    # the route of the parent commit's user, after the per-frame copies: numpy on the host
    rec = fr.get()
    H = max(1, min(a.host_filters, B))
    t0 = time.perf_counter()
    ref = RR.trajectory_error(rec["est"][:H], rec["tru"][:H], rec["valid"][:H], "yaw", delta=1)
    legs["host_numpy_yaw"] = [(time.perf_counter() - t0) * 1e3]
    te = {k: x.cpu().numpy() for k, x in last["trajectory_yaw"].items()}
    assert np.array_equal(te["n_used"][:H], ref["n_used"])
    diff = max(float(np.nanmax(np.abs(te[k][:H] - ref[k]))) for k in ("ate_pos", "ate_att", "rpe_pos", "rpe_att"))

    def med(x):
        x = np.array(x)
        return dict(ms=round(float(np.median(x)), 4), ms_min=round(float(x.min()), 4), ms_max=round(float(x.max()), 4), n=int(x.size))

    bytes_ = dict(trajectory_none=2 * B * T * 112, trajectory_yaw=3 * B * T * 112, trajectory_se3=3 * B * T * 112,
                  pose_ensemble=B * T * 113, channels=2 * T * B * CH * 8, push=B * (2 * 112 + 1 + 2 * CH * 8))
    ln = dict(tool="rec_bench", batch=B, features=N, frames=T, n_channels=CH, reps=a.reps, inner=a.inner, kernels=g.describe(),
              valid_share=round(float(rec["valid"].mean()), 4), resets_total=int(ng.get()["count"].sum()),
              ate_yaw_median_m=round(float(np.nanmedian(te["ate_pos"])), 4), rpe_median_m=round(float(np.nanmedian(te["rpe_pos"])), 5),
              anees_worst=round(float(np.nanmax(last["channels"]["per_frame"][:, 0, 1].cpu().numpy())), 3))
    for k in ("push", "trajectory_none", "trajectory_yaw", "trajectory_se3", "pose_ensemble", "channels", "host_per_frame", "host_numpy_yaw"):
        ln[k] = med(legs[k])
        if k in bytes_:
            ln[k]["bytes"] = bytes_[k]
            ln[k]["share_of_hbm_rate"] = round(bytes_[k] / (ln[k]["ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    ln["host_filters"] = H
    ln["host_numpy_yaw_times_batch_over_host_filters_ms"] = round(ln["host_numpy_yaw"]["ms"] * B / H, 1)
    ln["host_copies_whole_run_ms"] = round(ln["host_per_frame"]["ms"] * T, 2)
    ln["device_whole_run_ms"] = round(ln["push"]["ms"] * T + ln["trajectory_yaw"]["ms"] + ln["pose_ensemble"]["ms"] + ln["channels"]["ms"], 3)
    ln["max_abs_diff_yaw"] = diff
    print(json.dumps(ln), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rec_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
