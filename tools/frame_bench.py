"""Time of the device-resident frame intake (include/viekf_frame.h) on one GPU at the headline shape, next to the route that
existed before it for the same frames: the host sequencer's keep_only_features + add_frame + handle_measurements on host
arrays, with the device -> host copies of z and ids it needs.

    python tools/frame_bench.py [--batch 1024] [--features 50] [--reps 30] [--warmup 3] [--out profiles/frame]

One BatchSimulator flies `batch` vehicles; its frames feed two filter stacks side by side, a BatchVIEKF + FrameIntake that
never leaves the device and a BatchVIEKF + SeqVIEKF fed from host arrays.  Both fly 2 s with a frame every 10 ticks first,
so that the timed frames have the simulator's natural share of dropped and new features.  Every timed frame is preceded by
ten IMU ticks (untimed) in both stacks.
  intake     device events on the batch's stream around FrameIntake.intake(sync=False) with device tensors
  unpack     on every other frame a one-element viekf_batch_get_cov_block with a device pointer runs right after the step:
             it needs canonical, mirrored P and so does the intake's unpack and mirror ahead of it.  Timed with the same
             events, it is that share of an intake; the intake behind it (`intake_on_canonical_P`) is the rest.
  sequencer  host clock around z.cpu(), ids.cpu(), keep_only_features, add_frame, handle_measurements (the stream idle before)
Medians of --reps after --warmup, min .. max beside them.  Prints one JSON line and appends it to <out>/frame_bench_run.jsonl.
The per-kernel split comes from a run of its own: rocprofv3 --kernel-trace --stats -- python tools/frame_bench.py --reps 5."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-sequencer", action="store_true", help="the device legs only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, sim as S
    B, N, K = a.batch, a.features, a.ticks
    if v.device_count() < 1:
        raise SystemExit("frame_bench needs a GPU: a timing taken anywhere else says nothing")
    p = v.load_yaml(os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml"))
    pd = p.to_dict()
    rng = np.random.default_rng(7)
    bs = v.BatchSimulator(B, p, max_features=N, seed=np.arange(1, B + 1), radius=rng.uniform(0.35, 1.5, B), period=rng.uniform(6.0, 9.0, B))
    bs.set_landmarks(v.landmarks_like(S.Simulator(pd, seed=1)))
    dev = torch.device("cuda", bs.device)
    stream = torch.cuda.current_stream(dev)
    gd = v.BatchVIEKF(B, N, p)
    gd.set_stream(stream.cuda_stream)
    fi = v.FrameIntake(gd)
    seq = not a.no_sequencer
    if seq:
        gh = v.BatchVIEKF(B, N, p)
        sg = v.SeqVIEKF(gh, state_hist=64, meas_hist=4 * N)
        sg.propagate_state(bs.imu(), 0.0)
    R_host = np.diag([10.0, 10.0])
    R_dev = torch.as_tensor(R_host).to(dev)
    one = torch.zeros(B, dtype=torch.float64, device=dev)
    dt = torch.full((K, B), bs.dt, dtype=torch.float64, device=dev)
    stat = dict(new=[], dropped=[], gated=[])

    def frame(timed, canonical=False):
        """ten ticks, a frame, both stacks -> (intake ms by device events, sequencer ms by the host clock)"""
        u = bs.step(K, device=True)
        z, ids, cnt, dep, _ = bs.camera(N, device=True)
        gd.step_n(u, dt, None, None, None)
        before = fi.tracked(device=True)[1]
        torch.cuda.synchronize(dev)
        ms_u = float("nan")
        if canonical:                                    # (P canonical and mirrored: the intake finds nothing to unpack)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            capi.check(capi.lib().viekf_batch_get_cov_block(gd._h, C.c_int32(0), C.c_int32(0), C.c_int32(1), C.c_int32(1),
                                                            C.c_void_p(one.data_ptr()), C.c_int(capi.DEVICE)))
            e1.record(stream)
            e1.synchronize()
            ms_u = e0.elapsed_time(e1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fi.intake(z, ids, R_dev, sync=False)
        e1.record(stream)
        e1.synchronize()
        ms_d = e0.elapsed_time(e1)
        if timed:
            res = out["result"]
            stat["new"].append(float((res == 4).sum().item()) / B)
            stat["gated"].append(float(out["gated_count"].double().mean().item()))
            stat["dropped"].append(float((before.double().mean() + (res == 4).double().sum() / B - fi.tracked(device=True)[1].double().mean()).item()))
        ms_h = float("nan")
        if seq:
            uh = u.cpu().numpy()
            for i in range(K):
                sg.propagate_state(uh[i], (bs.tick - K + i + 1) * bs.dt)
            sg.handle_measurements()
            gh.sync()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            zh, idh = z.cpu().numpy(), ids.cpu().numpy()
            sg.keep_only_features(idh)
            sg.add_frame(bs.t, zh, R_host, idh)
            sg.handle_measurements()
            gh.sync()
            ms_h = (time.perf_counter() - t0) * 1e3
        return ms_d, ms_h, ms_u

    for _ in range(50):                                  # 2 s of flight with frames: the tables are full and turning over
        frame(False)
    legs = {"intake": [], "sequencer": [], "canonical": [], "unpack": []}
    for r in range(a.warmup + a.reps):
        d, h, _ = frame(r >= a.warmup)
        c, _, un = frame(False, canonical=True)
        if r >= a.warmup:
            legs["intake"].append(d)
            legs["sequencer"].append(h)
            legs["canonical"].append(c)
            legs["unpack"].append(un)

    def med(x):
        x = np.array(x)
        return dict(ms=round(float(np.median(x)), 4), ms_min=round(float(x.min()), 4), ms_max=round(float(x.max()), 4))

    i, s, c, un = med(legs["intake"]), med(legs["sequencer"]), med(legs["canonical"]), med(legs["unpack"])
    ln = dict(tool="frame_bench", batch=B, features=N, reps=a.reps, kernels=gd.describe(), intake=i, intake_on_canonical_P=c,
              unpack_and_mirror=un, unpack_share_of_intake=round(un["ms"] / i["ms"], 3), sequencer_route=s if seq else None,
              sequencer_over_intake=round(s["ms"] / i["ms"], 2) if seq else None,
              new_per_filter_and_frame=round(float(np.mean(stat["new"])), 3), dropped_per_filter_and_frame=round(float(np.mean(stat["dropped"])), 3),
              gated_per_filter_and_frame=round(float(np.mean(stat["gated"])), 3))
    print(json.dumps(ln), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "frame_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
