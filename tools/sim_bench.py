"""Time of the batched flight simulator (include/viekf_sim.h) on one GPU at the shape the stack it feeds runs at, next to
the route that exists without it: vi_ekf_amd/sim.py, one vehicle at a time in Python and numpy.

    python tools/sim_bench.py [--batch 1024] [--width 640] [--height 480] [--reps 30] [--warmup 3] [--host-vehicles 2] [--out profiles/sim]

  step     viekf_sim_step(K = 10): ten IMU periods of every vehicle in one launch, u on the device
  camera   viekf_sim_camera(50): projection, window, sort and pick of every vehicle, at a steady state reached by flying
           2 s with a frame every 10 ticks first (ten ticks are flown between two timed frames, outside the timed interval)
  render   viekf_sim_render at width x height without and with the depth image, into device tensors
Device legs: device events on the simulator's stream around each call (VIEKF_DEVICE pointers: nothing crosses the bus),
medians of --reps after --warmup.  Host legs: the same work for --host-vehicles vehicles of sim.Simulator on one CPU
thread, timed with a host clock and SCALED to the batch (x batch / vehicles): nobody waits for 1024 of them.
The output floor of render is batch * W * H * (1 + 4) bytes (grey + float depth; 1 byte without depth) at the stream rate
DESIGN.md uses.  Prints one JSON line per leg and appends them to <out>/sim_bench_run.jsonl."""
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
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-vehicles", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, sim as S
    B, W, H, N, K = a.batch, a.width, a.height, a.features, a.ticks
    if v.device_count() < 1:
        raise SystemExit("sim_bench needs a GPU: a timing taken anywhere else says nothing")
    p = v.load_yaml(os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml"))
    pd = p.to_dict()
    rng = np.random.default_rng(7)
    bs = v.BatchSimulator(B, p, max_features=N, seed=np.arange(1, B + 1), radius=rng.uniform(0.35, 1.5, B), period=rng.uniform(6.0, 9.0, B))
    bs.set_landmarks(v.landmarks_like(S.Simulator(pd, seed=1)))
    dev = torch.device("cuda", bs.device)
    stream = torch.cuda.current_stream(dev)
    bs.set_stream(stream.cuda_stream)
    L = bs._L
    ptr = lambda t: C.c_void_p(t.data_ptr())
    d_u = torch.empty((K, B, 6), dtype=torch.float64, device=dev)
    d_z = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
    d_ids = torch.empty((B, N), dtype=torch.int32, device=dev)
    d_cnt = torch.empty(B, dtype=torch.int32, device=dev)
    d_dep = torch.empty((B, N), dtype=torch.float64, device=dev)
    d_lm = torch.empty((B, N), dtype=torch.int32, device=dev)
    d_img = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    d_dmm = torch.empty((B, H, W), dtype=torch.float32, device=dev)

    def fly():
        capi.check(L.viekf_sim_step(bs._h, K, ptr(d_u), capi.DEVICE))

    def frame():
        capi.check(L.viekf_sim_camera(bs._h, N, ptr(d_z), ptr(d_ids), ptr(d_cnt), ptr(d_dep), ptr(d_lm), capi.DEVICE))

    def timed(call, before=None):
        ms = []
        for r in range(a.warmup + a.reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        return dict(ms=round(float(np.median(ms)), 4), ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4), reps=a.reps)

    for _ in range(50):                                  # 2 s of flight with frames: the tracked lists are full and turning over
        fly()
        frame()
    dev_legs = {}
    dev_legs["step"] = timed(fly)
    dev_legs["camera"] = timed(frame, before=fly)
    dev_legs["render"] = timed(lambda: capi.check(L.viekf_sim_render(bs._h, W, H, ptr(d_img), None, capi.DEVICE)))
    dev_legs["render_depth"] = timed(lambda: capi.check(L.viekf_sim_render(bs._h, W, H, ptr(d_img), ptr(d_dmm), capi.DEVICE)))
    tracked = float(d_cnt.cpu().numpy().mean())
    hit = float(torch.isfinite(d_dmm).double().mean().item())

    # the route that exists without the simulator: sim.py, one vehicle at a time, scaled to the batch
    nv = a.host_vehicles
    sims = [S.Simulator(pd, num_features=N, seed=b + 1, radius=0.35 + 0.5 * b) for b in range(nv)]
    for s in sims:                                       # the same steady state: 2 s of flight with frames
        for f in range(50):
            for _ in range(K):
                s._control(); s._step_truth(); s.k += 1; s.t = s.k * s.dt
            s._camera()
    host = {k: [] for k in dev_legs}
    for r in range(a.host_reps):
        t0 = time.perf_counter()
        for s in sims:
            for _ in range(K):
                s._control(); s._step_truth(); s.k += 1; s.t = s.k * s.dt
                s.imu()
        t1 = time.perf_counter()
        for s in sims:
            s._camera()
        t2 = time.perf_counter()
        for s in sims:
            s.render(W, H)
        t3 = time.perf_counter()
        for s in sims:
            s.render(W, H, depth=True)
        t4 = time.perf_counter()
        for k, dt in zip(("step", "camera", "render", "render_depth"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            host[k].append(dt * 1e3 / nv)

    lines = []
    work = dict(step="%d ticks" % K, camera="%d features" % N, render="%dx%d grey" % (W, H), render_depth="%dx%d grey + depth" % (W, H))
    for k, d in dev_legs.items():
        per_vehicle = float(np.median(host[k]))
        ln = dict(tool="sim_bench", leg=k, work=work[k], batch=B, **d, host_ms_per_vehicle=round(per_vehicle, 3),
                  host_ms_scaled_to_batch=round(per_vehicle * B, 1), host_vehicles_timed=nv, host_is_scaled=True,
                  speedup_vs_scaled_host=round(per_vehicle * B / d["ms"], 1))
        if k.startswith("render"):
            nbytes = B * W * H * (5 if k == "render_depth" else 1)
            floor = nbytes / (HBM_TBS * 1e12) * 1e3
            ln.update(bytes_out=int(nbytes), output_floor_ms=round(floor, 4), share_of_output_floor=round(floor / d["ms"], 4),
                      gpixel_per_s=round(B * W * H / d["ms"] / 1e6, 3), frames_per_s=round(B / d["ms"] * 1e3, 1), share_of_rays_hitting=round(hit, 4))
        if k == "camera":
            ln.update(mean_tracked=round(tracked, 2))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sim_bench_run.jsonl"), "a") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
