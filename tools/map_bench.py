"""Time of the device-resident landmark map (include/viekf_map.h) on one GPU at the headline shape, next to the only route
that existed before it for the same numbers: get_state + get_covariance to the host (all of P) and tests/map_ref.py's numpy
per feature slot.

    python tools/map_bench.py [--batch 1024] [--features 50] [--reps 30] [--warmup 3] [--inner 10] [--host-reps 2] [--out profiles/map]

One BatchSimulator flies `batch` vehicles with use_keyframe_reset on (params/ekf.yaml); BatchVIEKF + FrameIntake + NodeGraph +
LandmarkMap take its frames on the device.  2 s of flight with a frame every 10 ticks come first, so that the timed frames see
a steady state: full tables, nodes away from the identity, a filled store.  Every timed frame: ten ticks, step_n, camera,
intake, node update (untimed), then device events on the batch's stream around
  landmarks_first  ONE LandmarkMap.landmarks right after the intake: it includes bringing P to the canonical lower form when
                   the intake's fused FEAT update left it packed
  landmarks        --inner further calls (P canonical), the window divided by --inner
  update           --inner LandmarkMap.update, likewise
  error            --inner LandmarkMap.error, likewise
all with device tensors and sync=False.  Then, on --host-reps of the frames, the host clock (the stream idle before) around
  host_copies      get_state + get_covariance
  host_numpy       tests/map_ref.BatchMapRef.landmarks on them
and the two routes' four outputs are compared (max_abs_diff over the finite entries, the NaN patterns equal).  Medians after
--warmup, min .. max beside them.  Prints one JSON line and appends it to <out>/map_bench_run.jsonl."""
import argparse
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
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from tests import map_ref as MR
    from vi_ekf_amd import sim as S
    B, N, K = a.batch, a.features, a.ticks
    if v.device_count() < 1:
        raise SystemExit("map_bench needs a GPU: a timing taken anywhere else says nothing")
    p = v.load_yaml(os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml"))
    pd = p.to_dict()
    assert pd["use_keyframe_reset"]
    rng = np.random.default_rng(7)
    bs = v.BatchSimulator(B, p, max_features=N, seed=np.arange(1, B + 1), radius=rng.uniform(0.35, 1.5, B), period=rng.uniform(6.0, 9.0, B))
    lm = v.landmarks_like(S.Simulator(pd, seed=1))
    bs.set_landmarks(lm)
    dev = torch.device("cuda", bs.device)
    stream = torch.cuda.current_stream(dev)
    lm_dev = torch.as_tensor(np.ascontiguousarray(lm, dtype=np.float64)).to(dev)
    g = v.BatchVIEKF(B, N, p)
    g.set_stream(stream.cuda_stream)
    fi, ng = v.FrameIntake(g), v.NodeGraph(g)
    mp = v.LandmarkMap(g, fi, ng, a.capacity)
    ref = MR.BatchMapRef(B, N, pd["q_b_c"], pd["p_b_c"])
    R_dev = torch.as_tensor(np.diag([10.0, 10.0])).to(dev)
    dt = torch.full((K, B), bs.dt, dtype=torch.float64, device=dev)
    stat = dict(diff=[], valid=[])

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n, out

    def frame(timed, host):
        u = bs.step(K, device=True)
        z, ids, cnt, dep, lmk = bs.camera(N, device=True)
        g.step_n(u, dt, None, None, None)
        out = fi.intake(z, ids, R_dev)
        ng.update(out, x_true=bs.truth_state(fi.tracked(device=True)[0]))
        if not timed:
            mp.update(sync=True)
            return None
        torch.cuda.synchronize(dev)
        ms = {}
        ms["landmarks_first"], _ = window(lambda: mp.landmarks(device=True, sync=False), 1)
        ms["landmarks"], live = window(lambda: mp.landmarks(device=True, sync=False), a.inner)
        ms["update"], _ = window(lambda: mp.update(sync=False), a.inner)
        ms["error"], err = window(lambda: mp.error(lm_dev, ids, lmk, sync=False), a.inner)
        stat["valid"].append(float((~torch.isnan(err["nees"])).double().mean().item()))
        if host:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            x, P, ln = g.get_state(), g.get_covariance(), g.get_len_features()
            t1 = time.perf_counter()
            node = ng.get()["node"]
            t1b = time.perf_counter()
            rout = ref.landmarks(x, P, ln, node)
            t2 = time.perf_counter()
            ms["host_copies"], ms["host_numpy"] = (t1 - t0) * 1e3, (t2 - t1b) * 1e3
            for k in rout:
                d, r = live[k].cpu().numpy(), rout[k]
                assert np.array_equal(np.isnan(d), np.isnan(r)), k
                stat["diff"].append(float(np.abs(d - r)[~np.isnan(r)].max()))
        return ms

    for _ in range(50):                                      # 2 s of flight with frames
        frame(False, False)
    legs = {}
    for r in range(a.warmup + a.reps):
        ms = frame(True, r >= a.warmup and r - a.warmup < a.host_reps)
        if r >= a.warmup:
            for k, val in ms.items():
                legs.setdefault(k, []).append(val)

    def med(x):
        x = np.array(x)
        return dict(ms=round(float(np.median(x)), 4), ms_min=round(float(x.min()), 4), ms_max=round(float(x.max()), 4), n=int(x.size))

    st = mp.get()
    ln = dict(tool="map_bench", batch=B, features=N, reps=a.reps, inner=a.inner, capacity=a.capacity, kernels=g.describe(),
              valid_slots_with_a_landmark=round(float(np.mean(stat["valid"])), 4), store_entries_filled=round(float((st["ids"] >= 0).mean()), 4),
              resets_total=int(ng.get()["count"].sum()))
    for k in ("landmarks_first", "landmarks", "update", "error", "host_copies", "host_numpy"):
        if k in legs:
            ln[k] = med(legs[k])
    if "host_copies" in legs:
        ln["host_route_over_landmarks"] = round((ln["host_copies"]["ms"] + ln["host_numpy"]["ms"]) / ln["landmarks"]["ms"], 1)
        ln["copies_over_landmarks"] = round(ln["host_copies"]["ms"] / ln["landmarks"]["ms"], 1)
        ln["max_abs_diff"] = float(np.max(stat["diff"]))
    print(json.dumps(ln), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "map_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
