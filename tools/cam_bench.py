"""Time of the device-resident camera model (include/viekf_cam.h) on one GPU at the headline shapes.

    python tools/cam_bench.py [--batch 1024] [--features 50] [--width 640] [--height 480] [--reps 20] [--warmup 3] [--inner 20]
                              [--host-reps 2] [--out profiles/cam]

Points: `batch` cameras x `features` raw pixels spread over the image of ocam's lens (one shared set; one point in ten is NaN
padding), device tensors, the model on torch's current stream, sync=False.  Device events around --inner back-to-back calls of
  undistort        CameraModel.undistort_points with R (r_mode 0) -> z, R_out, status
  distort          CameraModel.distort_points with the Jacobian
the window divided by --inner.  Beside them, on --host-reps of the repetitions, the only route that existed before for the
same numbers, by the host clock with the stream idle before:
  host_copies      z to the host, z / R_out / status back to the device
  host_numpy       tests/cam_ref.undistort on the batch's points
and the two routes' z and R_out are compared (max_abs_diff over the finite entries, NaN patterns and status equal).

Pixels: `batch` simulator frames of width x height with depth, one lens per camera (so the mask has `batch` images too), one
call per window:
  rectify, distort CameraModel.warp with depth, each direction
  valid_mask       CameraModel.valid_mask
each against its HBM floor: the bytes the call must read and write per camera (warp: grey and depth in and out, 10 bytes per
pixel; mask: 1 byte per pixel) over the measured copy bandwidth of the part, 6.29 TB/s.  The inverse direction and the mask
run Newton per pixel in fp64 and are bound by that, not by memory: iterations per pixel are counted by the restatement on one
camera and the floor of the fp64 pipe (78.6 TFLOP/s) is given next to the memory floor.

Medians after --warmup, min .. max beside them.  Prints one JSON line and appends it to <out>/cam_bench_run.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBS, FP64_TFLOPS = 6.29, 78.6
# fp64 operations of the header's statements (a division counted as one): forward 63, one Newton iteration = forward + 15, the
# solution's forward + 4
FLOP_FORWARD, FLOP_ITER, FLOP_TAIL = 63, 78, 67


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cam"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from tests import cam_ref as CR
    B, M, W, H = a.batch, a.features, a.width, a.height
    if v.device_count() < 1:
        raise SystemExit("cam_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(7)
    sx, sy = W / 640.0, H / 480.0
    ocam = dict(focal=[CR.OCAM["focal"][0] * sx, CR.OCAM["focal"][1] * sy], center=[CR.OCAM["center"][0] * sx, CR.OCAM["center"][1] * sy],
                dist=CR.OCAM["dist"])
    cam = v.CameraModel(B)
    cam.set_stream(stream.cuda_stream)

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n, out

    legs, stat = {}, dict(diff=[])

    def note(k, ms):
        legs.setdefault(k, []).append(ms)

    # -- points ---------------------------------------------------------------------------------------------------------
    cam.set_intrinsics(**ocam)
    kref = CR.make(**ocam)
    z = rng.uniform([0.0, 0.0], [W - 1.0, H - 1.0], (B, M, 2))
    z[rng.uniform(size=(B, M)) < 0.1] = np.nan
    R_pix = np.diag([10.0, 10.0])
    tz, tR = torch.as_tensor(z).to(dev), torch.as_tensor(R_pix).to(dev)
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        ms_u, (dz, dR, ds) = window(lambda: cam.undistort_points(tz, tR, sync=False), a.inner)
        ms_d, _ = window(lambda: cam.distort_points(tz, jacobian=True, sync=False), a.inner)
        if r < a.warmup:
            continue
        note("undistort", ms_u)
        note("distort", ms_d)
        if r - a.warmup < a.host_reps:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            hz = tz.cpu().numpy()
            t1 = time.perf_counter()
            ref = CR.undistort(kref, hz, np.swapaxes(R_pix, -1, -2).reshape(4))
            t2 = time.perf_counter()
            back = [torch.as_tensor(ref[k]).to(dev) for k in ("z", "R_out", "status")]
            torch.cuda.synchronize(dev)
            t3 = time.perf_counter()
            note("host_copies", ((t1 - t0) + (t3 - t2)) * 1e3)
            note("host_numpy", (t2 - t1) * 1e3)
            gz, gR = dz.cpu().numpy(), dR.transpose(-1, -2).contiguous().cpu().numpy().reshape(B, M, 4)
            assert np.array_equal(ds.cpu().numpy(), ref["status"]) and np.array_equal(np.isnan(gz), np.isnan(ref["z"]))
            stat["diff"].append(float(max(np.nanmax(np.abs(gz - ref["z"])), np.nanmax(np.abs(gR - ref["R_out"])))))
            stat["iters_points"] = float(ref["iters"][ref["status"] == CR.OK].mean())
            del back

    # -- pixels ---------------------------------------------------------------------------------------------------------
    p = v.load_yaml(os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml"))
    bs = v.BatchSimulator(B, p, seed=np.arange(1, B + 1), radius=rng.uniform(0.35, 1.5, B), period=rng.uniform(6.0, 9.0, B))
    bs.step(100)
    img, dmm = bs.render(W, H, depth=True, device=True)
    k1 = CR.OCAM["dist"][0] * rng.uniform(0.8, 1.2, B)
    dist = np.tile(np.asarray(CR.OCAM["dist"]), (B, 1))
    dist[:, 0] = k1
    cam.set_intrinsics(focal=ocam["focal"], center=ocam["center"], dist=dist)
    assert cam.sets == B
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        ms_r, _ = window(lambda: cam.warp(img, "rectify", depth=dmm, fill=0, sync=False), 1)
        ms_w, _ = window(lambda: cam.warp(img, "distort", depth=dmm, fill=0, sync=False), 1)
        ms_m, _ = window(lambda: cam.valid_mask(W, H, device=True, sync=False), 1)
        if r >= a.warmup:
            note("rectify", ms_r)
            note("distort_warp", ms_w)
            note("valid_mask", ms_m)
    torch.cuda.synchronize(dev)
    # Newton iterations per pixel, by the restatement on camera 0
    r0 = CR.undistort(CR.make(ocam["focal"], ocam["center"], dist[0]), CR.pixel_grid(W, H))
    iters = float(r0["iters"].mean())
    valid = float((r0["status"] == CR.OK).mean())

    def med(x):
        x = np.array(x)
        return dict(ms=round(float(np.median(x)), 4), ms_min=round(float(x.min()), 4), ms_max=round(float(x.max()), 4), n=int(x.size))

    npx = B * W * H
    floors = dict(rectify=dict(bytes_per_camera=10 * W * H, flop_per_pixel=FLOP_FORWARD),
                  distort_warp=dict(bytes_per_camera=10 * W * H, flop_per_pixel=iters * FLOP_ITER + FLOP_TAIL),
                  valid_mask=dict(bytes_per_camera=W * H, flop_per_pixel=iters * FLOP_ITER + FLOP_TAIL))
    ln = dict(tool="cam_bench", batch=B, features=M, width=W, height=H, reps=a.reps, inner=a.inner, hbm_tb_s=HBM_TBS, fp64_tflops=FP64_TFLOPS,
              newton_iterations_per_pixel=round(iters, 3), pixels_inside_the_model=round(valid, 4),
              newton_iterations_per_point=round(stat.get("iters_points", float("nan")), 3))
    for k in ("undistort", "distort", "host_copies", "host_numpy", "rectify", "distort_warp", "valid_mask"):
        if k in legs:
            ln[k] = med(legs[k])
    for k, f in floors.items():
        hbm_ms = f["bytes_per_camera"] * B / (HBM_TBS * 1e12) * 1e3
        fp_ms = f["flop_per_pixel"] * npx / (FP64_TFLOPS * 1e12) * 1e3
        ln[k].update(bytes_per_camera=f["bytes_per_camera"], hbm_floor_ms=round(hbm_ms, 4), fp64_floor_ms=round(fp_ms, 4),
                     bound="hbm" if hbm_ms >= fp_ms else "fp64", over_hbm_floor=round(ln[k]["ms"] / hbm_ms, 2),
                     over_floor=round(ln[k]["ms"] / max(hbm_ms, fp_ms), 2), achieved_tb_s=round(f["bytes_per_camera"] * B / (ln[k]["ms"] * 1e-3) / 1e12, 3))
    if "host_copies" in legs:
        ln["host_route_over_undistort"] = round((ln["host_copies"]["ms"] + ln["host_numpy"]["ms"]) / ln["undistort"]["ms"], 1)
        ln["max_abs_diff"] = float(np.max(stat["diff"]))
    print(json.dumps(ln), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "cam_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
