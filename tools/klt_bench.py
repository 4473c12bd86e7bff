"""Frame rate of the batched KLT tracker (include/viekf_klt.h) on one GPU.

    python tools/klt_bench.py [--batches 1,256,1024] [--features 12,50] [--frames 40] [--warmup 10] [--size 640x480]

Input frames are device-resident (a panning texture generated once from a seed, per camera a different direction), and in
the steady state about 20 % of the points are replenished per frame (drop_features of every fifth id between frames).  Each
frame is timed with device events around viekf_klt_load_image (device pointers, no host copy inside the frame); the host
drop between frames is outside the timed interval.  Prints one JSON line per configuration and a last summary line.  The
per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/klt_bench.py ...`.

bytes/frame counts what the frame has to move through HBM at least: the input frame, pyramid level 0 written, each coarser
level written and read once, level 0 read by each of the two corner passes; the shared mask stays in the caches.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBS = 6.3      # measured stream rate of one MI355X (README), TB/s


def base_texture(W, H, seed):
    rng = np.random.default_rng(seed)
    xs, ys = np.arange(W), np.arange(H)
    img = 90.0 + 30.0 * np.outer(np.cos(ys / 29.0), np.sin(xs / 37.0))
    for _ in range(int(W * H / 1500)):
        cx, cy, a, s = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(-80, 110), rng.uniform(2.5, 6.0)
        x0, x1 = max(0, int(cx - 5 * s)), min(W, int(cx + 5 * s) + 1)
        y0, y1 = max(0, int(cy - 5 * s)), min(H, int(cy + 5 * s) + 1)
        img[y0:y1, x0:x1] += a * np.outer(np.exp(-(ys[y0:y1] - cy) ** 2 / (2 * s * s)), np.exp(-(xs[x0:x1] - cx) ** 2 / (2 * s * s)))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def bytes_per_frame(B, W, H, ch=1):
    lv, w, h = 0.0, W, H
    for _ in range(3):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= 21 or h <= 21:
            break
        lv += w * h
    return B * (W * H * ch + W * H + 2 * lv + 2 * W * H)


def run(B, MF, W, H, frames, warmup, radius, seed=1):
    import torch
    from vi_ekf_amd import capi
    from vi_ekf_amd.klt import KLTTracker
    dev = torch.device("cuda", 0)
    # a big periodic texture, cropped per camera and frame on the device: camera b pans in its own direction
    big = torch.from_numpy(base_texture(W + 256, H + 256, seed)).to(dev)
    ang = torch.arange(B, device=dev, dtype=torch.float64) * 2.399963
    vx, vy = (3.0 * torch.cos(ang)).round().long(), (3.0 * torch.sin(ang)).round().long()
    total = frames + warmup
    ox = [((64 + k * vx) % 256) for k in range(total)]
    oy = [((64 + k * vy) % 256) for k in range(total)]
    xi = torch.arange(W, device=dev)
    yi = torch.arange(H, device=dev)

    def frame(k):
        X = (ox[k][:, None] + xi[None, :])                                 # [B][W]
        Y = (oy[k][:, None] + yi[None, :])                                 # [B][H]
        return big[Y[:, :, None], X[:, None, :]].contiguous()             # [B][H][W]

    seqf = [frame(k) for k in range(total)]                                # device-resident sequence, made once
    trk = KLTTracker(B, W, H, max_features=MF, radius=radius)
    stream = torch.cuda.current_stream(dev)
    trk.set_stream(stream.cuda_stream)
    L = trk._L
    feats = torch.empty((B, MF, 2), dtype=torch.float64, device=dev)
    ids = torch.empty((B, MF), dtype=torch.int32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    ms, kept = [], []
    for k in range(total):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        capi.check(L.viekf_klt_load_image(trk._h, C.c_void_p(seqf[k].data_ptr()), 1, None, C.c_void_p(feats.data_ptr()),
                                          C.c_void_p(ids.data_ptr()), C.c_void_p(cnt.data_ptr()), capi.DEVICE))
        e1.record(stream)
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
        hid = ids.cpu().numpy()
        c = cnt.cpu().numpy()
        drop = np.where(np.arange(MF)[None, :] % 5 == 4, hid, -1)         # every fifth point: ~20 % replenished next frame
        found = trk.drop_features(drop)
        if k >= warmup:
            kept.append(float(c.mean()))
            kept.append(float(found.sum(1).mean()))
    ms = np.array(ms)
    bpf = bytes_per_frame(B, W, H)
    med = float(np.median(ms))
    floor_ms = bpf / (HBM_TBS * 1e12) * 1e3
    return dict(tool="klt_bench", batch=B, width=W, height=H, max_features=MF, radius=radius, frames=frames,
                ms_per_frame=round(med, 4), ms_min=round(float(ms.min()), 4), fps=round(1e3 / med, 1),
                camera_frames_per_s=round(B * 1e3 / med, 0), bytes_per_frame=int(bpf),
                hbm_floor_ms=round(floor_ms, 4), share_of_hbm_floor=round(floor_ms / med, 3),
                mean_points=round(float(np.mean(kept[0::2])), 2), mean_dropped=round(float(np.mean(kept[1::2])), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,1024")
    ap.add_argument("--features", default="12,50")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--radius", type=int, default=30)
    a = ap.parse_args()
    W, H = (int(s) for s in a.size.split("x"))
    res = []
    for B in [int(s) for s in a.batches.split(",")]:
        for MF in [int(s) for s in a.features.split(",")]:
            r = run(B, MF, W, H, a.frames, a.warmup, a.radius)
            res.append(r)
            print(json.dumps(r), flush=True)
    head = max(res, key=lambda r: (r["batch"], r["max_features"]))
    print(json.dumps(dict(tool="klt_bench", summary=True, headline_batch=head["batch"], headline_features=head["max_features"],
                          ms_per_frame=head["ms_per_frame"], fps=head["fps"], share_of_hbm_floor=head["share_of_hbm_floor"])))


if __name__ == "__main__":
    main()
