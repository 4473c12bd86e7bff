"""What per-filter parameter sets cost on one GPU at the headline shape: the fused step of a batch whose filters all have a set
of their own against the same step on the shared set.

    python tools/perfilter_bench.py [--batch 1024] [--features 50] [--reps 40] [--warmup 5] [--ticks 20] [--ones 64]
                                    [--out profiles/perfilter]

Three batches at the same state run step_n(K = 1, M = features), interleaved window by window in the same process with the
order rotating:

  A, A2   two batches on the shared set (the A/A pair: the spread a difference has to beat)
  B       `batch` distinct sets (viekf_batch_set_params_filters): noise, camera, extrinsics and lambda differ per filter;
          lam_feat keeps [1, 1, x], so B runs the unit-Lambda instance A runs

A window is --ticks steps between two device events on the batches' stream; all arguments are device tensors.  Medians of
--reps windows after --warmup, per step, min .. max beside them.  `B_ties_A` says whether |B - A| <= |A - A2|.

Beside it, for scale: what the same sets cost without the feature -- --ones batches of one, one set each, stepped one after
the other through the same call; the time per batch of one times `batch` is reported as `ones_extrapolated_ms` and is an
EXTRAPOLATION, not a measurement of `batch` batches.
Prints one JSON line and appends it to <out>/perfilter_bench_run.jsonl."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def draw_sets(base, B, seed):
    """B sets around `base`: every field the kernels read, within +-20 % (Qu within a factor of 3), quaternions turned by up to
    0.05 rad and renormalised, lambda within (0, 1], lam_feat[0:2] left at 1"""
    r = np.random.default_rng(seed)

    def turned(q):
        d = np.concatenate([[1.0], 0.5 * r.uniform(-0.05, 0.05, 3)])
        q = np.asarray(q, dtype=np.float64)
        w = np.array([q[0] * d[0] - q[1:] @ d[1:], *(q[0] * d[1:] + d[0] * q[1:] + np.cross(q[1:], d[1:]))])
        return w / np.linalg.norm(w)

    sets = []
    for _ in range(B):
        p = dict(base)
        f = lambda: r.uniform(0.8, 1.2)
        p["Qu"] = np.asarray(base["Qu"], dtype=np.float64) * 3.0 ** r.uniform(-1.0, 1.0)
        p["Qx"] = np.asarray(base["Qx"], dtype=np.float64) * f()
        p["Qx_feat"] = np.asarray(base["Qx_feat"], dtype=np.float64) * f()
        p["lam"] = np.minimum(1.0, np.asarray(base["lam"], dtype=np.float64) * r.uniform(0.8, 1.0))
        lf = np.asarray(base["lam_feat"], dtype=np.float64).copy()
        lf[2] = min(1.0, lf[2] * f())
        p["lam_feat"] = lf
        p["P0_feat"] = np.asarray(base["P0_feat"], dtype=np.float64) * f()
        p["cam_center"] = np.asarray(base["cam_center"], dtype=np.float64) * r.uniform(0.95, 1.05)
        p["focal_len"] = np.asarray(base["focal_len"], dtype=np.float64) * f()
        p["q_b_c"], p["q_b_u"] = turned(base["q_b_c"]), turned(base["q_b_u"])
        p["p_b_c"] = np.asarray(base["p_b_c"], dtype=np.float64) * f()
        p["min_depth"] = float(base["min_depth"]) * f()
        sets.append(p)
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ones", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perfilter"))
    a = ap.parse_args()
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import scene
    B, N = a.batch, a.features
    if v.device_count() < 1:
        raise SystemExit("perfilter_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    S = 4
    sc = scene.make_scene(B, N, S, seed=11)
    sets = draw_sets(sc["params"], B, 12)

    def make(params, rows=slice(None)):
        nb = len(params) if isinstance(params, list) else B
        g = v.BatchVIEKF(nb, N, params)
        g.set_stream(stream.cuda_stream)
        for i in range(N):
            g.init_feature(sc["pix"][rows, i, :].copy(), np.full(nb, np.nan))
        return g

    def dev_inputs(rows=slice(None)):
        return dict(u=[torch.tensor(np.ascontiguousarray(sc["u"][s][rows][None]), device=dev) for s in range(S)],
                    dt=torch.tensor(np.ascontiguousarray(sc["dt"][rows][None]), device=dev),
                    z=[torch.tensor(np.ascontiguousarray(sc["z"][s][rows]), device=dev) for s in range(S)],
                    slot=torch.tensor(np.ascontiguousarray(sc["slot"][rows]), device=dev),
                    R=torch.tensor(np.asarray(sc["R"], dtype=np.float64).reshape(2, 2), device=dev))

    def step(g, x, s, res):
        g.step_n(x["u"][s % S], x["dt"], x["z"][s % S], x["slot"], x["R"], result=res)

    batches = {"A": make(sc["params"]), "A2": make(sc["params"]), "B": make(sets)}
    x = dev_inputs()
    res = {k: torch.full((B, N), -9, dtype=torch.int32, device=dev) for k in batches}
    out = dict(tool="perfilter_bench", batch=B, features=N, ticks_per_window=a.ticks, reps=a.reps,
               kernels={k: g.describe() for k, g in batches.items()})
    assert out["kernels"]["A"] == out["kernels"]["B"], out["kernels"]
    ms = {k: [] for k in batches}
    accepted = {k: [] for k in batches}
    order = ["A", "B", "A2"]
    tick = 0
    for r in range(a.warmup + a.reps):
        order = order[1:] + order[:1]
        for k in order:
            g = batches[k]
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for t in range(a.ticks):
                step(g, x, tick + t, res[k])
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                ms[k].append(e0.elapsed_time(e1) / a.ticks)
                accepted[k].append(float((res[k] == 0).double().mean().item()))
        tick += a.ticks

    def med(xs):
        xs = np.array(xs)
        return dict(ms=round(float(np.median(xs)), 5), ms_min=round(float(xs.min()), 5), ms_max=round(float(xs.max()), 5))

    A, A2, Bm = med(ms["A"]), med(ms["A2"]), med(ms["B"])
    out.update(A=A, A_twin=A2, B=Bm, aa_spread=round(abs(A["ms"] - A2["ms"]) / A["ms"], 5),
               B_over_A=round(Bm["ms"] / A["ms"], 5), B_ties_A=bool(abs(Bm["ms"] - A["ms"]) <= abs(A["ms"] - A2["ms"])),
               accepted={k: round(float(np.mean(vv)), 4) for k, vv in accepted.items()},
               status_clean={k: bool((g.get_status() == 0).all()) for k, g in batches.items()})
    for g in batches.values():
        g.close()
    # for scale: the same sets as batches of one, stepped one after the other (an extrapolation to `batch` of them)
    n1 = min(a.ones, B)
    ones = [make([sets[b]], slice(b, b + 1)) for b in range(n1)]
    xs = [dev_inputs(slice(b, b + 1)) for b in range(n1)]
    r1 = torch.full((1, N), -9, dtype=torch.int32, device=dev)
    w = []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for b in range(n1):
            step(ones[b], xs[b], r, r1)
        e1.record(stream)
        e1.synchronize()
        if r >= a.warmup:
            w.append(e0.elapsed_time(e1) / n1)
    one = med(w)
    out.update(ones=n1, one_batch_of_one=one, ones_kernels=ones[0].describe(),
               ones_extrapolated_ms=round(one["ms"] * B, 3), ones_extrapolated_over_B=round(one["ms"] * B / Bm["ms"], 1),
               ones_note="extrapolated from %d batches of one to %d: not a measurement of %d batches" % (n1, B, B))
    print(json.dumps(out), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "perfilter_bench_run.jsonl"), "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
