"""Times every resident instance of the fused step with the library VIEKF_LIB names (one library per process: run it once per
library, alternating, and compare the files): per instance, at its largest feature count, the launches
  zu / gen        one step (propagate + N updates), unit-Lambda and general-Lambda kernel
  mp_zu / mp_gen  viekf_batch_step_n with K = 3 propagates + N updates (the multi-propagate kernels)
  prop / prop_n   one propagate-only launch; step_n with K = 3 and no measurements
HIP events around `reps` launches, `blocks` times; the figure kept is the median block, in microseconds per launch.
usage: python tools/inst_ab.py OUT.json [B] [reps] [blocks] [kinds] [instances]
kinds / instances: comma-separated launch names / row indices to time (default: all) -- e.g. only the launches whose kernels a
change touches."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import vi_ekf_amd as v  # noqa: E402
from vi_ekf_amd import capi, scene  # noqa: E402

K, STEPS = 3, 6
KINDS = ("zu", "gen", "mp_zu", "mp_gen", "prop", "prop_n")


def main():
    out = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    blocks = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    kinds = sys.argv[5].split(",") if len(sys.argv) > 5 and sys.argv[5] else list(KINDS)
    insts = [int(i) for i in sys.argv[6].split(",")] if len(sys.argv) > 6 and sys.argv[6] else range(len(NMAX))
    assert set(kinds) <= set(KINDS), kinds
    dev = torch.device("cuda:0")
    res = {}
    for inst in insts:
        N = NMAX[inst]
        sc = scene.make_scene(B, N, STEPS, seed=3)
        d = {k: torch.tensor(sc[k], device=dev) for k in ("u", "z", "dt", "slot", "R")}
        uK = torch.stack([d["u"][[(s + k) % STEPS for k in range(K)]] for s in range(STEPS)])     # [STEPS, K, B, 6]
        dtK = d["dt"].unsqueeze(0).repeat(K, 1).contiguous()
        pix = torch.tensor(np.ascontiguousarray(sc["pix"].transpose(1, 0, 2)), device=dev)
        nan = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
        out_codes = torch.empty((B, N), dtype=torch.int32, device=dev)
        for name in kinds:
            g = v.BatchVIEKF(B, N, sc["params"])
            g.set_tuning(capi.TUNE_RES_INSTANCE, inst)
            if name.endswith("gen"):
                g.set_tuning(capi.TUNE_UNIT_LAMBDA, 0)
            g.use_torch_stream()
            for f in range(N):
                g.init_feature(pix[f], nan)
            if name in ("zu", "gen"):
                def fn(s):
                    g.step(d["u"][s], d["dt"], d["z"][s], d["slot"], d["R"], result=out_codes)
            elif name in ("mp_zu", "mp_gen"):
                def fn(s):
                    g.step_n(uK[s], dtK, d["z"][s], d["slot"], d["R"], result=out_codes)
            elif name == "prop":
                def fn(s):
                    g.propagate(d["u"][s], d["dt"])
            else:
                def fn(s):
                    g.step_n(uK[s], dtK, None, None, None)
            for s in range(5):
                fn(s % STEPS)
            torch.cuda.synchronize()
            us = []
            for _ in range(blocks):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for s in range(reps):
                    fn(s % STEPS)
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / reps)
            desc = g.describe()
            assert "k_step_resident" in desc, desc
            res["%d:%s" % (inst, name)] = {"N": N, "us": sorted(us)[len(us) // 2], "blocks": us, "kernel": desc}
            print(inst, N, name, ["%.1f" % x for x in us], flush=True)
    json.dump({"lib": os.environ.get("VIEKF_LIB", "default"), "B": B, "reps": reps, "results": res}, open(out, "w"), indent=1)


# largest feature count of each row of kResInst (viekf_instance_rows.hpp), in row order
NMAX = [15, 22, 25, 38, 43, 47, 50, 29, 41, 50, 57, 67, 72, 77]

if __name__ == "__main__":
    main()
