"""Compares two hipcc -S listings kernel by kernel: resource numbers (as tools/asm_stats.py reads them, plus sgpr and agpr
counts) and the histogram of instruction mnemonics.  A kernel equal in both is the same code up to register numbering and
instruction order.    python tools/asm_compare.py parent.s new.s [--json out.json]"""
import collections
import json
import re
import sys

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def kernels(path):
    txt = open(path).read()
    out = {}
    for blk in ("  - .agpr_count:" + b for b in txt.split("  - .agpr_count:")[1:]):
        name = re.search(r"\.name:\s+(\S+)", blk)[1]
        out[name] = {"res": {k: re.search(r"\.%s:\s+(\S+)" % k, blk)[1] for k in KEYS}}
    for name, k in out.items():   # the body: from the kernel's label to its .Lfunc_end
        body = txt[txt.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        lines = (l.split(";")[0].strip() for l in body.splitlines()[2:])
        k["hist"] = collections.Counter(l.split()[0] for l in lines if l and not l.endswith(":") and not l.startswith("."))
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
rep = {"equal": [], "different": {}, "only_in_one": sorted(set(a) ^ set(b))}
for name in sorted(set(a) & set(b)):
    if a[name] == b[name]:
        rep["equal"].append(name)
        continue
    d = {k: [a[name]["res"][k], b[name]["res"][k]] for k in KEYS if a[name]["res"][k] != b[name]["res"][k]}
    ha, hb = a[name]["hist"], b[name]["hist"]
    d["instructions"] = [sum(ha.values()), sum(hb.values())]
    d["mnemonics"] = {m: [ha[m], hb[m]] for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m]}
    rep["different"][name] = d
print("%d kernels equal, %d different, %d in one listing only" % (len(rep["equal"]), len(rep["different"]), len(rep["only_in_one"])))
for name, d in rep["different"].items():
    print("DIFF", name[:100], {k: v for k, v in d.items() if k != "mnemonics"}, "%d mnemonics differ" % len(d["mnemonics"]))
if "--json" in sys.argv:
    json.dump(rep, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
