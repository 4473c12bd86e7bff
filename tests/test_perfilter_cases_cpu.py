"""No-GPU checks of the per-filter parameter sets (viekf_batch_set_params_filters): the cases of tests/perfilter_cases.py meet
their own conditions -- every filter's oracle run uses its own set, no entry is gated, and every varying field of every filter
b > 0 moves the result when it is replaced by filter 0's value --, include/viekf.h declares the two entry points as plain C11,
the library and the Python layer have them, and no kernel reads the parameter pointers of StreamArgs past its accessors."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import perfilter_cases as pc
from vi_ekf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi_ekf_amd", "csrc")
# tests/test_gpu_parity.py holds the GPU to TOL = 1e-9 of max|ref|: a field must move the oracle's result a thousand times that
MOVE = 1e-6
SENSITIVITY_CASES = [(3, 3, None), (12, 5, None), (50, 4, 2)]


def _move(o, c, b):
    return max(np.abs(o[k] - c[k + "_ref"][b]).max() / np.abs(c[k + "_ref"][b]).max() for k in ("x", "P"))


@pytest.mark.parametrize("N,B,nonunit", pc.ORACLE_CASES)
def test_every_filter_runs_on_its_own_set(N, B, nonunit):
    c = pc.case(N, B, nonunit)
    assert len(c["params"]) == B
    for b in range(B):
        p = c["params"][b]
        # the reset state is the set's own x0 and diag(P0 | P0_feat ...)
        assert np.array_equal(c["x0_ref"][b][:17], np.asarray(p["x0"])) and not c["x0_ref"][b][17:].any()
        assert np.array_equal(np.diag(c["P0_ref"][b]), np.concatenate([p["P0"], np.tile(p["P0_feat"], N)]))
        assert (np.asarray(p["lam"]) > 0).all() and (np.asarray(p["lam"]) <= 1).all()
        assert (np.asarray(p["lam_feat"]) > 0).all() and (np.asarray(p["lam_feat"]) <= 1).all()
        for q in ("q_b_c", "q_b_u"):
            assert abs(np.linalg.norm(p[q]) - 1.0) < 1e-15
        assert (p["lam_feat"][0] == 1.0) == (b != nonunit)
        for fld in pc.VARYING:       # at least 10 % from filter 0's, Qu a factor of 3
            if b % 5 == 0:
                continue
            a0, ab = np.asarray(c["params"][0][fld], dtype=np.float64), np.asarray(p[fld], dtype=np.float64)
            if fld == "Qu":
                ratio = ab / a0
                assert (np.maximum(ratio, 1.0 / ratio) >= 3.0 * (1.0 - 1e-5)).all()
            elif fld in ("q_b_c", "q_b_u"):
                assert 2.0 * np.arccos(min(1.0, abs(float(a0 @ ab)))) >= 0.0999
            elif fld == "lam_feat":
                assert abs(ab[2] / a0[2] - 1.0) >= 0.1
            elif fld == "x0":
                body = np.r_[0:6, 10:17]
                assert (np.abs(ab[body] / a0[body] - 1.0) >= 0.1).all()
            else:
                assert (np.abs(ab[a0 != 0] / a0[a0 != 0] - 1.0) >= 0.1).all() and (a0 != 0).any()
    # nothing is gated or refused: every entry is an accepted update, the feature goes into the free slot
    for k, v in c["codes"].items():
        assert (v == (1 if k == "init" else 0)).all(), k
    assert (c["len_ref"] == c["len_kept"]).all() and (c["len_kept"] == N - 1 - (np.arange(B) % 2)).all()
    # the filters differ from one another (a kernel that gives every filter one set cannot match all of them)
    for b in range(1, B):
        assert np.abs(c["x_ref"][b] - c["x_ref"][0]).max() > 1e-3


@pytest.mark.parametrize("N,B,nonunit", SENSITIVITY_CASES)
def test_cases_tell_every_field_of_every_filter_apart(N, B, nonunit):
    c = pc.case(N, B, nonunit)
    for fld in pc.VARYING:
        for b in range(1, B):
            p = dict(c["params"][b])
            p[fld] = c["params"][0][fld]
            o = pc.run_filter(c, b, p)
            for k in o["codes"]:
                assert np.array_equal(o["codes"][k], c["codes"][k][b]), (fld, b, k)     # (no entry gated in any variant)
            assert _move(o, c, b) >= MOVE, "%s of filter %d: the result moves by %.2e only" % (fld, b, _move(o, c, b))
    if nonunit is not None:          # ... and the one filter that is not unit-Lambda from the unit-Lambda set
        p = dict(c["params"][nonunit])
        p["lam_feat"] = np.array([1.0, 1.0, p["lam_feat"][2]])
        assert _move(pc.run_filter(c, nonunit, p), c, nonunit) >= MOVE


def test_tiled_sets_are_all_distinct():
    t = pc.tiled(pc.case(12, 5), 300)
    assert t["B"] == 300 and len(t["params"]) == 300 and t["zA"].shape[0] == 300 and t["u"].shape[1] == 300
    qu = np.stack([p["Qu"] for p in t["params"]])
    assert len({tuple(r) for r in qu}) == 300
    one = pc.one(t, 256)
    assert one["B"] == 1 and np.array_equal(one["zA"][0], t["zA"][256]) and one["params"][0] is t["params"][256]


# -- the C ABI without a device ------------------------------------------------------------------------------------------
def test_header_is_plain_c11(tmp_path):
    """tests/c/params_filters_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "params_filters_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "params_filters_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "params_filters header ok" in out.stdout, out.stderr


def test_library_and_python_layer_have_the_calls():
    import vi_ekf_amd
    L = capi.lib()
    for s in ("viekf_batch_set_params_filters", "viekf_batch_get_params_filter"):
        assert s in capi.SYMBOLS and hasattr(L, s)
    assert L.viekf_abi_version() == 1
    assert L.viekf_batch_set_params_filters(None, None) == capi.ERR_INVALID
    p = capi.Params()
    assert L.viekf_batch_get_params_filter(None, 0, p) == capi.ERR_INVALID
    assert callable(vi_ekf_amd.BatchVIEKF.set_params) and callable(vi_ekf_amd.BatchVIEKF.params_of)
    txt = open(os.path.join(ROOT, "include", "viekf.h")).read()
    assert "share one\n * parameter set" not in txt and re.search(r"#define\s+VIEKF_ABI_VERSION\s+1\b", txt)


def test_kernels_read_the_sets_through_the_accessors_only():
    """Outside viekf_kernel_args.hpp (the accessors) and viekf_batch.hpp (make_args fills the struct), no file under csrc reads
    .dp, .Qx or .lambda of a StreamArgs: every kernel names its StreamArgs `a` or takes it as `const StreamArgs& a`."""
    names = set()
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hpp", ".hip", ".cpp")):
            continue
        txt = open(os.path.join(CSRC, fn)).read()
        names |= set(re.findall(r"\bStreamArgs\s*&?\s*(\w+)\s*[,)=;]", txt))
    assert "a" in names
    pat = re.compile(r"\b(%s)\s*(\.|->)\s*(dp|Qx|lambda)\b" % "|".join(sorted(names)))
    hits = []
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hpp", ".hip", ".cpp")) or fn in ("viekf_kernel_args.hpp", "viekf_batch.hpp"):
            continue
        for i, ln in enumerate(open(os.path.join(CSRC, fn)), 1):
            code = ln.split("//")[0]
            if pat.search(code):
                hits.append("%s:%d: %s" % (fn, i, ln.strip()))
    assert not hits, "\n".join(hits)
    args = open(os.path.join(CSRC, "viekf_kernel_args.hpp")).read()
    for acc in ("prm(int b)", "qx(int b)", "lam(int b)", "int pstride;"):
        assert acc in args, acc
    # the accessors are in use: a tree that reads nothing through them reads no parameters at all
    used = sum(len(re.findall(r"\ba\.(prm|qx|lam)\(", open(os.path.join(CSRC, fn)).read())) for fn in os.listdir(CSRC) if fn.endswith(".hpp"))
    assert used >= 80, used
