"""tests/frame_ref.py, the restatement the device-resident frame intake (include/viekf_frame.h) is tested against, on its
own: its feature-id bookkeeping is SeqOracle.keep_only_features' (the line-by-line restatement of the reference), and the
restated stack flies the closed loop of tests/test_gpu_frame.py on the CPU, which fixes that test's bounds."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import seq_oracle as so
from tests import frame_ref as F
from tests import sim_ref as R
from vi_ekf_amd import capi, frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The closed loop of tests/test_gpu_frame.py::test_closed_loop_with_nothing_crossing_to_the_host, flown here through the
# restated stack: worst errors after t = 1 s over the four vehicles of sim_ref.LOOP.  Measured on the CPU (this test prints
# them): 0.0908 m, 0.1138 m/s, 0.690 degrees -- inside sim_ref.LOOP_BOUNDS (0.6, 0.4, 2.5), which are therefore the bounds
# of the GPU test as well.
CLOSED_LOOP_BOUNDS = R.LOOP_BOUNDS


def _params(**kw):
    p = dict(orc.EKF_YAML)
    p.update(kw)
    return p


def _pix(gid):
    return np.array([120.0 + 40.0 * (gid % 11), 90.0 + 35.0 * (gid % 9)])


# a scripted sequence of frames, ids handed out by a counter in order of first appearance and never more than the filter holds
# (the reference's init_feature numbers features itself, vi_ekf_feat.cpp:29-30: SeqOracle agrees with a tracker only then):
# fill, drop first / middle / last, grow to the capacity, all new, empty, back again
SCRIPT = [
    [0, 1, 2, 3, 4, 5],
    [1, 2, 3, 4, 5],
    [1, 2, 4, 5],
    [1, 2, 4],
    [1, 2, 4, 6, 7, 8, 9, 10],
    [1, 2, 4, 6, 7, 8, 9, 10],
    [11, 12, 13, 14],
    [11, 12, 13, 14, 15],
    [],
    [16, 17],
    [17, 16, 18],
    [18],
]


@pytest.mark.parametrize("use_kfr", [True, False])
def test_bookkeeping_is_keep_only_features(use_kfr):
    """tracked ids, keyframe list, and whether and when it resets: the restatement against SeqOracle.keep_only_features +
    the new-feature branch of add_measurement, frame by frame"""
    N, p = 8, _params(use_keyframe_reset=use_kfr)
    ref = F.FrameRef(orc.OracleFilter(N).init(**p), 0.8)
    o = so.SeqOracle(orc.OracleFilter(N).init(**p), 0.8, state_hist=8)
    Rm = np.diag([10.0, 10.0])
    resets = []
    for k, ids in enumerate(SCRIPT):
        z = np.array([_pix(g) for g in ids]).reshape(-1, 2)
        out = ref.intake(z, ids, Rm)
        o.keep_only_features(ids)
        for i, gid in enumerate(ids):
            if o.f.global_to_local_feature_id(gid) < 0:
                assert o.add_measurement(0.0, z[i], orc.FEAT, Rm, True, gid) == orc.MEAS_NEW_FEATURE
                assert out["result"][i] == orc.MEAS_NEW_FEATURE
            else:
                assert out["result"][i] in (orc.MEAS_SUCCESS, orc.MEAS_GATED)
        assert ref.tracked() == list(o.f.feature_ids), k
        assert ref.kf == o.keyframe_features, k
        assert ref.resets == len(o.keyframe_edges), k
        assert out["did_reset"] == (len(o.keyframe_edges) > len(resets)), k
        if out["did_reset"]:
            resets.append(k)          # (the edges themselves differ: SeqOracle's filter applied no update)
            assert out["edges"][3] > 0.0
        else:
            assert not out["edges"].any()
    if use_kfr:
        assert resets == [2, 3, 6, 8, 11], resets      # overlaps 4/6, 3/4, 0/3, 0/4, 1/2 < 0.8
    else:
        assert resets == [] and ref.kf == []
    assert ref.tracked() == [18]


def test_padding_repeats_nan_and_overflow():
    N, p = 4, _params(use_keyframe_reset=False)
    ref = F.FrameRef(orc.OracleFilter(N).init(**p))
    Rm = np.diag([10.0, 10.0])
    ids = [5, -1, 6, 5, 7, 8, 9, -1]
    z = np.array([_pix(abs(g)) for g in ids])
    z[4] = np.nan                                   # a NaN on an untracked id: MEAS_NAN, no feature
    out = ref.intake(z, ids, Rm)
    assert list(out["result"]) == [4, -1, 4, 3, 2, 4, 4, -1] and ref.tracked() == [5, 6, 8, 9]
    ids = [9, 8, 10, 6, 5]
    z = np.array([_pix(g) for g in ids])
    z[1] = np.nan                                   # a NaN on a tracked id: it stays, without an update
    z[3] += 300.0                                   # far from where the feature is: gated
    out = ref.intake(z, ids, Rm)
    assert list(out["result"]) == [0, 2, 4, 1, 0] and ref.tracked() == [5, 6, 8, 9]      # (full: 10 finds no slot)
    assert out["gated_count"] == 1 and list(out["gated"]) == [6, -1, -1, -1, -1]


def test_closed_loop_scenario_through_the_restated_intake():
    """the four vehicles of sim_ref.LOOP, N = 8, 2 s at 250 / 25 Hz: ten propagates, then the frame through FrameRef"""
    N, p = 8, _params(use_keyframe_reset=False)
    lm = R.jittered_landmarks(77)
    worst_all = np.zeros(3)
    for sim in R.vehicles(R.LOOP, p, N, lm, tmax=2.0):
        ref = F.FrameRef(orc.OracleFilter(N).init(**p), 0.8)
        clock = {"t": sim.t}

        def imu_cb(t, u, Rm, ref=ref, clock=clock):
            ref.f.propagate(u, t - clock["t"])
            clock["t"] = t

        sim.register_imu_cb(imu_cb)
        sim.register_feat_cb(lambda t, pix, ids, Rm, ref=ref: ref.intake(np.asarray(pix).reshape(-1, 2), list(ids), Rm))
        worst = np.zeros(3)
        while sim.run():
            if sim.k % 10 == 0 and sim.t > 1.0:
                st, x = sim.state(), ref.f.x
                e = [np.abs(x[0:3] - st[0:3]).max(), np.abs(x[3:6] - st[7:10]).max(),
                     np.degrees(np.abs(orc.q_boxminus(x[6:10], st[3:7])).max())]
                worst = np.maximum(worst, e)
        assert not np.isnan(ref.f.x).any()
        assert sim.next_feat_id >= N and len(ref.tracked()) == N
        worst_all = np.maximum(worst_all, worst)
    print("closed loop through the restated intake, worst errors (m, m/s, deg):", worst_all)
    assert (worst_all < np.array(CLOSED_LOOP_BOUNDS)).all(), worst_all
    assert (worst_all > 0).all()


# -- C ABI without a device -----------------------------------------------------------------------------------------------
def test_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "viekf_frame.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_frame_[a-z_0-9]+)\s*\(", txt)))
    assert sorted(frame.FRAME_SYMBOLS) == syms and len(syms) == 6
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    assert int(re.search(r"#define\s+VIEKF_FRAME_MAX_M\s+(\d+)", open(os.path.join(ROOT, "include", "viekf_frame.h")).read()).group(1)) == frame.MAX_M
    assert L.viekf_abi_version() == 1


def test_header_is_plain_c11(tmp_path):
    """tests/c/frame_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    import subprocess
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "frame_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "frame_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "frame header ok" in out.stdout, out.stderr


def test_null_handles_are_refused():
    L = capi.lib()
    assert L.viekf_frame_create(None, None) == capi.ERR_INVALID
    assert L.viekf_frame_destroy(None) == capi.ERR_INVALID
    assert L.viekf_frame_reset(None) == capi.ERR_INVALID
    assert L.viekf_frame_set_tracked(None, None, 0) == capi.ERR_INVALID
    assert L.viekf_frame_tracked(None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_frame_intake(None, 1, None, None, None, None, 0, None, None, None, None, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
