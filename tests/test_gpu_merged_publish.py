"""The single-propagate kernels of <7,3> publish the column pair of a measured feature with ONE store body per wave
(res_merged_publish, viekf_fused_lds.hpp): build_resmap's lane pass leaves the lanes of a wave's slots that hold one feature disjoint,
so they move their values into one set of temporaries and three stores serve all of them; a thread's second block of the feature
-- N = 50 leaves one such thread -- stores from its slot as before.  The multi-propagate kernels keep the per-slot statements.
The same values reach the same addresses, so both forms must agree BIT FOR BIT.

Which launch runs which kernel: `propagate` and `step` launch the single-propagate kernel (merged), `step_n` with K = 2 the
multi-propagate kernel (per slot).  Each case advances the same start by two rounds of (two propagates, one list of updates) along

  A  propagate, step          (merged publishing)
  C  step_n with K = 2        (per-slot publishing)

and asserts x, P, len, status and the result codes equal bit for bit; route A is also held to the CPU oracle with the tolerance of
the parity cases (assert_close of tests/test_gpu_parity.py: 1e-9 of max|ref| per array and 1e-6 element-wise).

The instance is forced (TUNE_RES_INSTANCE) at the smallest and the largest N it serves, B = 3; dt and, in the shuffled lists, the
order of the measurements differ between the filters.  The lists: the features forward, reversed and shuffled; the feature(s) of
the thread(s) the map leaves with a repeat, with their neighbours, at the head of the list (published ahead of the loop), in its
middle (published inside the loop) and twice; M = 1 and M = 2 (nothing is published inside the loop); skipped entries (slot -1: at
the head, second, in runs and at the end), measurements of inactive slots and NaN pixels.  Settings vary over unit and general
Lambda and P packed or canonical on entry (<7,3> at N = 26 does not fit the packed image and stays canonical).
"""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import make_oracle
from tests.test_gpu_packed_p import GENERAL_LAMBDA, I_7_3, Rec, same
from tests.test_gpu_parity import assert_close, oracle_params
from tests.test_resmap_cpu import build as build_map

pytestmark = pytest.mark.gpu

B = 3
DT_SCALE = np.array([1.0, 0.5, 1.7])
STEPS = 4


def repeat_features(N):
    """features a worker thread of <7,3> holds in two of its blocks (the second one takes the per-slot store), from the map"""
    rc, m = build_map(N, 7, 3)
    assert rc > 0
    out = set()
    for t in range(m.shape[1]):
        held = {}
        for a in range(m.shape[0]):
            e = int(m[a, t])
            if e >> 16:
                for f in {e & 0xFF, (e >> 8) & 0xFF}:
                    held[f] = held.get(f, 0) + 1
        out |= {f for f, c in held.items() if c > 1}
    return sorted(out)


def order_of(kind, N):
    """[B][M] features in the order they are measured; -1 = a skipped entry"""
    fwd = np.arange(N)
    if kind == "forward":
        o = np.tile(fwd, (B, 1))
    elif kind == "reversed":
        o = np.tile(fwd[::-1], (B, 1))
    elif kind == "shuffled":
        rng = np.random.default_rng(40 + N)
        o = np.stack([rng.permutation(N) for _ in range(B)])
    elif kind == "m1":
        o = np.array([[N - 1], [0], [N // 2]])
    elif kind == "m2":
        o = np.array([[N - 1, 0], [3, 4], [N // 2, N // 2 - 1]])
    elif kind == "repeats":
        # the repeat features (N = 50; features 7 and N - 2 stand in where the map leaves none) and their neighbours: first and
        # second in the list, in its middle, and a second time at its end
        f = (repeat_features(N) + [7, N - 2])[:2]
        near = [g for x in f for g in (x, min(x + 1, N - 1), max(x - 1, 0))]
        rest = [g for g in fwd[::-1] if g not in near]
        half = len(rest) // 2
        lst = near[:2] + rest[:half] + near[2:] + rest[half:] + [f[0], f[1]]
        o = np.tile(np.array(lst), (B, 1))
        o[1] = np.concatenate([o[1, 1:], o[1, :1]])   # another place in the list for filter 1
    elif kind == "skips":
        rng = np.random.default_rng(90 + N)
        o = np.stack([rng.permutation(N) for _ in range(B)])
        o[0, 0] = -1              # the first entry skipped
        o[1, 1] = -1              # the second one: nothing to publish into buffer 1 ahead of the loop but the third
        o[2, 4:9] = -1            # a run
        o[:, -2:] = -1            # the end
        o[1, 10::3] = -1          # every third
    else:
        raise ValueError(kind)
    return o.astype(np.int32)


# settings: (inactive slots, partial update: 1 on with unit Lambda / 0 off / 2 on with general Lambda, packed)
CASES = [(50, "forward", (3, 1, 1)), (50, "reversed", (1, 0, 0)), (50, "shuffled", (0, 2, 0)),
         (50, "repeats", (0, 2, 1)), (50, "repeats", (0, 1, 0)), (50, "m1", (0, 1, 1)), (50, "m2", (0, 2, 1)),
         (50, "skips", (3, 1, 1)), (50, "skips", (2, 2, 0)),
         (26, "forward", (0, 2, 1)), (26, "reversed", (2, 1, 0)), (26, "shuffled", (1, 0, 1)), (26, "repeats", (0, 1, 0)),
         (26, "m1", (0, 2, 0)), (26, "m2", (0, 1, 1)), (26, "skips", (2, 2, 1))]


def make(N, kind, settings):
    idle, partial, packed = settings
    params = dict(use_partial_update=int(partial != 0), Qx=[1e-4] * 16, Qx_feat=[1e-5, 2e-5, 3e-5])
    if partial == 2:
        params.update(GENERAL_LAMBDA)
    r = Rec(B, N, packed=bool(packed), inst=I_7_3, seed=500 + N, steps=STEPS, params=params)
    r.sc["dt"] = r.sc["dt"] * DT_SCALE
    order = order_of(kind, N)
    idx = np.where(order >= 0, N - 1 - order, 0)           # the frame's entry of feature f is N - 1 - f
    r.slot = np.ascontiguousarray(order)
    r.zl = [np.ascontiguousarray(np.take_along_axis(r.z[s], idx[:, :, None], axis=1)) for s in range(STEPS)]
    for s in range(STEPS):   # outliers on live slots (Rec's own sit on frame entry 0, which a list may leave out), and NaN pixels
        r.zl[s][:, 0, 0] += 5000.0 * (s == 1)
        if kind == "skips":
            r.zl[s][0, 3, 1] = np.nan
            r.zl[s][2, 12, :] = np.nan
    if idle:
        keep = np.ones((B, N), dtype=np.uint8)
        keep[:, N - idle:] = 0
        r.g.keep_features(keep)
        assert (r.g.get_len_features() == N - idle).all()
    r.start = (r.g.get_state(), r.g.get_covariance())
    if packed:   # reading P left it canonical: one launch that changes nothing packs it
        r.g.update_feat(r.zl[0], np.full_like(r.slot, -1), r.sc["R"])
    return r


def route_a(r):
    sc = r.sc
    for s in (0, 2):
        r.g.propagate(sc["u"][s], sc["dt"])
        r.read(r.g.step(sc["u"][s + 1], sc["dt"], r.zl[s + 1], r.slot, sc["R"]).copy())


def route_c(r):
    sc = r.sc
    dt2 = np.ascontiguousarray(np.tile(sc["dt"], (2, 1)))
    for s in (0, 2):
        r.read(r.g.step_n(np.ascontiguousarray(sc["u"][s:s + 2]), dt2, r.zl[s + 1], r.slot, sc["R"]).copy())


def oracle_route(r):
    sc = r.sc
    R = np.asarray(sc["R"]).reshape(2, 2)
    nlive = int(r.g.get_len_features()[0])
    fs, log = [], []
    for b in range(B):
        f = make_oracle(r.N, oracle_params(sc["params"]), sc["pix"][b][:nlive])
        f.x[:] = r.start[0][b]
        f.P[:] = r.start[1][b]
        fs.append(f)
    for s in (0, 2):
        codes = np.zeros(r.slot.shape, dtype=np.int32)
        for b, f in enumerate(fs):
            f.propagate(sc["u"][s, b], float(sc["dt"][b]))
            f.propagate(sc["u"][s + 1, b], float(sc["dt"][b]))
            ids = f.feature_ids
            for m, sl in enumerate(r.slot[b]):
                if sl < 0:
                    codes[b, m] = -1
                elif sl >= f.len_features:
                    codes[b, m] = 3
                elif np.isnan(r.zl[s + 1][b, m]).any():   # (a NaN pixel: reported, no update -- as tests/test_gpu_parity.py expects it)
                    codes[b, m] = 2
                else:
                    codes[b, m] = f.update(orc.FEAT, r.zl[s + 1][b, m], R, True, ids[sl])
        log.append((np.stack([f.x.copy() for f in fs]), np.stack([f.P.copy() for f in fs]), codes))
    return log


@functools.lru_cache(maxsize=None)
def run_a(N, kind, settings):
    r = make(N, kind, settings)
    route_a(r)
    r.desc = r.g.describe()
    return r


def test_the_headline_map_leaves_a_second_match():
    """the per-slot store of a thread's second block runs only where the map leaves a repeat: N = 50 must have one for the
    `repeats` lists to reach it (a better map would make this test, not the kernel, out of date)"""
    assert 1 <= len(repeat_features(50)) <= 3 and repeat_features(26) == []


@pytest.mark.parametrize("N,kind,settings", CASES)
def test_merged_equals_per_slot_bit_for_bit(N, kind, settings):
    a = run_a(N, kind, settings)
    assert "k_step_resident<7,3" in a.desc and (" ZU" in a.desc) == (settings[1] != 2), a.desc
    if settings[2] and N == 50:
        assert "P packed" in a.desc, a.desc
    else:
        assert "P canonical" in a.desc, a.desc
    c = make(N, kind, settings)
    route_c(c)
    same(a, c)
    codes = np.concatenate([np.asarray(rec[4]).ravel() for rec in a.log])
    assert (codes == 0).any()
    if kind == "skips":
        assert (codes == -1).any() and (codes == 2).any() and (codes == 3).any(), "no skipped, NaN or inactive-slot entry"


@pytest.mark.parametrize("N,kind,settings", CASES)
def test_merged_against_the_oracle(N, kind, settings):
    a = run_a(N, kind, settings)
    ref = oracle_route(a)
    nx = 17 + 5 * (N - settings[0])
    assert len(a.log) == len(ref) == 2
    for k, ((x, P, _, _, codes), (xr, Pr, cr)) in enumerate(zip(a.log, ref)):
        assert np.array_equal(codes, cr), "round %d: result codes" % k
        assert_close(x[:, :nx], xr[:, :nx], "x after round %d" % k)
        assert_close(P, Pr, "P after round %d" % k)
