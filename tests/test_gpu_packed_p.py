"""P kept PACKED between fused launches (VIEKF_TUNE_PACKED_P): the resident family stores the kernel's own register /
LDS image instead of the column-major matrix and loads it back in the next launch; every reader of P unpacks first.

The arithmetic between load and store is untouched, so everything here is compared BIT FOR BIT (np.array_equal on x, P as
get_covariance returns it, len, status and result codes) with the same call sequence on the same library with the switch off --
that path is the canonical one the rest of the suite pins against the oracle.  Where the image does not fit the filter's n * ld
doubles (small N on a wide instance) the library stays canonical: those cases check that fall-back.
"""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from vi_ekf_amd import capi, scene

pytestmark = pytest.mark.gpu

# rows of the resident dispatch table (viekf_instance_rows.hpp; the index VIEKF_TUNE_RES_INSTANCE takes)
I_2_1, I_7_3, I_1_7, I_2_7, I_5_6_2 = 0, 6, 7, 8, 10
GENERAL_LAMBDA = dict(lam_feat=[0.7, 0.85, 0.4], lam=[1.0] * 3 + [0.9] * 3 + [0.8] * 3 + [0.1] * 6 + [0.01])


def _p(a):
    return C.c_void_p(a.ctypes.data)


class Rec:
    """a batch under one setting of the switch, and the record of everything observable after each call"""

    def __init__(self, B, N, packed, inst=None, seed=1, params=None, steps=8):
        self.sc = scene.make_scene(B, N, steps, seed=seed, params=params)
        self.B, self.N = B, N
        g = self.g = v.BatchVIEKF(B, N, self.sc["params"])
        if inst is not None:
            g.set_tuning(capi.TUNE_RES_INSTANCE, inst)
        g.set_tuning(capi.TUNE_PACKED_P, 1 if packed else 0)
        for i in range(N):
            g.init_feature(self.sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        # fix_depth inside the updates, as tests/test_gpu_parity.py sets it up: features just in front of the camera's infinity
        # with a large depth variance correlated with the bearing; noisy pixels push some of them to rho < 0
        x, P = g.get_state(), g.get_covariance()
        for f in range(0, N, 2):
            d = 16 + 3 * f
            x[:, 17 + 5 * f + 4] = 2e-3
            P[:, d + 2, d + 2] = 4.0
            P[:, d + 2, d] = P[:, d, d + 2] = 0.1
            P[:, d + 2, d + 1] = P[:, d + 1, d + 2] = -0.1
        g.set_state(x=x, P=P)
        rng = np.random.default_rng(5)
        self.z = self.sc["z"] + rng.normal(0.0, 1.5, self.sc["z"].shape)
        self.z[1::3, :, 0, 0] += 5000.0          # outliers -> gated
        self.log = []

    def read(self, extra=None):
        g = self.g
        self.log.append((g.get_state(), g.get_covariance(), g.get_len_features(), g.get_status(), extra))

    def note(self, extra):
        self.log.append((None, None, None, None, extra))

    def step(self, s, M=None):
        """one fused step; M: a list of M measurements, entry m = the frame's entry m mod N (slot and pixel stay together)"""
        sc = self.sc
        sl, z = sc["slot"], self.z[s]
        if M is not None:
            idx = np.arange(M) % self.N
            sl, z = np.ascontiguousarray(sl[:, idx]), np.ascontiguousarray(z[:, idx, :])
        return self.g.step(sc["u"][s], sc["dt"], z, sl, sc["R"]).copy()


def same(a, b):
    assert len(a.log) == len(b.log)
    for k, (ra, rb) in enumerate(zip(a.log, b.log)):
        for what, xa, xb in zip(("x", "P", "len", "status", "extra"), ra, rb):
            if xa is None and xb is None:
                continue
            assert np.array_equal(np.asarray(xa), np.asarray(xb), equal_nan=True), "record %d: %s differs" % (k, what)


def both(script, *args, **kw):
    out = []
    for packed in (True, False):
        r = Rec(*args, packed=packed, **kw)
        script(r)
        out.append(r)
    same(out[0], out[1])
    return out


def eight_steps(r):
    for s in range(8):
        res = r.step(s)
        if s in (0, 3, 7):
            r.read(res)
        else:
            r.note(res)


# (B, N, instance, does the image fit): the ragged last tile row and unowned lanes (48, 50 on <7,3>), one worker wave, seven, two
# service waves, features on the body wave (N = 65: the automatic instance), and images that do not fit
CASES = [(3, 50, I_7_3, True), (3, 48, I_7_3, True), (2, 3, I_1_7, False), (2, 12, I_2_1, True), (2, 51, I_5_6_2, True),
         (1, 65, None, True), (2, 1, I_2_1, False),
         # seven worker waves in PACKED form: an odd register count (<1,7>: the last register on its own) and an even one (<2,7>)
         (2, 25, I_1_7, True), (2, 30, I_2_7, True)]


@pytest.mark.parametrize("B,N,inst,fits", CASES)
def test_packed_steps_equal_canonical_steps(B, N, inst, fits):
    a, b = both(eight_steps, B, N, inst=inst, seed=100 + N)
    assert ("P packed" in a.g.describe()) == fits, a.g.describe()
    assert "P canonical" in b.g.describe(), b.g.describe()
    st = a.log[-1][3]
    if N >= 12:
        assert ((st & 4) != 0).any(), "no filter took the negative-depth branch: the scene does not exercise fix_depth"
    res = np.concatenate([np.asarray(r[4]).ravel() for r in a.log])
    assert (res == 1).any() and (res == 0).any(), "the scene has no gated and no accepted update"


@pytest.mark.parametrize("N,inst,fits", [(3, None, False), (12, I_2_1, True)])
def test_general_lambda_instance(N, inst, fits):
    a, _ = both(eight_steps, 2, N, inst=inst, seed=900 + N, params=GENERAL_LAMBDA)
    assert " ZU" not in a.g.describe() and ("P packed" in a.g.describe()) == fits, a.g.describe()


@pytest.mark.parametrize("N,inst", [(3, None), (50, I_7_3)])
def test_step_n_multi_propagate_instances(N, inst):
    def script(r):
        sc = r.sc
        for s in range(0, 6, 3):
            u = np.ascontiguousarray(sc["u"][s:s + 3])
            dt = np.ascontiguousarray(np.tile(sc["dt"], (3, 1)))
            r.read(r.g.step_n(u, dt, r.z[s], sc["slot"], sc["R"]).copy())
        r.read(r.step(6))          # the single-propagate instance loads what the multi-propagate one stored
    both(script, 2, N, inst=inst, seed=40 + N)


def test_readers_and_writers_between_packed_steps():
    B, N = 2, 12
    L = capi.lib()

    def script(r):
        g, sc = r.g, r.sc
        r.read(r.step(0))                                   # get_state / get_covariance after a packed step
        r.read(r.step(1))
        keep = np.ones((B, N), dtype=np.uint8)
        keep[:, 4] = 0
        keep[1, 9] = 0
        r.read(g.keep_features(keep))                       # keep_features
        r.read(r.step(2))
        ok = g.init_feature(sc["pix"][:, 4, :] + 3.0, np.full(B, np.nan))   # init_feature of a freed slot, P packed
        r.read(np.asarray(ok))
        r.read(r.step(3))
        r.read(g.keyframe_reset())                          # keyframe reset
        r.read(r.step(4))
        x = g.get_state()
        x[:, 0:3] += 0.25
        g.set_state(x=x)                                    # set_state of x alone: P stays packed
        r.read(r.step(5))
        r.read(g.get_cov_diag())                            # the diagonal, straight after a packed step
        g.set_kernel(1)                                     # one propagate and one update through the streaming family
        g.propagate(sc["u"][6], sc["dt"])
        r.read(g.update_feat(r.z[6], sc["slot"], sc["R"]).copy())
        g.set_kernel(0)
        r.read(r.step(7))
        mask = np.array([1, 0], dtype=np.uint8)             # a participation mask on one step
        capi.check(L.viekf_batch_set_active(g._h, _p(mask), capi.HOST))
        res = r.step(0)
        capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
        r.read(res[0])
        r.read(r.step(1))
        r.read(r.step(2, M=80))                             # a chunked launch: M > res_mcap(N) = 64
        r.read(r.step(3))

    a, _ = both(script, B, N, inst=I_2_1, seed=17)
    assert "P packed" in a.g.describe()


def test_ring_routes():
    B, N = 2, 12
    L = capi.lib()

    def script(r):
        g, sc = r.g, r.sc
        g.history_resize(5)
        g.snapshot(0)
        capi.check(L.viekf_batch_select(g._h, 0))
        for s in range(1, 4):                               # propagate_to consecutive slots: slot s - 1 -> slot s
            capi.check(L.viekf_batch_propagate_to(g._h, _p(sc["u"][s]), _p(sc["dt"]), s, capi.HOST))
            r.read(g.update_feat(r.z[s], sc["slot"], sc["R"]).copy())
        g.snapshot(4)                                       # the live (packed) slot 3 saved, feature counts with it
        r.read(r.step(4))
        g.restore(4)                                        # an older packed slot into the live one, step, read
        r.read(r.step(4))
        capi.check(L.viekf_batch_select(g._h, 2))           # an older slot of the chain made live (the counts are the batch's own:
        r.read(r.step(5))                                   # only viekf_batch_snapshot writes a slot's, so no restore of those slots)
        g.snapshot(4)                                       # snapshot and restore across a switch of the tuning word
        g.set_tuning(capi.TUNE_PACKED_P, 0)
        r.read(r.step(6))
        g.restore(4)                                        # (the live P is packed again, the launch stores canonical:
        r.read(r.step(6, M=80))                             #  the second chunk must load what the first one stored)
        g.set_tuning(capi.TUNE_PACKED_P, 1 if "packed" in r.desc else 0)
        g.snapshot(0)
        g.restore(0)
        r.read(r.step(7))

    def with_desc(r):
        r.desc = r.g.describe()
        script(r)

    a, _ = both(with_desc, B, N, inst=I_2_1, seed=23)
    assert "P packed" in a.desc


def test_per_filter_mode_entered_from_packed_buffers():
    """per-filter ring copies and live slots entered while a ring slot AND the batch's own buffers hold packed images: every
    packed buffer is unpacked first (the slot loop of canonicalize_all), then back to whole-batch mode through a resize"""
    B, N = 2, 12
    L = capi.lib()

    def script(r):
        g, sc = r.g, r.sc
        g.history_resize(4)
        r.note(r.step(0))
        r.note(r.step(1))
        g.snapshot(1)                                       # a packed ring slot beside the packed live buffers
        r.note(r.step(2))
        live = np.array([0, 3], dtype=np.int32)
        capi.check(L.viekf_batch_snapshot_filters(g._h, _p(live), capi.HOST))
        g.select_filters(live)
        dst = np.array([2, -1], dtype=np.int32)             # filter 0 advances into slot 2, filter 1 stays put
        capi.check(L.viekf_batch_propagate_filters_to(g._h, _p(sc["u"][3]), _p(sc["dt"]), _p(dst), capi.HOST))
        r.read(g.update_feat(r.z[3], sc["slot"], sc["R"]).copy())
        g.history_resize(0)                                 # every filter's live slot goes home: whole-batch mode again
        g.history_resize(4)
        r.read(r.step(4))
        g.snapshot(1)
        g.restore(1)
        r.read(r.step(5))

    a, _ = both(script, B, N, inst=I_2_1, seed=29)
    assert "P packed" in a.g.describe()


@pytest.mark.parametrize("N,inst", [(3, None), (12, I_2_1)])
def test_shared_clock_sequencer_with_a_delayed_frame(N, inst):
    B = 2
    out = []
    for packed in (1, 0):
        sc = scene.make_scene(B, N, 1, seed=61)
        g = v.BatchVIEKF(B, N, dict(sc["params"], keyframe_overlap_threshold=0.8, name="seq"))
        if inst is not None:
            g.set_tuning(capi.TUNE_RES_INSTANCE, inst)
        g.set_tuning(capi.TUNE_PACKED_P, packed)
        sg = v.SeqVIEKF(g, state_hist=16, meas_hist=50)
        rng = np.random.default_rng(7)
        pix = rng.uniform(120, 480, (B, N, 2))
        R = np.eye(2) * 10.0
        log = []
        frame = 0
        for k in range(24):
            t = 0.004 * k
            u = np.tile(np.array([0, 0, -9.80665, 0, 0, 0.0]), (B, 1)) + rng.normal(0, 0.3, (B, 6)) * np.array([1, 1, 1, .05, .05, .05])
            sg.propagate_state(u, t)
            if k == 0:
                sg.add_frame(t, pix, R, np.arange(N))
            if k % 7 == 3:   # three camera frames; the second one is stamped 30 ms back: rewind and replay
                tz = t - (0.03 if frame == 1 else 0.0)
                zf = pix + rng.normal(0, 0.5, (B, N, 2))
                log.append(sg.add_frame(tz, zf, R, np.arange(N)).copy())
                log.append(np.array([len(q) for q in sg.handle_measurements()]))
                log.append(g.get_state())
                log.append(g.get_covariance())
                frame += 1
        assert frame == 3
        log.append(g.get_status())
        out.append(log)
    assert len(out[0]) == len(out[1])
    for k, (xa, xb) in enumerate(zip(*out)):
        assert np.array_equal(xa, xb, equal_nan=True), "record %d differs" % k


def test_unpack_is_an_identity_and_a_read_changes_nothing():
    B, N = 2, 12

    def script(read_between):
        def run(r):
            r.note(r.step(0))
            if read_between:
                P1 = r.g.get_covariance()
                P2 = r.g.get_covariance()
                assert np.array_equal(P1, P2, equal_nan=True)
                assert np.array_equal(P1, P1.transpose(0, 2, 1), equal_nan=True)
            r.read(r.step(1))
        return run

    a = Rec(B, N, packed=True, inst=I_2_1, seed=3)
    script(True)(a)
    b = Rec(B, N, packed=True, inst=I_2_1, seed=3)
    script(False)(b)
    same(a, b)
