"""Closed loop: the filter tracks a simulated flight from rendered images.  Simulator.render frames go through KLTTracker and
track_frame (the glue of VIEKF_ROS::color_image_callback) into SeqVIEKF; the estimate must follow the simulator's truth."""
import numpy as np
import pytest

from oracle import oracle as orc
from vi_ekf_amd import sim as S

pytestmark = pytest.mark.gpu


def test_filter_tracks_simulated_flight_from_rendered_images():
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, N, W, H = 4, 12, 640, 480
    p = dict(orc.EKF_YAML)
    p["use_keyframe_reset"] = False
    sim = S.Simulator(p, num_features=N, seed=3, tmax=4.0, cam_rate=30.0)
    g = v.BatchVIEKF(B, N, dict(p, keyframe_overlap_threshold=0.8, name="klt"))
    sg = v.SeqVIEKF(g, state_hist=64, meas_hist=200)
    trk = v.KLTTracker(B, W, H, max_features=N, radius=30)
    masks = np.full((B, H, W), 255, np.uint8)          # four cameras, four masks: four different feature sets
    masks[1, :, :160] = 0
    masks[2, :120, :] = 0
    masks[3, 200:280, 240:400] = 0
    trk.set_mask(masks)
    sg.propagate_state(np.tile(sim.imu(), (B, 1)), sim.t)
    worst = np.zeros(3)
    frames = 0
    while sim.run():
        sg.propagate_state(np.tile(sim.imu(), (B, 1)), sim.t)
        if sim.k % sim.cam_every:
            continue
        img, dmm = sim.render(W, H, depth=True)
        out = v.track_frame(sg, trk, sim.t, np.stack([img] * B), sim.R_pix, depth_mm=np.stack([dmm] * B))
        frames += 1
        for b in range(B):
            n = out["count"][b]
            assert n > 0
            assert not (out["result"][b, :n] == capi.MEAS_NAN).any()
        if sim.t > 1.0:
            x = g.get_state()
            st = sim.state()
            for b in range(B):
                worst = np.maximum(worst, [np.abs(x[b, 0:3] - st[0:3]).max(), np.abs(x[b, 3:6] - st[7:10]).max(),
                                           np.degrees(np.abs(orc.q_boxminus(x[b, 6:10], st[3:7])).max())])
    assert frames >= 120
    _, _, next_id = trk.get_points()
    assert (next_id > N).all()                          # the tracker replenished
    assert not np.isnan(g.get_state()).any()
    # bounds calibrated on the restated stack (tests/klt_ref.Tracker + oracle SeqOracle on the same frames and masks): worst
    # 0.30 m / 0.21 m/s / 2.37 deg over the four cameras after t = 1 s; the position and velocity bounds are those of
    # test_hip_sequencer_on_the_simulator, the attitude bound leaves room above the restated 2.37 deg
    assert worst[0] < 0.6 and worst[1] < 0.4 and worst[2] < 3.5, worst
