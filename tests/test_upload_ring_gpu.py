"""GPU: reuse of the pinned upload rings behind sd_track_set_prior / sd_track_set_measurements (the [max_batch][16] double
ring) and sd_track_set_keyframe_flags / _state / sd_track_set_next_map_id (the [max_batch][8] int32 ring).

Every setter copies its host array into the next of 4 pinned slots and queues the copy to the device on the tracking stream; a
slot is written again only after the copy out of it has run.  Nine calls in a row, with no synchronising call in between, go
more than twice round a ring: every one of the nine values must arrive, byte for byte.  The interleaved case issues 27 uploads
through the two rings in one run.

With nothing else queued on the tracking stream a copy has usually run long before its slot comes round again, so the first
four cases check the cursor, the slot sizes and the destinations, but would rarely notice a missing wait.  The last case
therefore queues a whole TrackWithMotionModel for nine 640x480 frames first: the 27 copies wait behind its kernels while the
host laps the rings, and a slot rewritten before its copy has run (a dropped pending flag, a missing wait, the two rings
sharing slots) delivers a later value to an earlier slot."""
import numpy as np
import pytest

from sdslam_amd import synth

pytestmark = pytest.mark.gpu
B = 9


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


@pytest.fixture()
def trk(sd):
    ext = [sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, B) for _ in range(2)]
    t = sd.Tracker(ext[0], ext[1], max_points=1000, max_batch=B, pnp_max_iterations=4)
    yield t
    t.close()
    for e in ext:
        e.close()


# nine distinct values of each kind (the setters need no extraction)
POSES = [synth.se3_exp((0.01 * f, -0.02 * f, 0.03 + 0.005 * f), (0.1 * f, 0.2 - 0.05 * f, -0.3 * f)) for f in range(B)]
FLAGS = np.array([0x11 + 0x19 * f for f in range(B)], np.uint8)
MEAS = np.array([[f + 0.125 * k + 1e-3 * f * k for k in range(6)] for f in range(B)], np.float64) - 3.0


def check_prior(trk):
    got = trk.get_align(0, B)["T"]
    for f in range(B):
        assert np.asarray(POSES[f], np.float64).tobytes() == got[f].tobytes(), f"slot {f}: the prior differs"


assert len({np.asarray(T, np.float64).tobytes() for T in POSES}) == len(set(FLAGS.tolist())) == len({m.tobytes() for m in MEAS}) == B


def test_prior_ring_laps(trk):
    for f in range(B):
        trk.set_prior(f, [POSES[f]])
    check_prior(trk)


def test_small_ring_laps(trk):
    for f in range(B):
        trk.set_keyframe_flags(f, FLAGS[f:f + 1])
    assert trk.get_keyframe_flags(0, B).tobytes() == FLAGS.tobytes()


def test_measurement_ring_laps(trk):
    trk.set_sensor_model(trk.SENSOR_IMU)
    for f in range(B):
        trk.set_measurements(f, MEAS[f])
    assert trk.get_imu(0, B)["measurements"].tobytes() == MEAS.tobytes()


def interleave_and_check(trk):
    for f in range(B):
        trk.set_prior(f, [POSES[f]])
        trk.set_keyframe_flags(f, FLAGS[f:f + 1])
        trk.set_measurements(f, MEAS[f])
    check_prior(trk)
    assert trk.get_keyframe_flags(0, B).tobytes() == FLAGS.tobytes()
    assert trk.get_imu(0, B)["measurements"].tobytes() == MEAS.tobytes()


def test_interleaved(trk):
    trk.set_sensor_model(trk.SENSOR_IMU)
    interleave_and_check(trk)


def test_interleaved_behind_queued_tracking(trk):
    s = synth.make_scene(20)
    trk.cur.extract_batch(np.repeat(s["cur"][None], B, 0))
    rk, rd, rn = trk.ref.extract_batch(np.repeat(s["ref"][None], B, 0))
    trk.set_camera(synth.FX, synth.FY, synth.CX, synth.CY, 0.0, (0.0, 640.0, 0.0, 480.0))
    trk.set_last(0, [synth.tracking_case(20, rk[0, :rn[0]], rd[0, :rn[0]])] * B)
    trk.set_poses(0, [s["T_ref"]] * B, [s["T_cur"]] * B)
    trk.set_sensor_model(trk.SENSOR_IMU)
    trk.track_with_motion_model(B, th=8.0, mono=True, align_mode=0)   # queued, not waited for
    interleave_and_check(trk)
    assert (trk.get_tracked(0, B)["status"] == 2).all()              # the work the copies queued behind did run
