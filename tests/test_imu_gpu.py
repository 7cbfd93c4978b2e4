"""GPU: the IMU sensor model on the device (sd_track_set_sensor_model, sd_track_set_measurements, sd_track_get_imu / _set_imu,
and sd_track_motion_predict / _update / _restart under SD_SENSOR_IMU).

The per-slot 16-state filter equals tests/imu_ref.py (the reference's dense EKF + IMU in numpy) fed the same poses and
measurements; unstarted and restarted slots get the last pose as prior; lost slots restart; the two models switch and refuse
each other's accessors; a saved filter continues bytewise; the device's prior drives the closed loop to the results of the
loop driven by the numpy filter's priors, queued or synchronised.

Bound of the float comparisons: 64 x the float64 / longdouble gap of tests/imu_ref.py on exactly these slot inputs
(tests/imu_cases.py: noise_floor()), measured by the machine that runs the test.  The factor covers a different but equally
valid operation order and pivoting on the device and a few ulp of sin / cos.  Measured when this was written: gap 2.36e-15
(slot 30, step 5), bound 1.51e-13; largest deviation of the device measured on the MI355X 3.98e-15 (n = 70 and n = 5).  Flags and it_time are
compared exactly."""
import numpy as np
import pytest

import imu_cases as IC
import imu_ref as R
import motion_ref as MR
import test_sequence_gpu as SQ
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
DT = 1.0 / 30.0
B70 = IC.B
TINY = (50, 1.2, 1, 20, 64, 64)          # a small extractor geometry the plan accepts: the filter calls read no image
X0 = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.float64)
P0 = np.diag([R.COV_X_2] * 3 + [R.COV_Q_2] * 4 + [R.COV_V_2] * 3 + [R.COV_W_2] * 3 + [R.COV_A_2] * 3)
_BLK = np.repeat(np.arange(5), [3, 4, 3, 3, 3])
BLOCKS = _BLK[:, None] == _BLK[None, :]   # the diagonal blocks of P, which IMU::Init assigns


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


@pytest.fixture(scope="module")
def tol():
    return 64.0 * IC.noise_floor()


@pytest.fixture(scope="module")
def streams():
    s = [IC.stream(i) for i in range(B70)]
    assert min(IC.trace_margin(p) for p, _ in s) > 1.0
    return [p for p, _ in s], np.stack([m for _, m in s])               # poses [70][9], measurements [70][8][6]


def make_tracker(sd):
    ext = [sd.ORBextractor(*TINY, B70) for _ in range(2)]
    return sd.Tracker(ext[0], ext[1], max_points=8, max_batch=B70, pnp_max_iterations=4), ext


@pytest.fixture()
def trk70(sd):
    trk, ext = make_tracker(sd)
    yield trk
    trk.close()
    for e in ext:
        e.close()


def check_state(im, refs, n, key, tol):
    """Device state of slots < n against the reference filters, slots >= n against a filter nobody touched (exactly)."""
    worst = 0.0
    for i in range(B70):
        f = refs[i] if i < n else R.EKF()
        assert im["started"][i] == int(f.started()), (key, i)
        assert im["it_time"][i] == f.it_time, (key, i)
        d = max(np.abs(im["X"][i] - f.X).max(), np.abs(im["P"][i] - f.P).max(), np.abs(im["gravity"][i] - f.gravity).max())
        assert d <= (tol if i < n else 0.0), (key, i, IC.slot_params(i)["kind"], d)
        worst = max(worst, d)
    return worst


def step(trk, refs, poses, meas, k, n, tol, key, kept=None):
    """One predict + update of slots < n at step k on device and reference; returns (largest deviation, prior, state)."""
    T, T2 = [p[k] for p in poses], [p[k + 1] for p in poses]
    kept = T if kept is None else kept
    trk.set_poses(0, T, kept)
    trk.set_measurements(0, meas[:n, k])
    trk.motion_predict(n, IC.DTS[k])
    prior, im = trk.get_align(0, B70)["T"], trk.get_imu(0, B70)
    worst = 0.0
    for i in range(B70):
        if i >= n:
            assert np.array_equal(prior[i], kept[i]) and not im["last_pose"][i].any() and not im["measurements"][i].any(), (key, k, i)
            continue
        was_started = refs[i].started()
        want = refs[i].predict(T[i], IC.DTS[k])
        d = np.abs(prior[i] - want).max()
        assert d <= tol, (key, k, i, d)
        if not was_started:
            assert prior[i].tobytes() == T[i].tobytes(), (key, k, i)
        worst = max(worst, d)
        assert np.array_equal(im["last_pose"][i], T[i]) and np.array_equal(im["measurements"][i], meas[i, k]), (key, k, i)
    worst = max(worst, check_state(im, refs, n, (key, "predict", k), tol))
    trk.set_poses(0, T, T2)                                              # the "tracked" pose of this frame in Tcur
    trk.motion_update(n, -1)
    for i in range(n):
        refs[i].track(T2[i], meas[i, k])
    im = trk.get_imu(0, B70)
    worst = max(worst, check_state(im, refs, n, (key, "update", k), tol))
    return worst, prior, im


@pytest.mark.parametrize("n", [B70, 5])
def test_filter_matches_reference(trk70, streams, tol, n):
    """70 slots x 8 steps, each slot its own (v, w, a) (tests/imu_cases.py: w = 0 exactly, a w that starts later, a
    gravity-sized a; dt = 1/30 and 0.1 alternating and one dt = 0): after every predict and every update X, the full P,
    gravity, started, it_time and the prior equal the dense reference filter; slots >= n equal an untouched filter exactly."""
    trk = trk70
    poses, meas = streams
    trk.set_sensor_model(1)
    assert trk.get_sensor_model() == 1
    refs = [R.EKF() for _ in range(B70)]
    kept = [np.eye(4) * (i + 2) for i in range(B70)]                    # what set_poses leaves in Tprior: slots >= n keep it
    worst = 0.0
    for k in range(len(IC.DTS)):
        w, _, _ = step(trk, refs, poses, meas, k, n, tol, "parity", kept)
        worst = max(worst, w)
    print(f"IMU filter, n = {n}: largest deviation from the reference {worst:.3e}, bound {tol:.3e}")
    # the filters arrived somewhere: velocities learnt, P dense, both branches of dq_by_dw taken (state w = 0 at the first
    # prediction, non-zero later)
    for i in range(n):
        p = IC.slot_params(i)
        assert np.abs(refs[i].P[~BLOCKS]).max() > 1e-9, i
        if p["kind"] != 2:                                              # (a gravity-sized a biases the state's a and with it v)
            assert np.abs(refs[i].X[7:10] - p["v"]).max() < 0.05, i
        if p["kind"] != 0:
            assert np.abs(refs[i].X[10:13]).max() > 1e-3, i
        if p["kind"] == 2:
            assert refs[i].gravity[1] > 1.0, i


@pytest.mark.parametrize("n", [B70, 5])
def test_unstarted_prior_is_the_last_pose(trk70, streams, tol, n):
    """A new handle under the IMU model and a restarted one: Tprior = Tref bit for bit, X and P untouched, started = 0; slots
    >= n keep state and prior; motion_restart touches its range only (IMU::Init: X, gravity and the diagonal blocks of P)."""
    trk = trk70
    poses, meas = streams
    trk.set_sensor_model(1)
    Tref, eye = [p[0] for p in poses], [np.eye(4)] * B70
    trk.set_poses(0, Tref, eye)
    trk.motion_predict(n, DT)
    got, im = trk.get_align(0, B70)["T"], trk.get_imu(0, B70)
    for i in range(B70):
        assert got[i].tobytes() == (Tref[i] if i < n else np.eye(4)).tobytes(), i
        assert np.array_equal(im["last_pose"][i], Tref[i] if i < n else np.zeros((4, 4))), i
        assert np.array_equal(im["X"][i], X0) and np.array_equal(im["P"][i], P0), i
    assert not im["started"].any() and not im["it_time"].any() and not im["gravity"].any()
    refs = [R.EKF() for _ in range(B70)]
    for k in range(3):                                                   # start the filters, give them velocities
        _, _, im = step(trk, refs, poses, meas, k, n, tol, "start")
    assert im["started"][:n].all() and not im["started"][n:].any()
    assert all(np.abs(im["P"][i][~BLOCKS]).max() > 0 for i in range(n)) and np.array_equal(im["P"][n:], np.tile(P0, (B70 - n, 1, 1)))
    trk.motion_restart(2, 3)                                             # slots 2..4 only
    after = trk.get_imu(0, B70)
    for i in range(B70):
        if 2 <= i < 5:
            assert after["started"][i] == 0 and np.array_equal(after["X"][i], X0) and not after["gravity"][i].any(), i
            assert np.array_equal(after["P"][i][BLOCKS], P0[BLOCKS]) and np.array_equal(after["P"][i][~BLOCKS], im["P"][i][~BLOCKS]), i
        else:
            for key in ("X", "P", "gravity", "started"):
                assert np.array_equal(after[key][i], im[key][i]), (i, key)
    trk.motion_restart(0, n)
    T = [p[3] for p in poses]
    trk.set_poses(0, T, eye)
    trk.motion_predict(n, DT)
    got, im2 = trk.get_align(0, B70)["T"], trk.get_imu(0, B70)
    for i in range(B70):
        assert got[i].tobytes() == (T[i] if i < n else np.eye(4)).tobytes(), i
        assert np.array_equal(im2["X"][i], X0) and np.array_equal(im2["P"][i][BLOCKS], P0[BLOCKS]), i
    assert not im2["started"].any() and not im2["it_time"].any()


def test_model_switch_and_errors(trk70, streams, tol):
    """Model 0 is the default and reproduces tests/motion_ref.py; switching restarts the filters of the model switched to; the
    cross-model accessors and the other documented errors return SD_ERR_INVALID_ARG and change nothing."""
    import sdslam_amd as sd
    trk = trk70
    poses, meas = streams
    assert trk.get_sensor_model() == 0
    cv = [MR.EKF() for _ in range(B70)]
    for k in range(3):
        T, T2 = [p[k] for p in poses], [p[k + 1] for p in poses]
        trk.set_poses(0, T, T2)
        trk.motion_predict(B70, DT)
        prior = trk.get_align(0, B70)["T"]
        for i in range(B70):
            assert np.abs(prior[i] - cv[i].predict(T[i], DT)).max() <= 1e-12, (k, i)
        trk.set_poses(0, T, T2)
        trk.motion_update(B70, -1)
        for i in range(B70):
            cv[i].track(T2[i])
    mo = trk.get_motion(0, B70)
    assert mo["started"].all()
    for i in range(B70):
        assert max(np.abs(mo["X"][i] - cv[i].X).max(), np.abs(mo["P"][i] - np.diag(cv[i].P)).max()) <= 1e-12, i

    def snapshot():
        s = trk.get_imu(0, B70)
        s["prior"] = trk.get_align(0, B70)["T"]
        s["model"] = trk.get_sensor_model()
        return s

    def refused(call, *args, **kw):
        before = snapshot()
        with pytest.raises(sd.SdError) as e:
            call(*args, **kw)
        assert e.value.code == 1, (call.__name__, args)
        after = snapshot()
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key])), (call.__name__, args, key)

    # under model 0
    refused(trk.set_measurements, 0, meas[:, 0])
    refused(trk.set_imu, 0, X=np.tile(X0, (2, 1)))
    refused(trk.set_sensor_model, 2)
    refused(trk.set_sensor_model, -1)
    mo_before = trk.get_motion(0, B70)
    trk.set_sensor_model(1)
    im = trk.get_imu(0, B70)
    assert not im["started"].any() and np.array_equal(im["X"], np.tile(X0, (B70, 1))) and np.array_equal(im["P"], np.tile(P0, (B70, 1, 1)))
    # under model 1
    refused(trk.get_motion, 0, B70)
    refused(trk.set_motion, 0, X=np.zeros((2, 6)))
    refused(trk.motion_update, B70, -1)                                  # measurements never set since the model was chosen
    bad = meas[:, 0].copy()
    bad[3, 4] = np.nan
    refused(trk.set_measurements, 0, bad)
    bad[3, 4] = np.inf
    refused(trk.set_measurements, 0, bad)
    trk.set_measurements(0, meas[:5, 0])
    refused(trk.motion_update, 6, -1)                                    # slot 5 has none yet
    refused(trk.motion_predict, 5, -1.0)
    refused(trk.motion_update, 5, 2)
    refs = [R.EKF() for _ in range(B70)]
    for k in range(3):
        step(trk, refs, poses, meas, k, B70, tol, "switch")
    im = trk.get_imu(0, B70)
    assert im["started"].all() and all(np.abs(im["P"][i][~BLOCKS]).max() > 0 for i in range(B70))
    # back to 0: the constant-velocity filters restart (they kept their state while the IMU model ran), the IMU state stays
    trk.set_sensor_model(0)
    mo = trk.get_motion(0, B70)
    assert mo_before["started"].all() and not mo["started"].any() and not mo["X"].any()
    assert np.array_equal(mo["P"], np.tile([MR.COV_V_2] * 3 + [MR.COV_W_2] * 3, (B70, 1)))
    refused(trk.set_measurements, 0, meas[:, 0])
    # and to 1 again: a newly constructed filter, all of P at Init, measurements to be set again
    trk.set_sensor_model(1)
    im = trk.get_imu(0, B70)
    assert not im["started"].any() and np.array_equal(im["X"], np.tile(X0, (B70, 1))) and np.array_equal(im["P"], np.tile(P0, (B70, 1, 1)))
    assert not im["gravity"].any()
    refused(trk.motion_update, B70, -1)


def test_save_and_restore_continues_bytewise(sd, trk70, streams, tol):
    """Steps 0..7 on one handle, against steps 0..3 there, sd_track_get_imu, sd_track_set_imu on a fresh handle and steps 4..7
    on that one: priors and states equal byte for byte."""
    poses, meas = streams
    trk70.set_sensor_model(1)
    refs = [R.EKF() for _ in range(B70)]
    full = []
    for k in range(len(IC.DTS)):
        _, prior, im = step(trk70, refs, poses, meas, k, B70, tol, "full")
        full.append((prior, im))
        if k == 3:
            saved = im
    trk2, ext2 = make_tracker(sd)
    try:
        trk2.set_sensor_model(1)
        trk2.set_imu(0, X=saved["X"], P=saved["P"], gravity=saved["gravity"], started=saved["started"], it_time=saved["it_time"])
        refs2 = [R.EKF() for _ in range(B70)]
        for i in range(B70):
            f = refs2[i]
            f.X, f.P, f.gravity = saved["X"][i].copy(), saved["P"][i].copy(), saved["gravity"][i].copy()
            f.updated, f.it_time = bool(saved["started"][i]), float(saved["it_time"][i])
        for k in range(4, len(IC.DTS)):
            _, prior, im = step(trk2, refs2, poses, meas, k, B70, 2 * tol, "resumed")
            assert np.asarray(prior).tobytes() == np.asarray(full[k][0]).tobytes(), k
            for key in ("X", "P", "gravity", "started", "it_time", "measurements"):
                assert im[key].tobytes() == full[k][1][key].tobytes(), (k, key)
    finally:
        trk2.close()
        for e in ext2:
            e.close()


# ---- closed loops on image sequences

A_CONST = np.array([0.05, -0.03, 0.02])


def gyro_from_poses(Ts):
    """w_k = 2 log(q_{k-1}^-1 (x) q_k) / dt from the ground-truth poses; row 0 is unused."""
    out = np.zeros((len(Ts), 3))
    for k in range(1, len(Ts)):
        q0, q1 = (MR.quat_normalize(MR.mat_to_quat(T[:3, :3])) for T in (Ts[k - 1], Ts[k]))
        d = R.quat_mul(q0 * np.array([1.0, -1.0, -1.0, -1.0]), q1)
        nv = np.linalg.norm(d[1:])
        out[k] = 0.0 if nv == 0.0 else 2.0 * np.arctan2(nv, d[0]) * d[1:] / nv / DT
    return out


@pytest.fixture()
def cached_sequences(monkeypatch):
    """The loops of one test share their rendered sequences."""
    made, make = {}, synth.make_sequence

    def cached(seed, n_frames, **kw):
        key = (seed, n_frames, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(seed, n_frames, **kw)
        return made[key]
    monkeypatch.setattr(synth, "make_sequence", cached)


class ILoop(SQ.Loop):
    """The loop of tests/test_sequence_gpu.py under the IMU model.  mode "device": motion_predict / motion_update; "host": the
    priors of tests/imu_ref.py through set_prior(relative = False)."""

    def __init__(self, sd, oracle, seeds, T, a=A_CONST):
        super().__init__(sd, oracle, SQ.CFGS["p8"], seeds, T)
        self.meas = np.stack([np.concatenate([gyro_from_poses(s["T"]), np.tile(a, (T, 1))], 1) for s in self.seqs], 1)   # [T][B][6]
        self.refs = [R.EKF() for _ in range(self.B)]
        self.Tref = [s["T"][0] for s in self.seqs]
        self.trk.set_sensor_model(1)

    def imu_step(self, t, mode, sync=False, source=1, blank=(), want_prior=False):
        trk, B = self.trk, self.B
        views = self.views[t]
        if blank:
            views = views.copy()
            views[list(blank)] = 0
        trk.cur.extract_batch(views)
        priors = None
        if mode == "device":
            trk.set_measurements(0, self.meas[t])
            if sync:
                trk.get_imu(0, B)
            trk.motion_predict(B, DT)
        else:
            priors = [self.refs[b].predict(self.Tref[b], DT) for b in range(B)]
            trk.set_prior(0, priors, relative=False)
        prior = trk.get_align(0, B)["T"] if sync or want_prior else None
        trk.track_with_motion_model(B, th=15.0, mono=True, align_mode=0)
        if sync:
            trk.get_tracked(0, B)
        if source == 1:
            trk.track_local_map(B, th=1.0, min_inliers=30)
            if sync:
                trk.get_local_map(0, B)
        if mode == "device":
            trk.motion_update(B, source)
        out = dict(tw=trk.get_tracked(0, B), fm=trk.get_matches(0, B), al=trk.get_align(0, B)["T"], im=trk.get_imu(0, B))
        if want_prior:
            out["prior"] = prior
        if source == 1:
            out.update(gl=trk.get_local_map(0, B), gp=trk.get_pose_opt(0, B))
        status = out["gl"]["status"] if source == 1 else out["tw"]["status"]
        if mode == "host":
            for b in range(B):
                self.refs[b].track(out["al"][b], self.meas[t][b], tracked=status[b] == 2)
        self.Tref = [out["al"][b] for b in range(B)]
        trk.advance(B, source)
        if sync:
            trk.get_last(0, B)
        return out


def flat(x):
    """Every array of a getter's result (dict, tuple, list or array), in a fixed order."""
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [a for v in x for a in flat(v)]
    return [np.asarray(x)]


def test_closed_loop_with_device_imu_prior(sd, oracle, cached_sequences):
    """3 monocular streams x 9 frames, gyro from the ground-truth poses, a constant.  (b) the loop whose priors come from
    tests/imu_ref.py tracks every stream at every frame; (a) the device loop equals it in statuses, match counts and match
    vectors with poses within POSE_TOL; (c) the device loop with a host synchronisation after every call equals (a) byte for
    byte."""
    runs = {}
    for name, mode, sync in (("b", "host", False), ("a", "device", False), ("c", "device", True)):
        L = ILoop(sd, oracle, [11, 12, 13], 9)
        try:
            runs[name] = [L.imu_step(t, mode, sync=sync) for t in range(1, L.T)]
            if name == "b":                                               # the inputs first: every stream tracked at every frame
                for t, o in enumerate(runs["b"], 1):
                    assert (o["tw"]["status"] == 2).all() and (o["gl"]["status"] == 2).all(), t
                assert all(np.abs(f.X[7:13]).max() > 1e-3 for f in L.refs)
        finally:
            L.close()
    for t, (a, b, c) in enumerate(zip(runs["a"], runs["b"], runs["c"]), 1):
        for key in ("tw", "fm", "gl"):
            for x, y in zip(flat(a[key]), flat(b[key])):
                assert np.array_equal(x, y), (t, key)
        assert np.array_equal(a["gp"]["outlier"], b["gp"]["outlier"]), t
        for x, y in ((a["gp"]["T"], b["gp"]["T"]), (a["al"], b["al"])):
            assert np.abs(np.asarray(x) - np.asarray(y)).max() <= SQ.POSE_TOL, t
        assert (a["im"]["started"] == 1).all(), t
        for key in a:
            for x, y in zip(flat(a[key]), flat(c[key])):
                assert x.tobytes() == y.tobytes(), (t, key)


def test_lost_slots_restart(sd, oracle, cached_sequences, tol):
    """source = 0: stream 1 receives an all-zero image at frame 4, so TrackWithMotionModel leaves it untracked: after
    motion_update(0) it is back at IMU::Init (not started, X, gravity, the diagonal blocks of P) while stream 0 updates and
    follows the reference filter; at frame 5 the prior of stream 1 is its Tref bit for bit."""
    L = ILoop(sd, oracle, [11, 12], 6, a=np.array([0.0, 1.0, 0.0]))
    B = L.B
    try:
        f0 = R.EKF()
        for t in range(1, L.T):
            Tref = L.Tref
            o = L.imu_step(t, "device", source=0, blank=(1,) if t == 4 else (), want_prior=True)
            im, st = o["im"], o["tw"]["status"]
            f0.predict(Tref[0], DT)
            f0.track(o["al"][0], L.meas[t][0], tracked=st[0] == 2)
            assert st[0] == 2 and im["started"][0] == 1, t
            d = max(np.abs(im["X"][0] - f0.X).max(), np.abs(im["P"][0] - f0.P).max(), np.abs(im["gravity"][0] - f0.gravity).max())
            assert d <= tol, (t, d)
            if t < 4:
                assert st[1] == 2 and im["started"][1] == 1, t
            if t == 3:
                assert im["gravity"][1][1] > 0.05 and np.abs(im["X"][1][7:10]).max() > 1e-3
            if t == 4:
                assert st[1] != 2 and im["started"][1] == 0
                assert np.array_equal(im["X"][1], X0) and not im["gravity"][1].any() and np.array_equal(im["P"][1][BLOCKS], P0[BLOCKS])
            if t == 5:
                assert o["prior"][1].tobytes() == Tref[1].tobytes()
                assert im["started"][1] == (1 if st[1] == 2 else 0)
    finally:
        L.close()
