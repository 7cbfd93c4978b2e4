"""GPU: the motion model on the device (sd_track_motion_predict / _update / _restart, sd_track_get_motion / _set_motion).

The per-slot EKF + ConstantVelocity state equals tests/motion_ref.py (the reference's dense 6x6 filter in numpy) fed the same
poses; the prior it produces drives the closed loop of tests/test_sequence_gpu.py to the oracle's results; a slot that loses
track restarts; queued and synchronised loops are identical; the documented errors leave the state alone.

Bound of the float comparisons, derived (not tuned): values are O(1) or smaller, the chain from the poses to X / P / E / the
prior is under ~200 double operations with the device's sin / cos / atan / tan within a few ulp of the host's, and the
cancelling terms (t - sin t) / t^3, (1 - cos t) / t^2, (1 - t / (2 tan(t / 2))) / t^2 are multiplied by Omega or Omega^2, so the
worst case is a few 1e-13: TOL = 1e-12 absolute.  Flags and it_time are compared exactly."""
import ctypes

import numpy as np
import pytest

import motion_cases as MC
import motion_ref as R
import test_sequence_gpu as SQ
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-12
DT = 1.0 / 30.0
B70 = 70
P0 = np.array([R.COV_V_2] * 3 + [R.COV_W_2] * 3)
TINY = (50, 1.2, 1, 20, 64, 64)          # a small extractor geometry the plan accepts: the filter calls read no image


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


@pytest.fixture()
def trk70(sd):
    ext = [sd.ORBextractor(*TINY, B70) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=8, max_batch=B70, pnp_max_iterations=4)
    yield trk
    trk.close()
    for e in ext:
        e.close()


def start_poses(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [R.exp(np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.6, 0.6, 3)])) for _ in range(B70)]


def check_state(mo, refs, n, key):
    """Device state of slots < n against the reference filters, slots >= n against a filter nobody touched."""
    worst = 0.0
    for i in range(B70):
        f = refs[i] if i < n else R.EKF()
        assert mo["started"][i] == int(f.started()), (key, i)
        assert mo["it_time"][i] == f.it_time, (key, i)
        assert (f.P[~np.eye(6, dtype=bool)] == 0).all()
        d = max(np.abs(mo["X"][i] - f.X).max(), np.abs(mo["P"][i] - np.diag(f.P)).max())
        if i < n:
            d = max(d, np.abs(mo["E"][i] - f.E).max())
        assert d <= TOL, (key, i, MC.NAMES[i % len(MC.NAMES)], d)
        worst = max(worst, d)
    return worst


@pytest.mark.parametrize("n", [B70, 5])
def test_unstarted_prior_is_the_last_pose(trk70, n):
    """A new handle and a restarted one: Tprior = Tref bit for bit, started = 0; slots >= n keep state and prior;
    motion_restart touches its range only."""
    trk = trk70
    Tref, eye = start_poses(1), [np.eye(4)] * B70
    trk.set_poses(0, Tref, eye)
    trk.motion_predict(n, DT)
    got, mo = trk.get_align(0, B70)["T"], trk.get_motion(0, B70)
    for i in range(B70):
        assert got[i].tobytes() == (Tref[i] if i < n else np.eye(4)).tobytes(), i
        assert np.array_equal(mo["last_pose"][i], Tref[i] if i < n else np.zeros((4, 4))), i
    assert not mo["started"].any() and not mo["it_time"].any() and not mo["X"].any() and np.array_equal(mo["P"], np.tile(P0, (B70, 1)))
    assert all(np.array_equal(mo["E"][i], np.eye(4)) for i in range(n))
    # start the filters and give them a velocity
    T = Tref
    for _ in range(3):
        T2 = [R.exp(MC.slot_twist(i)) @ T[i] for i in range(B70)]
        trk.set_poses(0, T, T2)
        trk.motion_predict(n, DT)
        trk.set_poses(0, T, T2)                                          # the frame's final pose in Tcur
        trk.motion_update(n, -1)
        T = T2
    mo = trk.get_motion(0, B70)
    assert mo["started"][:n].all() and not mo["started"][n:].any()
    assert all(mo["X"][i].any() for i in range(n) if i % len(MC.NAMES) != 0) and not mo["X"][n:].any()
    assert np.array_equal(mo["P"][n:], np.tile(P0, (B70 - n, 1)))
    trk.motion_restart(2, 3)                                             # slots 2..4 only
    after = trk.get_motion(0, B70)
    for i in range(B70):
        if 2 <= i < 5:
            assert after["started"][i] == 0 and not after["X"][i].any() and np.array_equal(after["P"][i], P0), i
        else:
            assert after["started"][i] == mo["started"][i] and np.array_equal(after["X"][i], mo["X"][i]), i
            assert np.array_equal(after["P"][i], mo["P"][i]), i
    trk.motion_restart(0, n)
    trk.set_poses(0, T, eye)
    trk.motion_predict(n, DT)
    got, mo = trk.get_align(0, B70)["T"], trk.get_motion(0, B70)
    for i in range(B70):
        assert got[i].tobytes() == (T[i] if i < n else np.eye(4)).tobytes(), i
    assert not mo["started"].any() and not mo["it_time"].any()


@pytest.mark.parametrize("n", [B70, 5])
def test_filter_matches_reference(trk70, n):
    """70 slots x 8 steps, every slot stepping by its own fixed twist (tests/motion_cases.py: every branch of Exp / Log and
    of the quaternion conversion), dt = 1/30 and 0.1 alternating and one dt = 0: after every step X, the diagonal of P, E,
    started, it_time and the prior equal the dense reference filter fed the same poses; the prior is the product of
    sd_track_set_prior on the getter's E, bit for bit."""
    trk = trk70
    refs = [R.EKF() for _ in range(B70)]
    T = start_poses(2)
    kept = [np.eye(4) * (i + 2) for i in range(B70)]                    # what set_poses leaves in Tprior: slots >= n keep it
    worst = 0.0
    for step, dt in enumerate(MC.DTS):
        T2 = [R.exp(MC.slot_twist(i)) @ T[i] for i in range(B70)]
        trk.set_poses(0, T, kept)
        trk.motion_predict(n, dt)
        prior, mo = trk.get_align(0, B70)["T"], trk.get_motion(0, B70)
        for i in range(B70):
            if i >= n:
                assert np.array_equal(prior[i], kept[i]), (step, i)
                continue
            want = refs[i].predict(T[i], dt)
            d = np.abs(prior[i] - want).max()
            assert d <= TOL, (step, i, MC.NAMES[i % len(MC.NAMES)], d)
            worst = max(worst, d)
            assert prior[i].tobytes() == SQ.prior_product(mo["E"][i], T[i]).tobytes(), (step, i)
            assert np.array_equal(mo["last_pose"][i], T[i]), (step, i)
        worst = max(worst, check_state(mo, refs, n, ("predict", step)))
        trk.set_poses(0, T, T2)                                          # the "tracked" pose of this frame
        trk.motion_update(n, -1)
        for i in range(n):
            refs[i].track(T2[i])
        worst = max(worst, check_state(trk.get_motion(0, B70), refs, n, ("update", step)))
        T = T2
    print(f"motion filter, n = {n}: largest deviation from the reference {worst:.3e}")
    if n == B70:                                                         # the filters arrived somewhere: not a comparison of zeros
        assert all(np.abs(refs[i].X).max() > 1e-3 for i in range(B70) if i % len(MC.NAMES) != 0)


def test_set_motion_restores_a_filter(trk70):
    trk = trk70
    rng = np.random.Generator(np.random.PCG64(3))
    X, P = rng.normal(size=(4, 6)) * 0.01, rng.uniform(1e-4, 1e-3, (4, 6))
    trk.set_motion(3, X=X, P=P, started=[1, 0, 1, 1], it_time=[0.1, 0.0, 0.2, 0.3])
    mo = trk.get_motion(0, B70)
    assert np.array_equal(mo["X"][3:7], X) and np.array_equal(mo["P"][3:7], P)
    assert list(mo["started"][2:8]) == [0, 1, 0, 1, 1, 0] and list(mo["it_time"][3:7]) == [0.1, 0.0, 0.2, 0.3]
    T = start_poses(4)
    trk.set_poses(0, T, T)
    trk.motion_predict(B70, 0.05)
    prior = trk.get_align(0, B70)["T"]
    mo = trk.get_motion(3, 2)
    for j, started in ((0, True), (1, False)):                           # the restored X drives the next prior
        f = R.EKF()
        f.X, f.updated = X[j].copy(), started
        f.P = np.diag(P[j])
        assert np.abs(prior[3 + j] - f.predict(T[3 + j], 0.05)).max() <= TOL
        assert mo["it_time"][j] == f.it_time == (0.05 if started else 0.0) and np.abs(mo["P"][j] - np.diag(f.P)).max() <= TOL


class MLoop(SQ.Loop):
    """The loop of tests/test_sequence_gpu.py with the device's own prior: motion_predict / motion_update for set_prior."""

    def motion_step(self, t, th_mm, th_lm, sync, blank=()):
        trk, B = self.trk, self.B
        views = self.views[t]
        if blank:
            views = views.copy()
            views[list(blank)] = 0
        trk.cur.extract_batch(views)
        if self.rgbd:
            trk.stereo_from_depth(np.stack([s["depth"][t] for s in self.seqs]))
        trk.motion_predict(B, DT)
        out = (trk.get_align(0, B)["T"], trk.get_motion(0, B)) if sync else None
        trk.track_with_motion_model(B, th=th_mm, mono=not self.rgbd, align_mode=0)
        if sync:
            trk.get_tracked(0, B)
        trk.track_local_map(B, th=th_lm, min_inliers=30)
        if sync:
            trk.get_local_map(0, B)
        trk.motion_update(B, 1)
        return out

    def oracle_step_prior(self, oracle, t, b, T_pred, th_mm, th_lm, u_right=None):
        """Loop.oracle_step with the prior given (the device's) instead of composed from the ground-truth velocity."""
        O = self.o_ext[b]
        ck, cd = O[1].extract(self.views[t][b])
        NL, tab, last = self.cfg[2], self.tab, self.o_last[b]
        Kc, M = SQ.K, SQ.M
        mb = np.float32(self.bf) / np.float32(Kc[0])
        pc = [O[1].level(l) for l in range(NL)]
        pr = [O[0].level(l) for l in range(NL)]
        mono = not self.rgbd
        kw = dict(u_right=u_right, mbf=self.bf, mb=mb) if not mono else {}
        r = oracle.track_with_motion_model(pc, pr, tab, ck, cd, self.bounds, Kc, self.o_T[b], T_pred, last, th_mm, mono=mono, align_mode=0, **kw)
        seen = r["match"]
        if r["status"] != 0:
            retried = bool(r["retried"])
            T_s = T_pred if retried or not r["align"]["ok"] else r["align"]["T"]
            _, seen = oracle.search_by_projection(ck, cd, tab["sf"], self.bounds, Kc, T_s, self.o_T[b], last, th=2 * th_mm if retried else th_mm,
                                                  mono=mono, check_ori=True, **kw)
            assert np.array_equal(np.where(r["match"] >= 0, seen, -1), r["match"])
        seen_ids = set(self.o_ids[b][seen[seen >= 0]].tolist()) - {-1}
        local = dict(self.local[b])
        local["cand"] = np.array([0 if i in seen_ids else 1 for i in self.lids[b]], np.uint8)
        rl = oracle.track_local_map(ck, cd, tab, np.log(np.float32(self.cfg[1])), self.bounds, Kc, r["T"], r["match"], last, local, th=th_lm,
                                    min_inliers=30, u_right=u_right, mbf=self.bf)
        un = np.where(rl["local_match"] >= 0, rl["local_match"] + M, rl["frame_match"])
        N = len(ck)
        h = SQ.host_handoff(ck, N, un, rl["outlier"], last, self.o_ids[b], self.local[b], self.lids[b])
        self.o_last[b], self.o_ids[b] = SQ.as_last(h, N)
        self.o_T[b] = rl["T"]
        O.reverse()
        return r, rl, un, N


@pytest.mark.parametrize("kind,seeds,T,th_lm", [("mono", [11, 12, 13], 10, 1.0), ("rgbd", [21, 22], 6, 3.0)])
def test_closed_loop_with_device_prior(sd, oracle, kind, seeds, T, th_lm):
    """predict(1/30) -> TrackWithMotionModel -> TrackLocalMap -> update(1) -> advance(1) per frame.  (a) prior, X and P equal
    the reference filter fed the device's own final poses; (b) the oracle's loop driven with the device's priors gives equal
    statuses, counts and match vectors and poses within POSE_TOL; (c) every stream is tracked at every frame, frame 1 (prior =
    the last pose, no velocity) included."""
    L = MLoop(sd, oracle, SQ.CFGS["p8"], seeds, T, rgbd=kind == "rgbd")
    trk, B = L.trk, L.B
    try:
        refs = [R.EKF() for _ in range(B)]
        Tref = [s["T"][0] for s in L.seqs]
        worst = 0.0
        for t in range(1, L.T):
            prior, mo_p = L.motion_step(t, 15.0, th_lm, sync=True)
            tw, (fm, _), gl, gp, al = trk.get_tracked(0, B), trk.get_matches(0, B), trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_align(0, B)
            ur = trk.get_stereo(0, B)[0] if L.rgbd else None
            _, _, cn = trk.cur.download(0, B)
            mo = trk.get_motion(0, B)
            trk.advance(B, 1)
            for b in range(B):
                key = (kind, t, b)
                # (a) the filter on the device's own poses
                want = refs[b].predict(Tref[b], DT)
                d = max(np.abs(prior[b] - want).max(), np.abs(mo_p["E"][b] - refs[b].E).max())
                assert prior[b].tobytes() == SQ.prior_product(mo_p["E"][b], Tref[b]).tobytes(), key
                assert mo_p["it_time"][b] == refs[b].it_time == (DT if t > 1 else 0.0), key
                if t == 1:
                    assert prior[b].tobytes() == Tref[b].tobytes(), key
                refs[b].track(al["T"][b], tracked=gl["status"][b] == 2)
                d = max(d, np.abs(mo["X"][b] - refs[b].X).max(), np.abs(mo["P"][b] - np.diag(refs[b].P)).max())
                assert d <= TOL and mo["started"][b] == int(refs[b].started()), (key, d)
                worst = max(worst, d)
                # (b) the oracle's loop on the device's prior
                n = cn[b]
                r, rl, un, N = L.oracle_step_prior(oracle, t, b, prior[b], 15.0, th_lm, u_right=ur[b, :n] if L.rgbd else None)
                assert N == n, key
                assert (tw["status"][b], tw["nmatches"][b], tw["nmatches_map"][b]) == (r["status"], r["nmatches"], r["nmatches_map"]), key
                assert np.array_equal(fm[b, :n], r["match"]) and np.array_equal(gl["match"][b, :n], un), key
                assert (gl["status"][b], gl["n_inliers"][b]) == (rl["status"], rl["n_inliers"]), key
                assert np.array_equal(gp["outlier"][b, :n], rl["outlier"]), key
                assert np.abs(gp["T"][b] - rl["T"]).max() <= SQ.POSE_TOL, (key, np.abs(gp["T"][b] - rl["T"]).max())
                assert np.abs(al["T"][b] - gp["T"][b]).max() == 0, key
                # (c) tracked, near the truth
                assert tw["status"][b] == 2 and gl["status"][b] == 2, key
                assert np.abs(gp["T"][b][:3, 3] - L.seqs[b]["T"][t][:3, 3]).max() < 0.02, key
                Tref[b] = al["T"][b]
        print(f"closed loop {kind}: largest deviation of prior / E / X / P from the reference {worst:.3e}")
        assert all(np.abs(f.X).max() > 1e-3 for f in refs)
    finally:
        L.close()


def test_restart_on_failure(sd, oracle):
    """Stream 1 receives an all-zero image at frame 4: after motion_update(1) it is not started, X = 0, P at its initial
    diagonal, stream 0 goes on; at frame 5 its prior is its Tref bit for bit.  A slot whose Tref is all zeros restarts
    instead of updating."""
    L = MLoop(sd, oracle, SQ.CFGS["p8"], [11, 12], 6)
    trk, B = L.trk, L.B
    try:
        f0 = R.EKF()
        Tref = [s["T"][0] for s in L.seqs]
        for t in range(1, L.T):
            prior, _ = L.motion_step(t, 15.0, 1.0, sync=True, blank=(1,) if t == 4 else ())
            gl, al, mo = trk.get_local_map(0, B), trk.get_align(0, B), trk.get_motion(0, B)
            trk.advance(B, 1)
            f0.predict(Tref[0], DT)
            f0.track(al["T"][0], tracked=gl["status"][0] == 2)
            assert gl["status"][0] == 2 and mo["started"][0] == 1, t
            assert max(np.abs(mo["X"][0] - f0.X).max(), np.abs(mo["P"][0] - np.diag(f0.P)).max()) <= TOL, t
            if t < 4:
                assert gl["status"][1] == 2 and mo["started"][1] == 1, t
            if t == 3:
                assert np.abs(mo["X"][1]).max() > 1e-3 and not np.array_equal(mo["P"][1], P0)
            if t == 4:
                assert gl["status"][1] != 2
                assert mo["started"][1] == 0 and not mo["X"][1].any() and np.array_equal(mo["P"][1], P0)
            if t == 5:
                assert prior[1].tobytes() == Tref[1].tobytes()
            Tref = [al["T"][b] for b in range(B)]
        assert trk.get_motion(0, 1)["started"][0] == 1
        good = L.seqs[0]["T"][0]
        trk.set_poses(0, [np.zeros((4, 4)), good], [good, good])
        trk.motion_predict(B, DT)
        trk.set_poses(0, [np.zeros((4, 4)), good], [good, good])
        trk.motion_update(B, -1)
        mo = trk.get_motion(0, B)
        assert list(mo["started"]) == [0, 1] and not mo["X"][0].any() and np.array_equal(mo["P"][0], P0)
    finally:
        L.close()


def test_queued_loop_equals_synchronised_loop(sd, oracle):
    """The loop with no getter between the calls gives the per-frame records, the final filter state and the final last
    frame of the loop that synchronises after every call."""
    out = []
    for sync in (True, False):
        L = MLoop(sd, oracle, SQ.CFGS["p8"], [11, 12, 13], 10)
        trk, B = L.trk, L.B
        try:
            rec = sd.DeviceBuffer(L.T * B * 160)
            for t in range(1, L.T):
                L.motion_step(t, 15.0, 1.0, sync=sync)
                trk.pack_records(B, 3, ctypes.c_void_p(rec.ptr.value + t * B * 160).value)
                if sync:
                    trk.get_motion(0, B)
                trk.advance(B, 1)
                if sync:
                    trk.get_last(0, B)
            mo, last = trk.get_motion(0, B), trk.get_last(0, B)
            out.append((SQ._download(rec.ptr, L.T * B * 160)[B * 160:], mo, last))
            rec.free()
        finally:
            L.close()
    assert np.array_equal(out[0][0], out[1][0])
    for k in ("X", "P", "started", "it_time", "E", "last_pose"):
        assert np.array_equal(np.asarray(out[0][1][k]), np.asarray(out[1][1][k])), k
    for k in out[0][2]:
        assert np.array_equal(out[0][2][k], out[1][2][k]), k
    recs = out[0][0].view(np.float64).reshape(-1, 20)
    assert (recs[:, 19] == 1).all()


def test_motion_errors(sd):
    """Each documented error returns its code and leaves filter state and prior untouched."""
    ext = [sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 2) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=SQ.M, max_batch=2)
    try:
        seq = synth.make_sequence(3, 3)
        trk.set_camera(*SQ.K, 0.0, SQ.BOUNDS)
        for t in (0, 1):                                                  # a started filter with a velocity
            trk.set_poses(0, [seq["T"][t]] * 2, [seq["T"][t + 1]] * 2)
            trk.motion_predict(2, DT)
            trk.set_poses(0, [seq["T"][t]] * 2, [seq["T"][t + 1]] * 2)
            trk.motion_update(2, -1)
        trk.ref.extract_batch(np.stack([seq["views"][0]] * 2))
        trk.cur.extract_batch(np.stack([seq["views"][1]] * 2))
        trk.set_poses(0, [seq["T"][0]] * 2, [seq["T"][1]] * 2)
        before, prior = trk.get_motion(0, 2), trk.get_align(0, 2)["T"]
        assert before["started"].all() and before["X"].any()

        def refused(code, call, *args):
            with pytest.raises(sd.SdError) as e:
                call(*args)
            assert e.value.code == code, (call.__name__, args)
            after = trk.get_motion(0, 2)
            for k in before:
                assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), (call.__name__, args, k)
            assert np.array_equal(np.asarray(prior), np.asarray(trk.get_align(0, 2)["T"])), (call.__name__, args)

        for src in (0, 1):                                                # neither call has run on this extraction
            refused(1, trk.motion_update, 2, src)
        trk.track_with_motion_model(2, th=15.0)
        prior = trk.get_align(0, 2)["T"]
        refused(1, trk.motion_update, 2, 1)                               # TrackLocalMap has not
        refused(1, trk.motion_update, 2, 5)
        refused(1, trk.motion_update, 2, -2)
        refused(1, trk.motion_predict, 2, -1.0)
        refused(1, trk.motion_predict, 2, float("nan"))
        refused(1, trk.motion_predict, 2, float("inf"))
        refused(3, trk.motion_predict, 3, DT)
        refused(3, trk.motion_update, 3, -1)
        refused(3, trk.motion_restart, 1, 2)
        trk.set_current_broadcast(0)
        refused(1, trk.motion_predict, 2, DT)
        refused(1, trk.motion_update, 2, -1)
        refused(1, trk.motion_update, 2, 0)
        trk.set_current_broadcast(-1)
        trk.motion_update(2, 0)                                           # the accepted call goes through: no last-frame points,
        assert not trk.get_motion(0, 2)["started"].any()                  # so TrackWithMotionModel failed and the filters restart
    finally:
        trk.close()
        for e_ in ext:
            e_.close()
