"""k_refresh_points (sdslam_amd/csrc/track_refresh.hip) on the MI355X against the numpy restatement tests/refresh_ref.py.

Through sd_debug_refresh_points: the seeded cases of tests/refresh_cases.py (every size in 1, 2, 3, 4, 63, 64, 65, 128, 255, 256;
257; complementary descriptors; identical descriptors; ties across a lane's rows; bad keyframes; bad and empty points; the
reference keyframe's octave 0 and nlevels - 1) and 1, 2, 5 and 700 points in one launch.  With a tracker on two small
extractions: observations in ref frames and the current keyframe with and without the broadcast, a keyframe that is not
resident, a keypoint index outside its frame, the write-through into the local row, the lifetime of the result, and queued
against synchronised calls.

status, best_obs, best_median and desc must be equal; normal, max_dist and min_dist bit-equal (compared as integers).  Outputs
start as a pattern no computation produces, so "untouched" is checked too."""
import numpy as np
import pytest

import refresh_cases as RC
import refresh_ref as RR
import test_triangulation_gpu as TG
import triangulation_cases as TC

pytestmark = pytest.mark.gpu
B, W, H = TG.B, TG.W, TG.H
M = 96
_RIG = {}


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def run_debug(sd, pts, seed=11):
    from sdslam_amd import capi
    c = RC.csr(pts)
    fill = RR.empty_outputs(len(pts), seed=seed)
    got = capi.debug_refresh_points(c["obs_off"], c["obs_desc"], c["obs_centre"], c["obs_octave"], c["ref_obs"], c["Xw"], RC.SF,
                                    obs_kf_bad=c["obs_kf_bad"], point_bad=c["point_bad"], fill=fill)
    want = RR.refresh_points(sf=RC.SF, fill=fill, **c)
    return got, want, fill


@pytest.mark.parametrize("name", list(RC.ALL))
def test_crafted_cases(sd, name):
    pts = RC.ALL[name]()
    got, want, fill = run_debug(sd, pts)
    assert RR.same_outputs(got, want) == [], name
    for i, p in enumerate(pts):
        if "winner" in p:
            assert got["best_obs"][i] == p["winner"]
        if int(got["status"][i]) & 0xFC:                                           # a reason: every output byte as it went in
            assert all(np.array_equal(got[k][i], fill[k][i]) for k in RR.FIELDS if k != "status"), (name, i)


@pytest.mark.parametrize("n_points", [1, 2, 5, 700])
def test_mixed_points_in_one_launch(sd, n_points):
    got, want, _ = run_debug(sd, RC.mixed(n_points))
    assert RR.same_outputs(got, want) == []
    assert n_points < 5 or {RR.SKIPPED, 3} <= set(got["status"].tolist())


def test_without_flag_arrays_and_errors(sd):
    from sdslam_amd import capi
    pts = RC.sized()[:5]
    c = RC.csr(pts)
    got = capi.debug_refresh_points(c["obs_off"], c["obs_desc"], c["obs_centre"], c["obs_octave"], c["ref_obs"], c["Xw"], RC.SF)
    assert RR.same_outputs(got, RR.refresh_points(sf=RC.SF, **c)) == []
    bad_off = c["obs_off"].copy()
    bad_off[2] = bad_off[1] - 1
    with pytest.raises(capi.SdError):
        capi.debug_refresh_points(bad_off, c["obs_desc"], c["obs_centre"], c["obs_octave"], c["ref_obs"], c["Xw"], RC.SF)
    bad_ref = c["ref_obs"].copy()
    bad_ref[0] = 1                                                            # point 0 has one observation
    with pytest.raises(capi.SdError):
        capi.debug_refresh_points(c["obs_off"], c["obs_desc"], c["obs_centre"], c["obs_octave"], bad_ref, c["Xw"], RC.SF)


# ------------------------------------------------------------------------------------------------ with a tracker
def rig(sd):
    if not _RIG:
        cfg = (300, 1.2, RC.NLEVELS, 20)
        cur, ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
        ci, ri = TG.images()
        k1, d1, n1 = cur.extract_batch(ci)
        k2, d2, n2 = ref.extract_batch(ri)
        assert n1.min() >= 100 and n2.min() >= 100
        trk = sd.Tracker(cur, ref, max_points=M, max_batch=B, pnp_max_iterations=8)
        trk.set_camera(*TC.K, 0.0, TG.BOUNDS)
        _RIG.update(trk=trk, cur=cur, ref=ref, imgs=(ci, ri), k=(k1, k2), d=(d1, d2), n=(n1, n2))
    return _RIG


def tracker_points(seed=21, n=40):
    """Observation lists of (frame, kp, kf_bad): ref frames 0..2 and the current keyframe (-1), 1..4 observations a point; one
    point with 130 observations (keypoints 0..129 of frame 1 and more), a bad point, an empty one."""
    rng = np.random.default_rng(seed)
    obs, ref_obs, bad = [], [], np.zeros(n, np.uint8)
    for i in range(n):
        frames = rng.permutation([0, 1, 2, -1])[:rng.integers(1, 5)]
        o = [(int(f), int(rng.integers(0, 100)), int(rng.random() < 0.2)) for f in frames]
        if i == 7:
            o = [(1, k, 0) for k in range(70)] + [(-1, k, k % 5 == 0) for k in range(60)]
        if i == 12:
            o = []
        obs.append(o)
        ref_obs.append(int(rng.integers(0, len(o))) if o else 0)
    bad[20] = 1
    X = rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 4.0]
    return obs, np.array(ref_obs, np.int32), bad, X


def local_row(X, seed=31):
    rng = np.random.default_rng(seed)
    n = len(X)
    return dict(cand=np.ones(n, np.uint8), Xw=X, normal=-rng.uniform(1, 2, (n, 3)), min_dist=-rng.uniform(1, 2, n).astype(np.float32),
                max_dist=-rng.uniform(3, 4, n).astype(np.float32), mf_max_dist=-rng.uniform(5, 6, n).astype(np.float32),
                desc=rng.integers(0, 256, (n, 32)).astype(np.uint8), obs=np.ones(n, np.int32))


def restate_tracker(r, obs, ref_obs, bad, X, bcast, fill, not_resident=(), bad_index=()):
    """The restatement on what the tracker's observations name: the device's own keypoints and descriptors, Ow of the poses."""
    cf = bcast if bcast >= 0 else 0
    flat = [(p, t) for p, o in enumerate(obs) for t in o]
    d, c, oc = np.zeros((len(flat), 32), np.uint8), np.zeros((len(flat), 3)), np.zeros(len(flat), np.int32)
    nr, bi = np.zeros(len(flat), bool), np.zeros(len(flat), bool)
    for j, (p, (f, k, *_)) in enumerate(flat):
        if f == -2:
            nr[j] = True
            continue
        side, fr = (0, cf) if f == -1 else (1, f)
        if k >= r["n"][side][fr] or k < 0:
            bi[j] = True
            continue
        d[j], oc[j] = r["d"][side][fr, k], r["k"][side][fr, k]["octave"]
        c[j] = RR.centre_of(TG.T_CUR[0] if f == -1 else TG.T_REF[f])
    off = np.zeros(len(obs) + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    kb = np.array([t[2] if len(t) > 2 else 0 for _, t in flat], np.uint8)
    return RR.refresh_points(off, d, c, oc, ref_obs, X, RC.SF, obs_kf_bad=kb, point_bad=bad, not_resident=nr, bad_index=bi, fill=fill)


def prepare(r, X, bcast):
    trk = r["trk"]
    trk.set_current_broadcast(-1)
    trk.set_poses(0, TG.T_REF, [TG.T_CUR[0]] * B)
    row = local_row(X)
    trk.set_local(0, [row] * B)
    trk.set_current_broadcast(bcast)
    return row


@pytest.mark.parametrize("bcast", [-1, 0, 2])
def test_tracker_refresh_and_write_through(sd, bcast):
    r = rig(sd)
    trk = r["trk"]
    obs, ref_obs, bad, X = tracker_points()
    obs[30] = obs[30] + [(-2, 0, 0)]                                          # a keyframe that is not resident
    obs[33] = [(0, 5, 0), (2, int(r["n"][1][2]), 0)]                          # a keypoint index one past its frame's count
    ref_obs[33] = 0
    row = prepare(r, X, bcast)
    zero = RR.empty_outputs(len(obs))
    trk.set_observations(obs, ref_obs, bad)
    trk.refresh_points(point_row=1, write_local=False)
    first = trk.get_refreshed()
    want = restate_tracker(r, obs, ref_obs, bad, X, bcast, {k: first[k] for k in RR.FIELDS})
    # entries the kernel does not write hold what the buffers held: compare the written parts, and the statuses exactly
    assert np.array_equal(first["status"], want["status"])
    assert first["status"][30] == RR.NOT_RESIDENT and first["status"][33] == RR.BAD_INDEX and first["status"][12] == first["status"][20] == RR.SKIPPED
    assert first["status"][32] & 3 and first["status"][34] & 3              # the neighbours of the bad index are served
    assert RR.same_outputs(first, want) == []
    assert (first["status"] == 3).sum() >= 25 and first["status"][7] == 3
    assert zero["status"].shape == first["status"].shape
    untouched = trk.read_local_row(1)
    for k in untouched:
        assert np.array_equal(untouched[k][:len(X)], np.asarray(row[k]).astype(untouched[k].dtype).reshape(untouched[k][:len(X)].shape)), k
    # write_local = 1: the row holds the refreshed fields, unwritten points keep the uploaded bytes exactly
    trk.refresh_points(point_row=1, write_local=True)
    got = trk.get_refreshed()
    assert RR.same_outputs(got, first) == []
    after = trk.read_local_row(1)
    for i in range(len(X)):
        st = int(got["status"][i])
        want_desc = got["desc"][i] if st & RR.DESC else row["desc"][i]
        assert np.array_equal(after["desc"][i], want_desc), i
        if st & RR.NORMAL:
            assert np.array_equal(after["normal"][i].view(np.int64), got["normal"][i].view(np.int64))
            assert after["mf_max_dist"][i] == got["max_dist"][i]
            assert after["max_dist"][i] == np.float32(np.float32(1.2) * got["max_dist"][i])
            assert after["min_dist"][i] == np.float32(np.float32(0.8) * got["min_dist"][i])
        else:
            assert np.array_equal(after["normal"][i], row["normal"][i]) and after["mf_max_dist"][i] == row["mf_max_dist"][i]
            assert after["max_dist"][i] == row["max_dist"][i] and after["min_dist"][i] == row["min_dist"][i]
    other = trk.read_local_row(0)                                             # the other rows are not touched
    assert np.array_equal(other["desc"][:len(X)], row["desc"]) and np.array_equal(other["mf_max_dist"][:len(X)], row["mf_max_dist"])
    trk.set_current_broadcast(-1)


def test_result_lifetime(sd):
    from sdslam_amd import capi
    r = rig(sd)
    trk = r["trk"]
    obs, ref_obs, bad, X = tracker_points()

    def fresh(write_local=False):
        prepare(r, X, -1)
        trk.set_observations(obs, ref_obs, bad)
        trk.refresh_points(0, write_local)
        trk.get_refreshed()

    def ended(what):
        with pytest.raises(capi.SdError) as e:
            trk.get_refreshed()
        assert e.value.code == 1, what

    ci, ri = r["imgs"]
    for what, call in (("cur extraction", lambda: r["cur"].extract_batch(ci)), ("ref extraction", lambda: r["ref"].extract_batch(ri)),
                       ("set_poses", lambda: trk.set_poses(0, TG.T_REF, [TG.T_CUR[0]] * B)),
                       ("set_local", lambda: trk.set_local(0, [local_row(X)])),
                       ("set_observations", lambda: trk.set_observations(obs, ref_obs, bad)),
                       ("broadcast", lambda: trk.set_current_broadcast(1))):
        fresh()
        call()
        ended(what)
        trk.set_current_broadcast(-1)
    # a write-through ends a Fuse result (it rewrites the rows the search read); write_local = 0 ends nothing
    trk.set_uright_ref(0, np.full((B, trk.cap), -1, np.float32))
    for write_local in (False, True):
        fresh()
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)
        trk.get_fuse(0, B)
        trk.refresh_points(0, write_local)
        if write_local:
            with pytest.raises(capi.SdError):
                trk.get_fuse(0, B)
        else:
            trk.get_fuse(0, B)
        trk.get_refreshed()
    with pytest.raises(capi.SdError):                                         # frame index outside [-2, max_batch)
        trk.set_observations([[(B, 0, 0)]], [0])
    with pytest.raises(capi.SdError):
        trk.set_observations([[(-3, 0, 0)]], [0])
    with pytest.raises(capi.SdError):                                         # ref_obs outside its list
        trk.set_observations([[(0, 0, 0)]], [1])


def test_fuse_sees_the_refreshed_row(sd):
    """sd_track_fuse after a write-through equals sd_track_fuse after uploading the refreshed fields through sd_track_set_local."""
    r = rig(sd)
    trk = r["trk"]
    n = 60
    rng = np.random.default_rng(5)
    kp = rng.permutation(100)[:n]
    # the surface points ref keyframe 0's own keypoints see, observed there and in the current keyframe
    from sdslam_amd import synth
    R, t = TG.T_REF[0][:3, :3], TG.T_REF[0][:3, 3]
    k = r["k"][1][0, kp]
    rays = np.stack([(k["x"].astype(np.float64) - TC.K[2]) / TC.K[0], (k["y"].astype(np.float64) - TC.K[3]) / TC.K[1], np.ones(n)], -1)
    X = synth.intersect_surface(-R.T @ t, rays @ R, 2.0)
    obs = [[(0, int(k), 0), (-1, int(k2), 0)] for k, k2 in zip(kp, rng.integers(0, 100, n))]
    ref_obs, bad = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    row = prepare(r, X, -1)
    trk.set_uright_ref(0, np.full((B, trk.cap), -1, np.float32))
    trk.set_observations(obs, ref_obs, bad)
    trk.refresh_points(0, True)
    trk.fuse(1, kf_side=1, point_row=0, th=3.0)                               # queued behind the refresh: no upload, no wait
    a = trk.get_fuse(0, 1)
    g = trk.get_refreshed()
    assert (g["status"] == 3).all()
    up = dict(row, desc=g["desc"], normal=g["normal"], mf_max_dist=g["max_dist"], max_dist=np.float32(1.2) * g["max_dist"],
              min_dist=np.float32(0.8) * g["min_dist"])
    trk.set_local(0, [up])
    trk.fuse(1, kf_side=1, point_row=0, th=3.0)
    b = trk.get_fuse(0, 1)
    assert np.array_equal(a["best_idx"], b["best_idx"]) and np.array_equal(a["best_dist"], b["best_dist"])
    assert (a["best_idx"][0, :n] >= 0).sum() >= 20                            # and the search found the points with the new fields
    trk.set_local(0, [row])                                                   # with the uploaded junk fields it finds none
    trk.fuse(1, kf_side=1, point_row=0, th=3.0)
    assert (trk.get_fuse(0, 1)["best_idx"][0, :n] >= 0).sum() == 0


def test_queued_equals_synchronised(sd):
    """set_observations + refresh + fuse queued back to back equal the same calls with a getter (a host wait) after each."""
    r = rig(sd)
    trk = r["trk"]
    obs, ref_obs, bad, X = tracker_points(seed=22)
    obs2, ref2, bad2, _ = tracker_points(seed=23)
    outs = []
    for sync in (False, True):
        prepare(r, X, -1)
        trk.set_observations(obs, ref_obs, bad)
        trk.refresh_points(0, True)
        if sync:
            trk.get_refreshed()
        trk.set_observations(obs2, ref2, bad2)                                # the lists are replaced while the first refresh may still run
        trk.refresh_points(0, True)
        if sync:
            trk.get_refreshed()
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)
        if sync:
            trk.get_fuse(0, B)
        g, f, row = trk.get_refreshed(), trk.get_fuse(0, B), trk.read_local_row(0)
        outs.append(b"".join(np.ascontiguousarray(v).tobytes() for d in (g, f, row) for v in d.values()))
    assert outs[0] == outs[1]
