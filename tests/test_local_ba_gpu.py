"""sd_track_local_ba (sdslam_amd/csrc/track_ba.hip) on the MI355X against the numpy restatement tests/ba_ref.py.

Through sd_debug_local_ba: every case of tests/ba_cases.py -- info16, point_status and obs_erase equal, poses and points within
ba_cases.GPU_BOUND (64 times the noise floor tests/test_local_ba_cpu.py measures, never more than 1e-5) -- and two runs with the
same bytes.  With a tracker on planted keyframes: the resident path equals the debug entry byte for byte, write_back = 0 changes
nothing, write_back = 1 leaves exactly the getter's values in Tref / Tcur / Xw and every other byte alone, queued equals
synchronised, a refresh queued behind the run equals tests/refresh_ref.py on the optimised values, refusals write nothing, and a
call without observations is SD_ERR_INVALID_ARG."""
import numpy as np
import pytest

import ba_cases
import ba_ref
import refresh_ref as RR

pytestmark = pytest.mark.gpu
B, W, H, M = 8, 640, 480, 160
SCALE, NLEVELS = 2.0, 3                     # level sigma^2 = 4^level: the inverse is the same float whoever computes it
SF = (SCALE ** np.arange(NLEVELS)).astype(np.float32)
_RIG = {}


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


@pytest.fixture(scope="module")
def cases():
    return ba_cases.cases()


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in ("T", "Xw", "point_status", "obs_erase", "info16"))


@pytest.mark.parametrize("name", ba_cases.RUN_CASES + tuple(ba_cases.REFUSED))
def test_debug_entry_against_the_restatement(sd, cases, name):
    from sdslam_amd import capi
    p = cases[name]
    want, got = ba_ref.run(p), capi.debug_local_ba(p)
    dev = max(np.abs(got["T"] - want["T"]).max(), np.abs(got["Xw"] - want["Xw"]).max())
    print(f"{name}: info16 {got['info16'][:14].tolist()} deviation {dev:.3e} (bound {ba_cases.GPU_BOUND:.1e})")
    assert got["info16"].tolist() == want["info16"].tolist()
    assert np.array_equal(got["point_status"], want["point_status"]) and np.array_equal(got["obs_erase"], want["obs_erase"])
    assert dev <= ba_cases.GPU_BOUND
    if name in ba_cases.REFUSED:
        assert got["info16"][0] == ba_cases.REFUSED[name]
        assert np.array_equal(got["T"], p["poses"]) and np.array_equal(got["Xw"], p["Xw"]) and not got["obs_erase"].any()
    if name == "exact":                                                     # a rejected first trial leaves the inputs, exactly
        assert np.array_equal(got["Xw"], p["Xw"]) and np.array_equal(got["T"], p["poses"])


def test_two_runs_give_the_same_bytes(sd, cases):
    from sdslam_amd import capi
    for name in ("noisy", "special"):
        assert same_bytes(capi.debug_local_ba(cases[name]), capi.debug_local_ba(cases[name])), name


# ------------------------------------------------------------------------------------------------ with a tracker
def rig(sd):
    if not _RIG:
        cfg = (300, SCALE, NLEVELS, 20)
        cur, ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
        img = np.random.default_rng(5).integers(0, 256, (B, H, W)).astype(np.uint8)
        cur.extract_batch(img)                                              # the geometry a planted frame needs
        ref.extract_batch(img)
        trk = sd.Tracker(cur, ref, max_points=M, max_batch=B, pnp_max_iterations=8)
        _RIG.update(trk=trk, cur=cur, ref=ref)
    return _RIG


def resident_problem(name):
    """A case whose cameras 0 .. n_kf - 2 become ref frames and whose last camera the current keyframe, with the information of
    the rig's levels"""
    p = dict(ba_cases.cases()[name])
    octave = np.minimum(np.searchsorted(-ba_cases.INV_SIGMA2, -p["inv_sigma2"]), NLEVELS - 1)
    p["octave"] = octave.astype(np.int32)
    p["inv_sigma2"] = (1.0 / SF[octave] ** 2).astype(np.float32)
    assert len(p["roles"]) == B + 1
    if p["roles"][B] == 0:                                                  # the current keyframe is a local one: swap cameras 0 and B
        swap = np.arange(B + 1)
        swap[[0, B]] = [B, 0]
        p.update(kf=swap[p["kf"]].astype(np.int32), poses=p["poses"][swap], roles=p["roles"][swap])
    return p


def plant(sd, p, seed=3, extra_obs=None):
    """The problem as resident keyframes: every camera's observations become its keypoints 0, 1, ... in edge order.  Returns the
    observation lists, ref_obs, the descriptors per camera and the local row."""
    from sdslam_amd import capi
    r = rig(sd)
    trk, rng = r["trk"], np.random.default_rng(seed)
    n_kf, E, P = len(p["roles"]), len(p["kf"]), len(p["off"]) - 1
    kp_of = np.zeros(E, np.int64)
    kps, descs, ur = [], [], -np.ones((n_kf, trk.cap), np.float32)
    for c in range(n_kf):
        e = np.flatnonzero(p["kf"] == c)
        kp_of[e] = np.arange(len(e))
        k = np.zeros(len(e), capi.KP_DTYPE)
        k["x"], k["y"], k["octave"], k["size"] = p["uv"][e, 0], p["uv"][e, 1], p["octave"][e], 31.0
        kps.append(k)
        descs.append(rng.integers(0, 256, (len(e), 32)).astype(np.uint8))
        ur[c, :len(e)] = p["ur"][e]
    r["ref"].set_keypoints(0, kps[:B], descs[:B])
    r["cur"].set_keypoints(0, [kps[B]] + [kps[B][:1]] * (B - 1), [descs[B]] + [descs[B][:1]] * (B - 1))
    fx, fy, cx, cy = p["cam"]
    trk.set_current_broadcast(-1)
    trk.set_camera(fx, fy, cx, cy, p["bf"], (0.0, float(W), 0.0, float(H)))
    trk.set_uright_ref(0, ur[:B])
    trk.set_uright(0, np.concatenate([ur[B:], -np.ones((B - 1, trk.cap), np.float32)]))
    trk.set_poses(0, list(p["poses"][:B]), [p["poses"][B]] * B)
    row = dict(cand=np.ones(P, np.uint8), Xw=p["Xw"], normal=-rng.uniform(1, 2, (P, 3)), min_dist=-rng.uniform(1, 2, P).astype(np.float32),
               max_dist=-rng.uniform(3, 4, P).astype(np.float32), mf_max_dist=-rng.uniform(5, 6, P).astype(np.float32),
               desc=rng.integers(0, 256, (P, 32)).astype(np.uint8), obs=np.ones(P, np.int32))
    trk.set_local(0, [row] * 2)
    obs = [[(int(p["kf"][e]) if p["kf"][e] < B else -1, int(kp_of[e]), int(p["kf_bad"][e])) for e in range(p["off"][i], p["off"][i + 1])]
           for i in range(P)]
    for i, o in (extra_obs or {}).items():
        obs[i] = obs[i] + [o]
    ref_obs = np.zeros(P, np.int32)
    trk.set_observations(obs, ref_obs, p["point_bad"])
    trk.set_ba_keyframes(p["roles"][:B], int(p["roles"][B]))
    return dict(obs=obs, ref_obs=ref_obs, descs=descs, row=row, kps=kps)


def resident_result(g):
    return dict(T=np.concatenate([g["T_ref"], g["T_cur"][None]]), Xw=g["Xw"], point_status=g["point_status"], obs_erase=g["obs_erase"],
                info16=g["info16"])


@pytest.mark.parametrize("name", ["noisy", "noisy_cur_fixed"])
def test_resident_path_equals_the_debug_entry_and_write_back(sd, name):
    from sdslam_amd import capi
    p = resident_problem(name)
    trk = rig(sd)["trk"]
    pl = plant(sd, p)
    want = capi.debug_local_ba(p)
    assert want["info16"].tolist() == ba_ref.run(p)["info16"].tolist() and want["info16"][13] > 0
    # write_back = 0 changes nothing
    trk.local_ba(point_row=1, write_back=False)
    got = resident_result(trk.get_local_ba())
    assert same_bytes(got, want)
    Tr, Tc = trk.read_poses(B)
    assert np.array_equal(Tr, p["poses"][:B]) and np.array_equal(Tc, np.stack([p["poses"][B]] * B))
    assert np.array_equal(trk.get_local_points(1)["Xw"][:len(p["Xw"])], p["Xw"])
    # write_back = 1: exactly the getter's values, every other byte alone
    before = [trk.get_local_points(rw) for rw in (0, 1)]
    trk.local_ba(point_row=1, write_back=True)
    got2 = resident_result(trk.get_local_ba())
    assert same_bytes(got2, want)
    Tr, Tc = trk.read_poses(B)
    assert np.array_equal(Tr, want["T"][:B]) and np.array_equal(Tc[0], want["T"][B]) and np.array_equal(Tc[1:], np.stack([p["poses"][B]] * (B - 1)))
    fixed = np.flatnonzero(p["roles"] != 1)
    assert np.array_equal(want["T"][fixed], p["poses"][fixed]) and not np.array_equal(want["T"], p["poses"])
    after = [trk.get_local_points(rw) for rw in (0, 1)]
    n = len(p["Xw"])
    assert np.array_equal(after[1]["Xw"][:n], want["Xw"]) and np.array_equal(after[1]["Xw"][n:], before[1]["Xw"][n:])
    for k in before[0]:
        assert np.array_equal(after[0][k], before[0][k]), k
        assert k == "Xw" or np.array_equal(after[1][k], before[1][k]), k


def test_queued_equals_synchronised_and_the_refresh_behind_it(sd):
    p = resident_problem("noisy")
    p["uv"] = p["uv"].copy()
    trk = rig(sd)["trk"]
    # no erasures: take the planted wrong observations out by running the restatement once and marking them bad keyframes
    p["kf_bad"] = ba_ref.run(p)["obs_erase"].copy()
    assert p["kf_bad"].sum() > 20 and ba_ref.run(p)["info16"][13] == 0
    results = []
    for synchronised in (False, True):
        pl = plant(sd, p)
        if synchronised:
            trk.read_poses(1)
        trk.local_ba(point_row=0, write_back=True)
        if synchronised:
            trk.get_local_ba()
        trk.refresh_points(point_row=0, write_local=True)
        if synchronised:
            trk.get_refreshed()
        results.append((resident_result(trk.get_local_ba()), trk.get_refreshed(), trk.get_local_points(0)))
    (ba_q, rf_q, row_q), (ba_s, rf_s, row_s) = results
    assert same_bytes(ba_q, ba_s) and ba_q["info16"][13] == 0 and ba_q["info16"][0] == 0
    for k in RR.FIELDS:
        assert np.array_equal(rf_q[k], rf_s[k]), k
    for k in row_q:
        assert np.array_equal(row_q[k], row_s[k]), k
    # the refresh is UpdateNormalAndDepth (and the descriptor) of tests/refresh_ref.py on the optimised poses and positions
    flat = [(i, t) for i, o in enumerate(pl["obs"]) for t in o]
    d, c = np.zeros((len(flat), 32), np.uint8), np.zeros((len(flat), 3))
    oc = np.zeros(len(flat), np.int32)
    for j, (i, (f, k, _)) in enumerate(flat):
        cam = B if f == -1 else f
        d[j], oc[j], c[j] = pl["descs"][cam][k], pl["kps"][cam][k]["octave"], RR.centre_of(ba_q["T"][cam])
    want = RR.refresh_points(p["off"], d, c, oc, pl["ref_obs"], ba_q["Xw"], SF, obs_kf_bad=p["kf_bad"], point_bad=p["point_bad"],
                             fill={k: rf_q[k] for k in RR.FIELDS})
    assert RR.same_outputs(rf_q, want) == []
    assert (rf_q["status"] & RR.NORMAL).sum() >= 140


def test_refusals_write_nothing(sd):
    p = resident_problem("noisy")
    trk = rig(sd)["trk"]
    for extra, status in (({40: (-2, 0, 0)}, ba_ref.SD_BA_NOT_RESIDENT), ({41: (2, 250, 0)}, ba_ref.SD_BA_BAD_INDEX)):
        plant(sd, p, extra_obs=extra)
        before = trk.get_local_points(0)
        trk.local_ba(point_row=0, write_back=True)
        g = trk.get_local_ba()
        assert g["info16"].tolist() == [status] + [0] * 15 and not g["obs_erase"].any()
        assert np.array_equal(g["T_ref"], p["poses"][:B]) and np.array_equal(g["T_cur"], p["poses"][B]) and np.array_equal(g["Xw"], p["Xw"])
        Tr, Tc = trk.read_poses(B)
        assert np.array_equal(Tr, p["poses"][:B]) and np.array_equal(Tc[0], p["poses"][B])
        after = trk.get_local_points(0)
        assert all(np.array_equal(after[k], before[k]) for k in before)
        if status == ba_ref.SD_BA_BAD_INDEX:
            assert g["point_status"][41] == ba_ref.POINT_BAD_INDEX and (np.delete(g["point_status"], 41) == ba_ref.POINT_SKIPPED).all()


def test_too_many_free_keyframes_on_the_resident_path(sd):
    """33 ref frames and the current keyframe, all with role 1: the host queues the short schedule, the device counts and refuses"""
    from sdslam_amd import capi
    nb = ba_ref.MAX_FREE_KF + 1
    cfg = (100, SCALE, NLEVELS, 20)
    cur, ref = sd.ORBextractor(*cfg, 320, 240, nb), sd.ORBextractor(*cfg, 320, 240, nb)
    img = np.random.default_rng(6).integers(0, 256, (nb, 240, 320)).astype(np.uint8)
    cur.extract_batch(img)
    ref.extract_batch(img)
    k = np.zeros(1, capi.KP_DTYPE)
    k["x"], k["y"] = 100.0, 90.0
    ref.set_keypoints(0, [k] * nb, [np.zeros((1, 32), np.uint8)] * nb)
    cur.set_keypoints(0, [k] * nb, [np.zeros((1, 32), np.uint8)] * nb)
    trk = sd.Tracker(cur, ref, max_points=16, max_batch=nb, pnp_max_iterations=8)
    trk.set_camera(*ba_cases.CAM, ba_cases.BF, (0.0, 320.0, 0.0, 240.0))
    T = np.stack([np.eye(4)] * nb)
    T[:, 0, 3] = -0.1 * np.arange(nb)
    trk.set_poses(0, list(T), list(T))
    X = np.array([[0.1, 0.0, 4.0], [0.0, 0.1, 5.0]])
    row = dict(cand=np.ones(2, np.uint8), Xw=X, normal=np.zeros((2, 3)), min_dist=np.zeros(2, np.float32), max_dist=np.zeros(2, np.float32),
               mf_max_dist=np.zeros(2, np.float32), desc=np.zeros((2, 32), np.uint8), obs=np.ones(2, np.int32))
    trk.set_local(0, [row])
    trk.set_observations([[(0, 0, 0), (1, 0, 0), (-1, 0, 0)], [(2, 0, 0), (3, 0, 0)]], np.zeros(2, np.int32))
    for n_role1, status in ((nb, ba_ref.SD_BA_TOO_MANY_KF), (nb - 2, ba_ref.SD_BA_OK)):
        roles = np.ones(nb, np.uint8)
        roles[n_role1:] = 0
        trk.set_ba_keyframes(roles, 1)                                      # n_role1 ref frames and the current keyframe are free
        trk.local_ba(point_row=0, write_back=True)
        g = trk.get_local_ba()
        assert g["info16"][0] == status and g["info16"][1] == (0 if status else ba_ref.MAX_FREE_KF)
        if status:
            assert g["info16"].tolist() == [status] + [0] * 15 and np.array_equal(g["T_ref"], T) and np.array_equal(g["Xw"], X)
            Tr, Tc = trk.read_poses(nb)
            assert np.array_equal(Tr, T) and np.array_equal(Tc, T) and np.array_equal(trk.get_local_points(0)["Xw"][:2], X)


def test_a_call_without_observations_is_an_invalid_argument(sd):
    from sdslam_amd import capi
    r = rig(sd)
    fresh = sd.Tracker(r["cur"], r["ref"], max_points=16, max_batch=B, pnp_max_iterations=8)
    fresh.set_camera(*ba_cases.CAM, ba_cases.BF, (0.0, float(W), 0.0, float(H)))
    fresh.set_ba_keyframes(np.ones(B, np.uint8), 1)
    with pytest.raises(capi.SdError) as e:
        fresh.local_ba()
    assert e.value.code == 1 and "sd_track_set_observations" in str(e.value)            # SD_ERR_INVALID_ARG
