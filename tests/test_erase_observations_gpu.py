"""sd_track_erase_observations (sdslam_amd/csrc/track_cull.hip) on the MI355X.

Through sd_debug_erase_observations: the hand cases of tests/cull_cases.py and a seeded random list against tests/cull_ref.py,
exactly.  With a tracker on the planted keyframes of tests/test_local_ba_gpu.py: local_ba -> erase(LOCAL_BA) -> refresh_points
gives the bytes of the host round trip it replaces (get_local_ba, the restatement's erase, set_observations, refresh_points);
cull -> erase(CULL) -> local_ba likewise; a cull alone leaves the resident lists as they were; an erase on lists that changed
since the run it names is SD_ERR_INVALID_ARG; sd_track_get_local_ba after the erase still gives the whole obs_erase."""
import numpy as np
import pytest

import ba_cases
import cull_cases as CC
import cull_ref as R
import refresh_ref as RR
import test_local_ba_gpu as LB

pytestmark = pytest.mark.gpu
B = LB.B
ERASE = CC.erase_cases()


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def debug(q, flags):
    from sdslam_amd import capi
    return capi.debug_erase_observations(q["off"], q["stereo"], flags, q["ref_obs"], q["point_bad"])


@pytest.mark.parametrize("name", sorted(ERASE))
def test_debug_entry_equals_the_restatement(sd, name):
    q, flags, hand = ERASE[name]
    got, want = debug(q, flags), R.erase(q, flags)
    print(f"{name}: info8 {got['info8'].tolist()} obs_off {got['obs_off'].tolist()}")
    assert R.differing(got, want, R.ERASE_FIELDS) == []
    for k, v in hand.items():
        assert np.asarray(got[k]).tolist() == np.asarray(v).tolist(), k
    if name == "nothing":                                                   # byte-identical lists
        assert got["obs_off"].tobytes() == q["off"].tobytes() and got["ref_obs"].tobytes() == q["ref_obs"].tobytes()
        assert got["obs_map"].tolist() == list(range(len(q["kf"])))


def test_debug_entry_on_random_lists_twice(sd):
    for seed, P in ((0, 600), (1, 1025), (2, 1)):
        q = CC.random_map(seed, n_points=P)["q"]
        flags = (np.random.default_rng(seed).uniform(size=len(q["kf"])) < 0.25).astype(np.uint8)
        got, want = debug(q, flags), R.erase(q, flags)
        assert R.differing(got, want, R.ERASE_FIELDS) == [] and (P == 1 or want["info8"][2] >= 1)
        again = debug(q, flags)
        assert all(got[k].tobytes() == again[k].tobytes() for k in R.ERASE_FIELDS)


# ------------------------------------------------------------------------------------------------ with a tracker
def erase_problem(p):
    """What tests/cull_ref.py reads of a planted bundle-adjustment problem: camera B is the current keyframe"""
    return dict(off=p["off"], kf=np.where(p["kf"] == B, R.CUR, p["kf"]).astype(np.int32), stereo=(p["ur"] >= 0).astype(np.uint8),
                octave=p["octave"], depth=np.ones(len(p["kf"]), np.float32), ref_obs=np.zeros(len(p["off"]) - 1, np.int32),
                point_bad=p["point_bad"], n_kf=B, kf_bad=p["kf_bad"])


def dense_problem():
    """9 cameras, 150 points: nine of ten are seen by 7 .. 9 cameras, so most keyframes are redundant; the rest by 3, so a cull
    takes some of them to nObs <= 2"""
    p = ba_cases.scene(22, [1, 1, 1, 1, 2, 0, 0, 0, 1], 150, lambda r: int(r.integers(7, 10)) if r.uniform() < 0.9 else 3, stereo_share=0.4,
                       pix_noise=0.5, pose_noise=0.003, point_noise=0.02, wrong_share=0.05)
    octave = np.minimum(np.searchsorted(-ba_cases.INV_SIGMA2, -p["inv_sigma2"]), LB.NLEVELS - 1)
    p["octave"] = octave.astype(np.int32)
    p["inv_sigma2"] = (1.0 / LB.SF[octave] ** 2).astype(np.float32)
    return p


def refreshed(trk):
    return trk.get_refreshed(), trk.get_local_points(0)


def assert_same_refresh(a, b):
    for k in RR.FIELDS:
        assert a[0][k].tobytes() == b[0][k].tobytes(), k
    for k in a[1]:
        assert np.asarray(a[1][k]).tobytes() == np.asarray(b[1][k]).tobytes(), k


def test_local_ba_erase_refresh_equals_the_host_round_trip(sd):
    from sdslam_amd import capi
    p = LB.resident_problem("noisy")
    trk = LB.rig(sd)["trk"]
    q = erase_problem(p)
    # the device chain: nothing comes to the host between the calls
    LB.plant(sd, p)
    trk.local_ba(point_row=0, write_back=True)
    trk.erase_observations(capi.ERASE_LOCAL_BA)
    trk.refresh_points(point_row=0, write_local=True)
    chain, er = refreshed(trk), trk.get_erased()
    ba_after_erase = LB.resident_result(trk.get_local_ba())                 # the run's record outlives the erasure it asked for
    with pytest.raises(capi.SdError) as err:                                # the lists are no longer the ones that run saw
        trk.erase_observations(capi.ERASE_LOCAL_BA)
    assert err.value.code == 1
    # the host round trip it replaces
    pl = LB.plant(sd, p)
    trk.local_ba(point_row=0, write_back=True)
    g = trk.get_local_ba()
    assert g["info16"][0] == 0 and g["info16"][13] > 0
    assert LB.same_bytes(ba_after_erase, LB.resident_result(g)) and ba_after_erase["obs_erase"].sum() == g["info16"][13]
    want = R.erase(q, g["obs_erase"])
    assert R.differing(er, want, R.ERASE_FIELDS) == [] and want["info8"][1] >= g["info16"][13]
    obs, ref_obs, point_bad = R.apply_erase(pl["obs"], pl["ref_obs"], p["point_bad"], want)
    trk.set_observations(obs, ref_obs, point_bad)
    trk.refresh_points(point_row=0, write_local=True)
    assert_same_refresh(chain, refreshed(trk))
    assert (chain[0]["status"] & RR.NORMAL).sum() >= 100


def test_cull_erase_local_ba_equals_the_host_round_trip(sd):
    from sdslam_amd import capi
    p = dense_problem()
    trk = LB.rig(sd)["trk"]
    q = erase_problem(p)
    cand, flags = np.arange(B, dtype=np.int32), np.zeros(B, np.uint8)
    flags[4] = 1                                                            # the fixed keyframe is mnId == 0
    want_cull = R.cull(q, cand, flags, 1, 40.0)
    assert want_cull["info8"][1] >= 2 and want_cull["info8"][4] >= 1 and (want_cull["verdict"] == R.KEPT).any()

    def ba_result():
        g = trk.get_local_ba()
        return LB.resident_result(g)

    LB.plant(sd, p)
    trk.refresh_points(point_row=0, write_local=False)
    before = trk.get_refreshed()
    trk.cull_keyframes(cand, flags, 1, 40.0)
    culled = trk.get_culled()
    assert R.differing(culled, want_cull) == []
    trk.refresh_points(point_row=0, write_local=False)                      # a cull alone leaves the resident lists as they were
    after = trk.get_refreshed()
    for k in RR.FIELDS:
        assert before[k].tobytes() == after[k].tobytes(), k
    trk.cull_keyframes(cand, flags, 1, 40.0)
    trk.erase_observations(capi.ERASE_CULL)
    trk.local_ba(point_row=0, write_back=False)
    chain, er = ba_result(), trk.get_erased()
    with pytest.raises(capi.SdError):                                       # that cull ran on the lists before the erase
        trk.erase_observations(capi.ERASE_CULL)
    # the round trip
    pl = LB.plant(sd, p)
    want = R.erase(q, culled["obs_dead"] != 0)
    assert R.differing(er, want, R.ERASE_FIELDS) == []
    assert want["point_bad"].tolist() == (culled["point_bad"] | p["point_bad"]).tolist()      # the cull's own cascade, found again
    obs, ref_obs, point_bad = R.apply_erase(pl["obs"], pl["ref_obs"], p["point_bad"], want)
    trk.set_observations(obs, ref_obs, point_bad)
    trk.local_ba(point_row=0, write_back=False)
    trip = ba_result()
    n_left = int(want["info8"][3])
    assert trip["info16"][0] == 0 and len(trip["obs_erase"]) == n_left < len(chain["obs_erase"])
    for k in ("T", "Xw", "point_status", "info16"):
        assert chain[k].tobytes() == trip[k].tobytes(), k
    assert chain["obs_erase"][:n_left].tobytes() == trip["obs_erase"].tobytes() and not chain["obs_erase"][n_left:].any()
    # and a second cull on the erased lists sees what a cull on the uploaded ones sees
    trk.cull_keyframes(cand, flags, 1, 40.0)
    on_uploaded = trk.get_culled()
    LB.plant(sd, p)
    trk.cull_keyframes(cand, flags, 1, 40.0)
    trk.erase_observations(capi.ERASE_CULL)
    trk.cull_keyframes(cand, flags, 1, 40.0)
    on_erased = trk.get_culled()
    for k in ("verdict", "counts2", "point_bad", "ref_obs", "n_obs", "info8"):
        assert on_erased[k].tobytes() == on_uploaded[k].tobytes(), k
    assert on_erased["obs_dead"][:n_left].tobytes() == on_uploaded["obs_dead"].tobytes()
