"""sd_track_cull_keyframes (sdslam_amd/csrc/track_cull.hip) on the MI355X against the restatement tests/cull_ref.py.

Through sd_debug_cull_keyframes: every hand case of tests/cull_cases.py and seeded random maps of 24 keyframes and 600 points,
every output exactly equal (they are all integers).  Through the handle: the cases that fit the rig and random maps of 8 + 1
keyframes, built on planted keypoints (sd_debug_orb_set_keypoints), mvuRight rows and the mvDepth rows of sd_track_set_tri_depth.
Each is run twice and the bytes compared."""
import numpy as np
import pytest

import cull_cases as CC
import cull_ref as R

pytestmark = pytest.mark.gpu
B, W, H, M = 8, 640, 480, 160
_RIG = {}
CASES = CC.cases()
RANDOM = {f"random_{s}": CC.random_map(s) for s in range(3)}
# what the rig holds: keyframes 0 .. 7 and the current one, M points, candidates among the ref frames
SMALL = {f"small_random_{s}": CC.random_map(10 + s, n_kf=B, n_points=150, lo=2, hi=7, n_cand=B) for s in range(2)}
ON_HANDLE = sorted(n for n, c in CASES.items() if c["q"]["n_kf"] <= B and len(c["q"]["off"]) - 1 <= M
                   and c["q"]["kf"].min() >= -2 and c["q"]["kf"].max() < B) + sorted(SMALL)   # (a frame outside [-2, B) cannot be uploaded)


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in R.FIELDS)


def debug(c):
    from sdslam_amd import capi
    return capi.debug_cull_keyframes(c["q"], c["cand"], c["flags"], c["mono"], c["th"])


def want_of(c):
    return R.cull(c["q"], c["cand"], c["flags"], c["mono"], c["th"])


@pytest.mark.parametrize("name", sorted(CASES) + sorted(RANDOM))
def test_debug_entry_equals_the_restatement(sd, name):
    c = CASES.get(name) or RANDOM[name]
    got, want = debug(c), want_of(c)
    print(f"{name}: info8 {got['info8'].tolist()} verdicts {np.bincount(got['verdict'], minlength=4).tolist()}")
    assert R.differing(got, want) == []
    for k, v in c["want"].items():                                          # and the hand answer itself
        assert np.asarray(got[k]).tolist() == np.asarray(v).tolist(), k
    assert same_bytes(debug(c), got)


def rig(sd):
    if not _RIG:
        cfg = (300, 2.0, 3, 20)
        cur, ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
        img = np.random.default_rng(5).integers(0, 256, (B, H, W)).astype(np.uint8)
        cur.extract_batch(img)                                              # the geometry a planted frame needs
        ref.extract_batch(img)
        _RIG.update(trk=sd.Tracker(cur, ref, max_points=M, max_batch=B, pnp_max_iterations=8), cur=cur, ref=ref)
    return _RIG


def plant(sd, c, seed=3, kp_shift=None):
    """The problem as resident keyframes: every keyframe's entries become its keypoints 0, 1, ... in entry order, with their
    octave, an mvuRight >= 0 where stereo and their mvDepth.  kp_shift: (entry, value) plants one keypoint index by hand."""
    from sdslam_amd import capi
    r, q = rig(sd), c["q"]
    trk, rng = r["trk"], np.random.default_rng(seed)
    E, P = len(q["kf"]), len(q["off"]) - 1
    kp_of = np.zeros(E, np.int64)
    kps, descs = [], []
    ur, depth = -np.ones((B + 1, trk.cap), np.float32), -np.ones((B + 1, trk.cap), np.float32)
    for cam in list(range(B)) + [R.CUR]:
        e = np.flatnonzero(q["kf"] == cam)
        kp_of[e] = np.arange(len(e))
        k = np.zeros(max(len(e), 1), capi.KP_DTYPE)
        k["x"], k["y"], k["size"] = rng.uniform(20, W - 20, len(k)), rng.uniform(20, H - 20, len(k)), 31.0
        k["octave"][:len(e)] = q["octave"][e]
        kps.append(k)
        descs.append(rng.integers(0, 256, (len(k), 32)).astype(np.uint8))
        ur[cam, :len(e)] = np.where(q["stereo"][e] != 0, 100.0, -1.0)
        depth[cam, :len(e)] = q["depth"][e]
    r["ref"].set_keypoints(0, kps[:B], descs[:B])
    r["cur"].set_keypoints(0, [kps[B]] + [kps[B][:1]] * (B - 1), [descs[B]] + [descs[B][:1]] * (B - 1))
    trk.set_current_broadcast(-1)
    trk.set_camera(458.654, 457.296, 367.215, 248.375, 47.9, (0.0, float(W), 0.0, float(H)))
    trk.set_uright_ref(0, ur[:B])
    trk.set_uright(0, np.concatenate([ur[B:], -np.ones((B - 1, trk.cap), np.float32)]))
    trk.set_tri_depth(1, 0, depth[:B])
    if kp_shift is not None:
        kp_of[kp_shift[0]] = kp_shift[1]
    obs = [[(int(q["kf"][e]), int(kp_of[e]), int(q["kf_bad"][e])) for e in range(q["off"][i], q["off"][i + 1])] for i in range(P)]
    trk.set_observations(obs, q["ref_obs"], q["point_bad"])
    return obs


@pytest.mark.parametrize("name", ON_HANDLE)
def test_resident_path_equals_the_restatement(sd, name):
    c = CASES.get(name) or SMALL[name]
    trk = rig(sd)["trk"]
    plant(sd, c)
    want = want_of(c)
    runs = []
    for _ in range(2):
        trk.cull_keyframes(c["cand"], c["flags"], c["mono"], c["th"])
        runs.append(trk.get_culled())
    print(f"{name}: info8 {runs[0]['info8'].tolist()}")
    if want["info8"][0] == R.OK:
        assert R.differing(runs[0], want) == [] and same_bytes(runs[0], runs[1])
    else:
        assert runs[0]["info8"].tolist() == want["info8"].tolist() == runs[1]["info8"].tolist()


def test_resident_refusals_and_arguments(sd):
    from sdslam_amd import capi
    trk = rig(sd)["trk"]
    c = CASES["observations_4"]
    plant(sd, c, kp_shift=(2, 299))                                         # a keypoint index outside its frame
    trk.cull_keyframes(c["cand"], c["flags"], 0, CC.TH)
    assert trk.get_culled()["info8"].tolist() == [R.BAD_INDEX] + [0] * 7
    plant(sd, c)
    for cand, flags in (([B], [0]), ([-1], [0]), ([1, 1], [0, 0])):         # outside [0, max_batch), the current keyframe, twice
        with pytest.raises(capi.SdError) as err:
            trk.cull_keyframes(cand, flags, 0, CC.TH)
        assert err.value.code == 1
    trk.cull_keyframes([], [], 0, CC.TH)
    assert trk.get_culled()["info8"].tolist() == [0] * 8
    # a new handle holds -1 in the depth rows: with monocular = 0 every point is skipped
    trk.set_tri_depth(1, 0, -np.ones((B, trk.cap), np.float32))
    trk.cull_keyframes(c["cand"], c["flags"], 0, CC.TH)
    assert trk.get_culled()["counts2"].tolist() == [[0, 0]]
    trk.cull_keyframes(c["cand"], c["flags"], 1, CC.TH)
    assert trk.get_culled()["counts2"].tolist() == [[1, 1]]
