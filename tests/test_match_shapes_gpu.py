"""GPU parity of the matchers at the smallest shapes at which an LDS layout can go wrong: ~100 features per frame (the keypoint
capacity is no power of two; the LDS sorts run on 128 keys) and max_points = 77 (odd, no multiple of 32: every alignment pad of
the layouts in track_match_lds.h is non-zero somewhere and the last mask word is partial), and SearchByPoints at the edges of
its tile and row loops.  Integer work: match vectors and counts equal the oracle's."""
import numpy as np
import pytest

from sdslam_amd import synth

pytestmark = pytest.mark.gpu
K = (synth.FX, synth.FY, synth.CX, synth.CY)
CFG = (100, 1.2, 8, 20)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
MP = 77


@pytest.fixture(scope="module")
def small(oracle):
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    motions = [((0.02, -0.01, 0.015), (0.4, -0.3, 0.5)), ((-0.03, 0.02, -0.01), (-0.6, 0.2, 0.3))]
    B = len(motions)
    scenes = [synth.make_scene(20 + i, *m) for i, m in enumerate(motions)]
    cur, ref = sd.ORBextractor(*CFG, 640, 480, B), sd.ORBextractor(*CFG, 640, 480, B)
    ck, cd, cn = cur.extract_batch(np.stack([s["cur"] for s in scenes]))
    rk, rd, rn = ref.extract_batch(np.stack([s["ref"] for s in scenes]))
    cap = ck.shape[1]
    assert 64 < cap < 128 and cap & (cap - 1), cap      # no power of two; the sorts run on 128 keys
    fr = []
    for i, s in enumerate(scenes):
        k1, d1, k2, d2 = ck[i, :cn[i]], cd[i, :cn[i]], rk[i, :rn[i]], rd[i, :rn[i]]
        oc = oracle.OrbOracle(*CFG)
        ock, _ = oc.extract(s["cur"])
        assert np.array_equal(ock, k1)
        last = {k: v[:MP] for k, v in synth.tracking_case(i, k2, d2, max_points=MP).items()}
        fr.append(dict(ck=k1, cd=d1, rk=k2, rd=d2, last=last, sf=oc.tables()["sf"]))
    trk = sd.Tracker(cur, ref, max_points=MP, max_batch=B, pnp_max_iterations=8)
    trk.set_camera(*K, 0.0, BOUNDS)
    trk.set_last(0, [f["last"] for f in fr])
    trk.set_poses(0, [s["T_ref"] for s in scenes], [s["T_cur"] for s in scenes])
    yield dict(sd=sd, B=B, scenes=scenes, trk=trk, fr=fr, cap=cap)
    trk.close()
    cur.close()
    ref.close()


@pytest.mark.parametrize("split", [1, 0], ids=["split", "single"])
@pytest.mark.parametrize("th", [8.0, 64.0])
def test_search_by_projection_odd_max_points(oracle, small, split, th):
    trk, B = small["trk"], small["B"]
    with small["sd"].options({"track.match_split": split}):
        trk.match(B, th=th, mono=True, check_ori=True)
    cm, nm = trk.get_matches(0, B)
    for i in range(B):
        f, s = small["fr"][i], small["scenes"][i]
        n, ocm = oracle.search_by_projection(f["ck"], f["cd"], f["sf"], BOUNDS, K, s["T_cur"], s["T_ref"], f["last"], th=th, mono=True,
                                             check_ori=True)
        assert nm[i] == n, (th, i, nm[i], n)
        assert np.array_equal(cm[i, :len(ocm)], ocm) and (cm[i, len(ocm):] == -1).all()
        assert n >= 40      # the oracle finds 45 ... 49 on these inputs


def test_local_map_search_odd_max_points(oracle, small):
    trk, B = small["trk"], small["B"]
    T = [s["T_cur"] for s in small["scenes"]]
    cases = [{k: v[:MP] for k, v in synth.local_map_case(100 + i, small["fr"][i]["ck"], small["fr"][i]["cd"], T[i], n_extra=30).items()}
             for i in range(B)]
    trk.set_local(0, cases)
    trk.match_local(B, th=1.0, nnratio=0.8)
    g = trk.get_local(0, B)
    for i in range(B):
        f = small["fr"][i]
        n = len(f["ck"])
        r = oracle.search_local_points(f["ck"], f["cd"], f["sf"], np.log(np.float32(CFG[1])), BOUNDS, K, 0.0, T[i], cases[i], th=1.0,
                                       nnratio=0.8)
        assert np.array_equal(g["in_view"][i, :MP], r["in_view"]) and np.array_equal(g["level"][i, :MP], r["level"])
        assert g["n"][i] == r["n"], (i, g["n"][i], r["n"])
        assert np.array_equal(g["match"][i, :n], r["match"]) and (g["match"][i, n:] == -1).all()
        assert r["n"] >= 50      # the oracle finds 57 and 64


def test_search_by_points_small_capacity(oracle, small):
    trk, B, cap = small["trk"], small["B"], small["cap"]
    h = np.ones((B, cap), np.uint8)
    trk.set_point_flags(0, h, h)
    trk.search_by_points(B, 0.75, True)
    m, nm = trk.get_point_matches(0, B)
    for i in range(B):
        f = small["fr"][i]
        n1, n2 = len(f["ck"]), len(f["rk"])
        n, om = oracle.search_by_points(f["ck"], f["cd"], h[i, :n1], f["rk"], f["rd"], h[i, :n2], 0.75, True)
        assert nm[i] == n, (i, nm[i], n)
        assert np.array_equal(m[i, :n1], om) and (m[i, n1:] == -1).all()
        assert n >= 40      # the oracle finds 48 and 45


# ---- SearchByPoints at the edges of the brute-force scaffold (tiles of 512 pKF keypoints, passes of 512 currentKF rows)
BF_CFG = (1000, 1.2, 8, 20)


def _dots(points):
    """Isolated pixels of value 24 on black: FAST fires at level 0 only, one keypoint per dot"""
    img = np.zeros((480, 640), np.uint8)
    for x, y in points:
        img[y, x] = 24
    return img


@pytest.fixture(scope="module")
def bf_edges(oracle):
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    s0, s1 = synth.make_scene(20), synth.make_scene(23, (0.01, 0.03, 0.02), (0.2, 0.5, -0.8))
    blank = np.zeros((480, 640), np.uint8)
    pairs = [(blank, blank), (_dots([(320, 240)]), _dots([(200, 150), (322, 241), (451, 333)])), (s0["cur"], s0["ref"]),
             (s1["cur"], s1["ref"]), (s0["cur"], s0["ref"])]
    B = len(pairs)
    cur, ref = sd.ORBextractor(*BF_CFG, 640, 480, B), sd.ORBextractor(*BF_CFG, 640, 480, B)
    k1, d1, n1 = cur.extract_batch(np.stack([p[0] for p in pairs]))
    k2, d2, n2 = ref.extract_batch(np.stack([p[1] for p in pairs]))
    assert (n1[0], n2[0], n1[1], n2[1]) == (0, 0, 1, 3), (n1, n2)
    assert n2[2] > 513 and n1[3] >= 600, (n1, n2)
    cap = k1.shape[1]
    rng = np.random.default_rng(5)
    h1, h2 = np.ones((B, cap), np.uint8), np.ones((B, cap), np.uint8)
    h2[2, 513:] = 0                                            # 513 valid: the last one is the first bit of the second tile
    h1[3] = 0
    h1[3, rng.permutation(n1[3])[:600]] = 1                    # 600 valid rows: a second pass of 512
    h2[3] = rng.random(cap) > 0.3
    h1[4] = h2[4] = 0                                          # no point on either side holds a map point
    trk = sd.Tracker(cur, ref, max_points=1000, max_batch=B, pnp_max_iterations=8)
    trk.set_camera(*K, 0.0, BOUNDS)
    trk.set_point_flags(0, h1, h2)
    want = {}
    for ori in (True, False):
        want[ori] = [oracle.search_by_points(k1[b, :n1[b]], d1[b, :n1[b]], h1[b, :n1[b]], k2[b, :n2[b]], d2[b, :n2[b]], h2[b, :n2[b]], 0.75, ori)
                     for b in range(B)]
    assert int(h2[2, :n2[2]].sum()) == 513 and int(h1[3, :n1[3]].sum()) == 600
    assert want[False][2][0] > 100 and want[False][3][0] > 100      # the large cases are not vacuous
    yield dict(B=B, trk=trk, n1=n1, want=want)
    trk.close()
    cur.close()
    ref.close()


@pytest.mark.parametrize("check_ori", [True, False], ids=["ori", "no_ori"])
def test_search_by_points_edge_shapes(bf_edges, check_ori):
    """Slots: 0 x 0 keypoints | 1 x 3 | N2 = 513 valid | N1 = 600 valid | nothing valid on either side"""
    trk, B = bf_edges["trk"], bf_edges["B"]
    trk.search_by_points(B, 0.75, check_ori)
    m, nm = trk.get_point_matches(0, B)
    for b in range(B):
        n, om = bf_edges["want"][check_ori][b]
        n1 = bf_edges["n1"][b]
        assert nm[b] == n, (b, nm[b], n)
        assert np.array_equal(m[b, :n1], om) and (m[b, n1:] == -1).all(), b
    assert nm[0] == 0 and nm[4] == 0
