"""CPU (no GPU): the numpy restatement tests/new_points_ref.py and the crafted pairs tests/new_points_cases.py that
tests/test_new_points_gpu.py holds k_triangulate / k_new_points_resolve to -- the float Jacobi SVD against np.linalg.svd, noise-free
projections triangulating back to the planted point, every verdict code and branch reached by the crafted pairs and each row
reaching what it claims, the stereo margin of every crafted stereo row, "one broadcast search + triangulate + resolve" equal to
the reference's sequential loop point for point and id for id (3 neighbours and 20), and the new C entry points' presence and
argument checks."""
import collections

import numpy as np
import pytest

import new_points_cases as NC
import new_points_ref as NR
import triangulation_cases as TC
import triangulation_ref as TR
from sdslam_amd import synth

F32 = np.float32
NEW_CALLS = ["sd_track_set_tri_depth", "sd_track_set_tri_median_depth", "sd_track_triangulate", "sd_track_get_triangulated",
             "sd_track_get_new_points", "sd_debug_triangulate"]


def test_float_jacobi_svd_against_numpy():
    rng = np.random.default_rng(1)
    mats = [rng.normal(size=(4, 4)) for _ in range(40)]
    for _ in range(20):                                        # near-singular: one singular value ~1e-6 of the largest
        u, _, vt = np.linalg.svd(rng.normal(size=(4, 4)))
        mats.append(u @ np.diag([3.0, 1.0, 0.2, 3e-6]) @ vt)
    for A in mats:
        A = A.astype(F32)
        st = {}
        w, vt = NR.jacobi_svd_float(A, st)
        wn = np.linalg.svd(A.astype(np.float64), compute_uv=False)
        scale = wn[0]
        assert st["sweeps"] < 30
        assert np.abs(w - wn).max() <= 64 * 2.0 ** -24 * scale, (w, wn)          # float elements: a few float ulps of the norm
        assert np.abs(vt.astype(np.float64) @ vt.T.astype(np.float64) - np.eye(4)).max() < 1e-5
        # the last row spans the null direction: |A v| is of the order of the smallest singular value
        assert np.linalg.norm(A.astype(np.float64) @ vt[3].astype(np.float64)) <= wn[3] + 64 * 2.0 ** -24 * scale
        assert (np.diff(w) <= 0).all()


def test_noise_free_projections_triangulate_back():
    rng = np.random.default_rng(2)
    pr = NC.Pair("planted")
    Xs = [NC.world_point(NC.T1, rng.uniform(40, 600), rng.uniform(40, 440), rng.uniform(1.0, 6.0)) for _ in range(40)]
    for X in Xs:
        pr.row(X)
    v, b, Xw = NC.reference(pr.build())
    assert (v == NR.ACCEPTED).all() and (b == NR.BR_SVD).all()
    # keypoints are float pixels (2^-15 px at 300) seen over a 0.25 baseline at depth z: depth error ~ z^2 / (0.25 fx) * 2^-15
    for X, got in zip(Xs, Xw):
        z = NC.project(NC.T1, X)[2]
        assert np.linalg.norm(got - X) <= 50 * z * z / (0.25 * float(NC.CAM5[0])) * 2.0 ** -15, (X, got)


def test_every_verdict_and_branch_is_reached_and_claims_hold():
    seen, branches, names = collections.Counter(), collections.Counter(), set()
    for c, (v, b, X), _ in NC.cases_with_reference():
        names.add(c["name"])
        for i, (cv, cb) in c["claims"].items():
            assert cv is None or v[i] == cv, (c["name"], i, NR.VERDICTS[v[i]], NR.VERDICTS[cv])
            assert cb is None or b[i] == cb, (c["name"], i, b[i], cb)
        assert ((v == NR.NO_MATCH) == (c["m"] < 0)).all()
        seen.update(v.tolist())
        branches.update(b.tolist())
        if c["name"].startswith("count_"):
            assert (c["m"] >= 0).sum() == int(c["name"].split("_")[1])
    assert set(seen) == set(range(len(NR.VERDICTS))), seen
    assert set(branches) == {NR.BR_NONE, NR.BR_SVD, NR.BR_UNPROJECT1, NR.BR_UNPROJECT2}
    assert {"count_0", "count_1", "count_64", "count_65", "w_zero", "rank_deficient"} <= names
    steps = next(c for c, _, _ in NC.cases_with_reference() if c["name"] == "thresholds")["steps"]
    assert steps == dict(parallax=(NR.ACCEPTED, NR.LOW_PARALLAX), reproj1=(NR.ACCEPTED, NR.REPROJ1), reproj2=(NR.ACCEPTED, NR.REPROJ2),
                         scale=(NR.ACCEPTED, NR.SCALE))


def test_stereo_margin_of_every_crafted_stereo_row():
    n = 0
    for c, _, margins in NC.cases_with_reference():
        stereo_rows = int((((c["ur1"] >= 0) | (c["ur2"][np.maximum(c["m"], 0)] >= 0)) & (c["m"] >= 0)).sum())
        gated = c["name"].endswith("_shut")
        assert len(margins) == (0 if gated else stereo_rows), c["name"]
        assert all(m > NC.MARGIN for m in margins), (c["name"], min(margins))
        n += len(margins)
    assert n >= 15


_SCENE = {}


def batched_scene(oracle):
    """The batched scene of tests/test_new_points_gpu.py on the oracle's keypoints (they are the device's): the stereo mix of
    new_points_cases.batched_mix, paired and broadcast, searched and triangulated by the restatements.  Computed once.
    {(broadcast, slot): (verdict, branch)} and the stereo margins of every matched stereo row."""
    if not _SCENE:
        import test_triangulation_gpu as TG
        sc = TG.scene(dict(cfg=(1000, 1.2, 8, 20)), oracle=oracle)
        bf = 40.0
        mix = NC.batched_mix(sc["k1"], sc["k2"], TG.T_CUR, TG.T_REF, TC.K, bf)
        cam5 = np.array([*TC.K, bf], F32)
        res, margins = {}, []
        for bc, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2)):
            f1 = 0 if bc else b
            n1, n2 = int(sc["n1"][f1]), int(sc["n2"][b])
            T1, T2 = TG.T_CUR[f1], TG.T_REF[b]
            k1, k2, none1, none2 = sc["k1"][f1, :n1], sc["k2"][b, :n2], np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
            _, m12 = TR.search_for_triangulation(k1, sc["d1"][f1, :n1], none1, mix["u1"][f1, :n1], k2, sc["d2"][b, :n2], none2,
                                                 mix["u2"][b, :n2], TR.compute_f12(T1, T2, TC.K), TR.epipole(T1, T2, TC.K), TC.SF, TC.SIGMA2)
            v, br, _ = NR.triangulate(k1, k1, mix["u1"][f1, :n1], mix["z1"][f1, :n1], k2, k2, mix["u2"][b, :n2], mix["z2"][b, :n2], m12,
                                      T1, T2, cam5, TC.SF, TC.SIGMA2, 1.2, False, -1.0, margins)
            res[(bc, b)] = (v, br)
        res[(1, 0)] = res[(0, 0)]                               # the broadcast's slot 0 is the paired slot 0
        _SCENE.update(res=res, margins=margins)
    return _SCENE


def test_batched_scene_meets_the_coverage_and_margin_conditions(oracle):
    s = batched_scene(oracle)
    for bc in (0, 1):
        counts = collections.Counter()
        for b in range(3):
            v, br = s["res"][(bc, b)]
            assert (v == NR.ACCEPTED).sum() >= 50, (bc, b)
            counts.update(v.tolist())
        assert counts[NR.LOW_PARALLAX] >= 5 and counts[NR.REPROJ1] + counts[NR.REPROJ2] >= 5 and counts[NR.SCALE] >= 5, (bc, counts)
    accepted = np.concatenate([br[v == NR.ACCEPTED] for v, br in s["res"].values()])
    assert set(np.unique(accepted)) == {NR.BR_SVD, NR.BR_UNPROJECT1, NR.BR_UNPROJECT2}
    assert len(s["margins"]) > 100 and min(s["margins"]) > NC.MARGIN, min(s["margins"])


def _keyframes(n_neigh, n_kp, seed):
    """One keyframe and n_neigh neighbours looking at the same random points, descriptors a few bits apart, some keypoints
    stereo, some already holding a map point; neighbour 1 too close (gated), octaves mixed so that scale rejects some."""
    rng = np.random.default_rng(seed)
    T1 = NC.T1
    Xs = [NC.world_point(T1, rng.uniform(30, 610), rng.uniform(30, 450), rng.uniform(1.5, 6.0)) for _ in range(n_kp)]
    desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)

    def frame(T, jitter):
        k = np.zeros(n_kp, NC.KP_DTYPE)
        uvz = np.array([NC.project(T, X) for X in Xs])
        k["x"], k["y"] = (uvz[:, 0] + rng.normal(0, jitter, n_kp)).astype(F32), (uvz[:, 1] + rng.normal(0, jitter, n_kp)).astype(F32)
        k["octave"] = rng.integers(0, 8, n_kp)
        st = rng.random(n_kp) < 0.25
        ur = np.where(st, uvz[:, 0] - float(NC.CAM5[4]) / uvz[:, 2], -1).astype(F32)
        z = np.where(st, uvz[:, 2], -1).astype(F32)
        d = np.array([TC.flip(desc[i], rng.choice(256, int(rng.integers(0, 12)), replace=False)) for i in range(n_kp)])
        return k, d, ur, z
    k1, d1, ur1, z1 = frame(T1, 0.0)
    has1 = (rng.random(n_kp) < 0.2).astype(np.uint8)
    neigh = []
    for b in range(n_neigh):
        step = 0.004 if b == 1 else rng.uniform(0.15, 0.4)
        ang = rng.uniform(0, 2 * np.pi)
        T = synth.se3_exp((step * np.cos(ang), step * np.sin(ang), rng.uniform(-0.05, 0.05)), rng.uniform(-2, 2, 3)) @ T1
        k, d, ur, z = frame(T, 0.5)
        perm = rng.permutation(n_kp)
        neigh.append(dict(ku=k[perm], k=k[perm], d=d[perm], ur=ur[perm], z=z[perm], has=(rng.random(n_kp) < 0.3).astype(np.uint8), T=T,
                          median=3.5))
    return dict(k1=k1, d1=d1, ur1=ur1, z1=z1, has1=has1, T1=T1, neigh=neigh)


@pytest.mark.parametrize("n_neigh", [3, 20])
def test_one_broadcast_pass_equals_the_sequential_loop(n_neigh):
    kf = _keyframes(n_neigh, 48, 40 + n_neigh)
    K = tuple(float(v) for v in NC.CAM5[:4])
    log = []
    want = NR.create_new_map_points(kf["k1"], kf["k1"], kf["d1"], kf["has1"], kf["ur1"], kf["z1"], kf["neigh"], kf["T1"], NC.CAM5, NC.SF,
                                    NC.SIGMA2, NC.SCALE_FACTOR, True, 500, log)
    # the device's way: every neighbour searched with the ORIGINAL flags, every match triangulated, then the in-order resolve
    verdicts, matches, Xws = [], [], []
    for nb in kf["neigh"]:
        F12, epi = TR.compute_f12(kf["T1"], nb["T"], K), TR.epipole(kf["T1"], nb["T"], K)
        _, m12 = TR.search_for_triangulation(kf["k1"], kf["d1"], kf["has1"], kf["ur1"], nb["ku"], nb["d"], nb["has"], nb["ur"], F12, epi,
                                             NC.SF, NC.SIGMA2, False)
        v, _, X = NR.triangulate(kf["k1"], kf["k1"], kf["ur1"], kf["z1"], nb["ku"], nb["k"], nb["ur"], nb["z"], m12, kf["T1"], nb["T"],
                                 NC.CAM5, NC.SF, NC.SIGMA2, NC.SCALE_FACTOR, True, nb["median"])
        verdicts.append(v)
        matches.append(m12)
        Xws.append(X)
    got, nid = NR.resolve(verdicts, matches, Xws, [kf["T1"]] * n_neigh, [nb["T"] for nb in kf["neigh"]], kf["k1"], kf["d1"], NC.SF, [500],
                          True)
    assert NR.same_points(got, want)
    assert len(want) >= 10 and nid[0] == 500 + len(want) and [p["id"] for p in want] == list(range(500, 500 + len(want)))
    assert (verdicts[1][matches[1] >= 0] == NR.SLOT_GATED).all() and all(b != 1 for b, _, _, _ in log)      # the gated neighbour
    assert len({p["slot"] for p in want}) >= 2                                                  # later neighbours contribute ...
    assert sum(int((v == NR.ACCEPTED).sum()) for v in verdicts) > len(want)                     # ... and lose keypoints to earlier ones
    assert any(v != NR.ACCEPTED for _, _, _, v in log)


def test_entry_points_exist_and_check_their_arguments():
    import ctypes as C
    import sdslam_amd
    from sdslam_amd import build, capi
    build.build()
    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in capi._SIGNATURES, name
    assert L.sd_track_triangulate(None, 1, 1) == 1 and b"NULL" in L.sd_last_error()
    assert L.sd_track_set_tri_depth(None, 0, 0, 1, None, 1) == 1
    assert L.sd_track_get_new_points(None, None, None, None, None, None, None, None, None, None, None, 0) == 1
    # the debug entry checks before it touches a device: capacity, NULL arrays, a match outside KF2
    k = np.zeros(2, capi.KP_DTYPE)
    f, m, T, cam = np.zeros(2, F32), np.array([0, 5], np.int32), np.eye(4).ravel(), np.array(NC.CAM5)
    v, X = np.zeros(2, np.uint8), np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = lambda n1, n2, mm: (n1, n2, p(k), p(k), p(f), p(f), p(k), p(k), p(f), p(f), p(mm), p(T), p(T), p(cam), p(NC.SF), p(NC.SIGMA2), 8,
                               1.2, 1, -1.0, p(v), p(v), p(X))
    assert L.sd_debug_triangulate(*args(2, 2, m)) == 1 and b"matches12" in L.sd_last_error()
    assert L.sd_debug_triangulate(*args(4096, 2, m)) == 3
    assert L.sd_debug_triangulate(*args(0, 0, m)) == 0
