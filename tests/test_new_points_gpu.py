"""k_triangulate / k_new_points_resolve (sdslam_amd/csrc/track_newpoints_tri.hip) on the MI355X against the numpy restatement
tests/new_points_ref.py: the crafted pairs of tests/new_points_cases.py through the debug entry (verdict, branch and the bits of
Xw); the batched path on the six views of test_triangulation_gpu.py (paired and broadcast, monocular and with mvuRight / mvDepth
mixes), the restatement fed the device's own matches so that only the triangulation is under test; the resolved points (winner,
id, every field, bit for bit); lifetime, error codes, and queued = synchronised.

Stereo rows: the device's atan2f is not the host's, so every stereo row the batched scene uses must keep
new_points_ref.stereo_margin above 1e-5; asserted here on the rows the device actually matched."""
import collections

import numpy as np
import pytest

import new_points_cases as NC
import new_points_ref as NR
import test_triangulation_gpu as TG
import triangulation_cases as TC
import triangulation_ref as TR

pytestmark = pytest.mark.gpu
B, W, H = TG.B, TG.W, TG.H
CFG = (1000, 1.2, 8, 20)
BF = 40.0
CAM5 = np.array([*TC.K, BF], np.float32)
_RIG = {}


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def rig(sd):
    if not _RIG:
        cur, ref = sd.ORBextractor(*CFG, W, H, B), sd.ORBextractor(*CFG, W, H, B)
        ci, ri = TG.images()
        k1, d1, n1 = cur.extract_batch(ci)
        k2, d2, n2 = ref.extract_batch(ri)
        cap = k1.shape[1]
        trk = sd.Tracker(cur, ref, max_points=max(cap, 8), max_batch=B, pnp_max_iterations=8)
        trk.set_camera(*TC.K, BF, TG.BOUNDS)
        mono = np.full((B, cap), -1, np.float32)
        stereo = NC.batched_mix(k1, k2, TG.T_CUR, TG.T_REF, TC.K, BF)      # the scene tests/test_new_points_cpu.py checks
        has = np.zeros((B, cap), np.uint8)
        _RIG.update(trk=trk, cur=cur, ref=ref, imgs=(ci, ri), k1=k1, d1=d1, n1=n1, k2=k2, d2=d2, n2=n2, cap=cap, has=has,
                    stereo=stereo, mono=dict(u1=mono, u2=mono, z1=mono, z2=mono))
    return _RIG


def upload(r, mix, bc, median=None):
    trk = r["trk"]
    m = r[mix]
    trk.set_current_broadcast(-1)
    trk.set_poses(0, TG.T_REF, [TG.T_CUR[0]] * B if bc else TG.T_CUR)
    trk.set_point_flags(0, r["has"], r["has"])
    trk.set_uright(0, m["u1"])
    trk.set_uright_ref(0, m["u2"])
    trk.set_tri_depth(0, 0, m["z1"])
    trk.set_tri_depth(1, 0, m["z2"])
    trk.set_tri_median_depth(0, np.full(B, -1.0, np.float32) if median is None else median)
    trk.set_current_broadcast(0 if bc else -1)


def restate_slot(r, mix, b, bc, m12, monocular, median=-1.0, margins=None):
    f1 = 0 if bc else b
    m = r[mix]
    n1, n2 = int(r["n1"][f1]), int(r["n2"][b])
    return NR.triangulate(r["k1"][f1, :n1], r["k1"][f1, :n1], m["u1"][f1, :n1], m["z1"][f1, :n1], r["k2"][b, :n2], r["k2"][b, :n2],
                          m["u2"][b, :n2], m["z2"][b, :n2], m12[:n1], TG.T_CUR[f1], TG.T_REF[b], CAM5, TC.SF, TC.SIGMA2, 1.2, monocular,
                          median, margins)


def raw(trk):
    g, p = trk.get_triangulated(0, B), trk.get_new_points()
    return b"".join(np.ascontiguousarray(a).tobytes() for a in list(g.values()) + list(p.values()))


# ------------------------------------------------------------------------------------------------ 1. the debug entry
def test_debug_entry_is_bit_exact_on_every_case(sd):
    from sdslam_amd import capi
    seen = collections.Counter()
    for c, (v, b, X), _ in NC.cases_with_reference():
        gv, gb, gX = capi.debug_triangulate(c["k1u"], c["k1"], c["ur1"], c["z1"], c["k2u"], c["k2"], c["ur2"], c["z2"], c["m"], c["T1"],
                                            c["T2"], c["cam5"], c["sf"], c["sigma2"], c["scale_factor"], c["monocular"], c["median"])
        assert np.array_equal(gv, v), (c["name"], np.flatnonzero(gv != v)[:8], gv[gv != v][:8], v[gv != v][:8])
        assert np.array_equal(gb, b), (c["name"], np.flatnonzero(gb != b)[:8])
        bad = np.flatnonzero((gX.view(np.uint64) != X.view(np.uint64)).any(axis=1))
        assert bad.size == 0, (c["name"], bad[:8], gX[bad[:2]], X[bad[:2]])
        seen.update(gv.tolist())
    assert set(seen) == set(range(11))


def test_debug_entry_on_empty_and_unaligned_inputs(sd):
    """Both keyframes empty (nothing runs, nothing is written), and 1 keypoint against 3: counts that are no multiple of the 16
    bytes the entry's device arrays are carved in, KF1 shorter than the padded capacity."""
    from sdslam_amd import capi
    c = NC.count_case(1, 11)
    side1, side2 = ("k1u", "k1", "ur1", "z1"), ("k2u", "k2", "ur2", "z2")

    def run(c):
        return capi.debug_triangulate(c["k1u"], c["k1"], c["ur1"], c["z1"], c["k2u"], c["k2"], c["ur2"], c["z2"], c["m"], c["T1"], c["T2"],
                                      c["cam5"], c["sf"], c["sigma2"], c["scale_factor"], c["monocular"], c["median"])
    v, b, X = run(dict(c, m=c["m"][:0], **{k: c[k][:0] for k in side1 + side2}))
    assert len(v) == len(b) == len(X) == 0
    i = int(np.flatnonzero(c["m"] >= 0)[0])
    j = int(c["m"][i])
    rest = [k for k in range(len(c["k2"])) if k != j]
    one = dict(c, m=np.array([1], np.int32), **{k: c[k][[i]] for k in side1}, **{k: c[k][[rest[0], j, rest[1]]] for k in side2})
    want_v, want_b, want_X = NC.reference(one)
    v, b, X = run(one)
    assert want_v[0] == NR.ACCEPTED                            # the row does go through the triangulation
    assert np.array_equal(v, want_v) and np.array_equal(b, want_b) and X.tobytes() == want_X.tobytes()


# ------------------------------------------------------------------------------------------------ 2. the batched path, 3. resolve
@pytest.mark.parametrize("mix,monocular", [("mono", True), ("stereo", False)])
@pytest.mark.parametrize("bc", [False, True])
def test_batched_path_and_resolve(sd, mix, monocular, bc):
    r = rig(sd)
    trk = r["trk"]
    upload(r, mix, bc)
    first_id = [1000, 2000, 3000]
    try:
        trk.set_next_map_id(0, first_id)
        trk.search_for_triangulation(B, False, False)
        trk.triangulate(B, monocular)                          # queued behind the search: no host wait in between
        g = trk.get_triangulation_matches(0, B)
        t = trk.get_triangulated(0, B)
        pts = trk.get_new_points()
    finally:
        trk.set_current_broadcast(-1)
    verdicts, Xws, counts, margins = [], [], collections.Counter(), []
    for b in range(B):
        n1 = int(r["n1"][0 if bc else b])
        v, br, X = restate_slot(r, mix, b, bc, g["matches12"][b], monocular, margins=margins)
        assert np.array_equal(t["verdict"][b, :n1], v), (mix, bc, b, np.flatnonzero(t["verdict"][b, :n1] != v)[:8])
        assert np.array_equal(t["branch"][b, :n1], br), (mix, bc, b)
        assert t["Xw"][b, :n1].tobytes() == X.tobytes(), (mix, bc, b)
        assert (t["verdict"][b, n1:] == 0).all() and t["n_accepted"][b] == (v == NR.ACCEPTED).sum()
        verdicts.append(v)
        Xws.append(X)
        counts.update(v.tolist())
        print("slot %d %s bc=%d: %s" % (b, mix, bc, {NR.VERDICTS[k]: n for k, n in sorted(collections.Counter(v.tolist()).items())}))
        assert (v == NR.ACCEPTED).sum() >= 50, (mix, bc, b)     # coverage: at least 50 accepted points per pairing
    assert all(m > 1e-5 for m in margins) and (mix == "mono" or len(margins) > 20), (min(margins) if margins else None)
    if mix == "stereo":                                         # the scene's coverage, as the CPU test finds it on the oracle's keypoints
        assert counts[NR.LOW_PARALLAX] >= 5 and counts[NR.REPROJ1] + counts[NR.REPROJ2] >= 5 and counts[NR.SCALE] >= 5, counts
        acc = np.concatenate([t["branch"][b][t["verdict"][b] == NR.ACCEPTED] for b in range(B)])
        assert bc == 0 or set(np.unique(acc)) == {1, 2, 3}      # accepted points of every branch reach the resolve
    if bc:
        want, nid = NR.resolve(verdicts, g["matches12"], Xws, [TG.T_CUR[0]] * B, TG.T_REF, r["k1"][0], r["d1"][0], TC.SF, first_id, True)
    else:
        want, nid = NR.resolve(verdicts, g["matches12"], Xws, TG.T_CUR, TG.T_REF, r["k1"], r["d1"], TC.SF, first_id, False)
    assert pts["info"][0] == len(want) > 0 and pts["info"][1] == (0 if bc else -1) and pts["info"][2] == B
    got = [dict(kp1=int(pts["kp1"][i]), slot=int(pts["slot"][i]), idx2=int(pts["idx2"][i]), id=int(pts["id"][i]), Xw=pts["Xw"][i],
                normal=pts["normal"][i], max_dist=pts["max_dist"][i], min_dist=pts["min_dist"][i], desc=pts["desc"][i])
           for i in range(len(want))]
    assert NR.same_points(got, want)
    if bc:
        assert pts["info"][3] == nid[0] and len({p["kp1"] for p in got}) == len(got)
        assert sum(int((v == NR.ACCEPTED).sum()) for v in verdicts) > len(got)          # a later neighbour lost a keypoint
    # the counters advanced: a second run numbers on
    trk.set_current_broadcast(0 if bc else -1)
    try:
        trk.triangulate(B, monocular)
        again = trk.get_new_points()
    finally:
        trk.set_current_broadcast(-1)
    assert np.array_equal(again["id"], pts["id"] + (len(want) if bc else np.bincount(pts["slot"], minlength=B)[pts["slot"]]))


def test_monocular_gate_per_slot(sd):
    r = rig(sd)
    trk = r["trk"]
    upload(r, "mono", False, np.array([1e6, -1.0, 0.5], np.float32))      # slot 0: baseline / 1e6 < 0.01
    trk.search_for_triangulation(B, False, False)
    trk.triangulate(B, True)
    g, t = trk.get_triangulation_matches(0, B), trk.get_triangulated(0, B)
    m0 = g["matches12"][0] >= 0
    assert m0.sum() > 0 and (t["verdict"][0][m0] == NR.SLOT_GATED).all() and t["n_accepted"][0] == 0
    assert t["n_accepted"][1] > 0 and t["n_accepted"][2] > 0 and (t["verdict"][1:] != NR.SLOT_GATED).all()
    pts = trk.get_new_points()
    assert (pts["slot"] > 0).all()


# ------------------------------------------------------------------------------------------------ 4. lifetime and errors
def test_result_ends_with_its_inputs_and_errors(sd):
    r = rig(sd)
    trk = r["trk"]
    upload(r, "mono", False)
    for call in (lambda: trk.triangulate(B, True), lambda: trk.get_triangulated(0, B), trk.get_new_points):
        with pytest.raises(sd.SdError) as e:                   # upload() ended the search's result
            call()
        assert e.value.code == 1
    trk.search_for_triangulation(B, False, False)
    with pytest.raises(sd.SdError) as e:                       # searched, not triangulated
        trk.get_triangulated(0, B)
    assert e.value.code == 1
    m = r["mono"]
    ending = {
        "set_tri_depth": lambda: trk.set_tri_depth(1, 0, m["z2"]),
        "set_tri_median_depth": lambda: trk.set_tri_median_depth(0, np.full(B, -1.0, np.float32)),
        "set_camera": lambda: trk.set_camera(*TC.K, BF, TG.BOUNDS),
        "set_uright_ref": lambda: trk.set_uright_ref(0, m["u2"]),
        "set_poses": lambda: trk.set_poses(0, TG.T_REF, TG.T_CUR),
    }
    for name, call in ending.items():
        trk.search_for_triangulation(B, False, False)
        trk.triangulate(B, True)
        first = raw(trk)
        trk.get_triangulation_matches(0, B)
        assert raw(trk) == first                               # reading does not end it
        call()
        with pytest.raises(sd.SdError) as e:
            trk.get_triangulated(0, B)
        assert e.value.code == 1, name
        with pytest.raises(sd.SdError) as e:
            trk.get_new_points()
        assert e.value.code == 1, name
    trk.search_for_triangulation(2, False, False)
    trk.triangulate(2, True)
    trk.get_triangulated(0, 2)
    for bad in (lambda: trk.triangulate(B, True), lambda: trk.get_triangulated(0, B)):
        with pytest.raises(sd.SdError) as e:                   # more slots than the search / the triangulation covered
            bad()
        assert e.value.code == 1
    for n in (0, B + 1):
        with pytest.raises(sd.SdError) as e:
            trk.triangulate(n, True)
        assert e.value.code == 3
    # under the broadcast the search must have run without the rotation check (paired slots may use it)
    trk.search_for_triangulation(B, False, True)
    trk.triangulate(B, True)
    trk.set_current_broadcast(0)
    try:
        trk.search_for_triangulation(B, False, True)
        with pytest.raises(sd.SdError) as e:
            trk.triangulate(B, True)
        assert e.value.code == 1 and "check_ori" in str(e.value)
    finally:
        trk.set_current_broadcast(-1)
    with pytest.raises(sd.SdError) as e:
        trk.set_tri_depth(2, 0, m["z1"])
    assert e.value.code == 1
    with pytest.raises(sd.SdError) as e:
        trk.set_tri_depth(1, B, m["z1"][:1])
    assert e.value.code == 3
    trk.search_for_triangulation(B, False, False)
    trk.triangulate(B, True)
    L = trk.L
    info = np.zeros(4, np.int32)
    one = np.zeros(1, np.int32)
    assert L.sd_track_get_new_points(trk.h, info.ctypes.data, one.ctypes.data, None, None, None, None, None, None, None, None, 1) == 3
    assert info[0] > 1                                         # the count is reported before the capacity error
    assert L.sd_track_triangulate(None, B, 1) == 1


def test_queued_equals_synchronised(sd):
    r = rig(sd)
    trk = r["trk"]

    def run(sync):
        upload(r, "stereo", True)
        try:
            trk.set_next_map_id(0, [7, 8, 9])
            steps = [lambda: trk.search_for_triangulation(B, False, False), lambda: trk.triangulate(B, False),
                     lambda: trk.set_tri_median_depth(0, np.array([3.0, -1.0, 1e7], np.float32)),
                     lambda: trk.search_for_triangulation(B, False, False), lambda: trk.triangulate(B, True),
                     lambda: trk.set_next_map_id(0, [50, 60, 70]), lambda: trk.triangulate(B, True)]
            for s in steps:
                s()
                if sync:
                    trk.get_stereo(0, B)                       # a synchronising getter
            return raw(trk)
        finally:
            trk.set_current_broadcast(-1)
    queued = run(False)
    assert run(True) == queued
