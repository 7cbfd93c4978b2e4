"""k_append_points / k_append_commit (sdslam_amd/csrc/track_append.hip) on the MI355X against the numpy restatement
tests/append_ref.py, on the three VGA views of test_new_points_gpu.py with max_points a little above the keypoint capacity.  The
restatement is fed the device's own new points (sd_track_get_new_points, which test_new_points_gpu.py holds to the resolve's
restatement), so only the append is under test: the rows through sd_track_get_local_points byte for byte (row and paired mode,
mono and the stereo mix, every base, a sentinel in every byte the append must not touch); search -> triangulate -> append -> fuse
equal to the host's round trip; mark_flags equal to a host sd_track_set_point_flags; lifetime, error codes; queued = synchronised."""
import numpy as np
import pytest

import append_ref as AR
import new_points_cases as NC
import test_triangulation_gpu as TG
import triangulation_cases as TC

pytestmark = pytest.mark.gpu
B, W, H = TG.B, TG.W, TG.H
CFG = (1000, 1.2, 8, 20)
BF = 40.0
EXTRA = 19                                 # max_points = keypoint capacity + 19: no multiple of a wave, of 16 bytes or of a tile
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
        trk = sd.Tracker(cur, ref, max_points=cap + EXTRA, max_batch=B, pnp_max_iterations=8)
        trk.set_camera(*TC.K, BF, TG.BOUNDS)
        mono = np.full((B, cap), -1, np.float32)
        stereo = NC.batched_mix(k1, k2, TG.T_CUR, TG.T_REF, TC.K, BF)
        _RIG.update(trk=trk, cur=cur, ref=ref, k1=k1, k2=k2, n1=n1, n2=n2, cap=cap, M=cap + EXTRA, has=np.zeros((B, cap), np.uint8),
                    stereo=stereo, mono=dict(u1=mono, u2=mono, z1=mono, z2=mono))
    return _RIG


def upload(r, mix, bc, median=None, has=None):
    trk, m = r["trk"], r[mix]
    h1, h2 = (r["has"], r["has"]) if has is None else has
    trk.set_current_broadcast(-1)
    trk.set_poses(0, TG.T_REF, [TG.T_CUR[0]] * B if bc else TG.T_CUR)
    trk.set_point_flags(0, h1, h2)
    trk.set_uright(0, m["u1"])
    trk.set_uright_ref(0, m["u2"])
    trk.set_tri_depth(0, 0, m["z1"])
    trk.set_tri_depth(1, 0, m["z2"])
    trk.set_tri_median_depth(0, np.full(B, -1.0, np.float32) if median is None else median)
    trk.set_next_map_id(0, [1000, 2000, 3000])
    trk.set_current_broadcast(0 if bc else -1)


def put_rows(trk, rows):
    """All B rows with every byte of every array, n_local as given (Tracker.set_local takes n_local from the arrays' length)."""
    p = lambda a: np.ascontiguousarray(a).ctypes.data
    arrays = [np.ascontiguousarray(rows[k]) for k, _, _ in AR.FIELDS]
    n = np.ascontiguousarray(rows["n"], np.int32)
    rc = trk.L.sd_track_set_local(trk.h, 0, B, p(n), *[p(a) for a in arrays], None)
    assert rc == 0, trk.L.sd_last_error()


def read_rows(trk):
    return [trk.get_local_points(b) for b in range(B)]


def device_points(trk):
    g = trk.get_new_points()
    pts = [dict(kp1=int(g["kp1"][i]), slot=int(g["slot"][i]), idx2=int(g["idx2"][i]), id=int(g["id"][i]), Xw=g["Xw"][i],
                normal=g["normal"][i], max_dist=g["max_dist"][i], min_dist=g["min_dist"][i], desc=g["desc"][i])
           for i in range(int(g["info"][0]))]
    return pts, g["info"]


def check_rows(trk, want, result, where):
    got = read_rows(trk)
    for b in range(B):
        bad = AR.rows_equal(got[b], AR.row_of(want, b))
        assert bad is None, (where, b, bad)
    ap = trk.get_appended(0, B)
    assert np.array_equal(np.stack([ap["base"], ap["appended"], ap["dropped"]], 1), result), (where, ap, result)


# ------------------------------------------------------------------------------------------------ 1. the rows, byte for byte
@pytest.mark.parametrize("mix,monocular", [("mono", True), ("stereo", False)])
@pytest.mark.parametrize("paired", [False, True])
def test_rows_equal_the_restatement(sd, mix, monocular, paired):
    r = rig(sd)
    trk, M, m = r["trk"], r["M"], r[mix]
    bc = -1 if paired else 0
    row = -1 if paired else 1                                  # row mode appends to row 1: a row offset that is not 0
    upload(r, mix, not paired)
    try:
        trk.search_for_triangulation(B, False, False)
        trk.triangulate(B, monocular)
        pts, info = device_points(trk)
        per_row = np.bincount([p["slot"] for p in pts], minlength=B) if paired else np.array([0, len(pts), 0])
        assert len(pts) >= 150 and (not paired or per_row.min() >= 50)
        assert M > r["cap"] and info[1] == bc and info[2] == B
        cases = {"base 0": np.zeros(B, int), "base 5": np.array([5, 5, 5]), "mid-way": M - per_row // 2 - (per_row == 0) * 7,
                 "full": np.array([M, M, M]), "mixed": np.array([M - 1, 0, 5]) if paired else np.array([3, M - 1, 2])}
        for name, bases in cases.items():
            if name != "base 0":
                trk.triangulate(B, monocular)                  # a new result: the last one has been appended
                pts, _ = device_points(trk)                    # (the ids count on)
            rows = AR.sentinel_rows(B, M, bases, seed=len(name))
            put_rows(trk, rows)
            trk.append_new_points(row, 0 if paired else B, False)
            want, result, pos = AR.append(rows, pts, bc, B, m["u1"], m["u2"], row, 0 if paired else B)
            check_rows(trk, want, result, (mix, paired, name))
            appended = result[:, 1]
            if name in ("base 0", "base 5"):
                assert appended.sum() == len(pts) and result[:, 2].sum() == 0
            if name == "mid-way":
                assert ((appended > 0) & (result[:, 2] > 0))[per_row > 0].all()      # the list is cut inside every receiving row
            if name == "full":
                assert appended.sum() == 0 and result[:, 2].sum() == len(pts) and np.array_equal(want["n"], rows["n"])
            if name == "base 5" and mix == "stereo" and not paired:
                seen = set(np.concatenate([want["obs"][b, 5:5 + appended[b]] for b in range(B)]).tolist())
                assert seen == {2, 3, 4}, seen
            again, _ = device_points(trk)                      # the list stays readable after the append
            assert [p["id"] for p in again] == [p["id"] for p in pts]
    finally:
        trk.set_current_broadcast(-1)


def test_a_result_without_points_changes_nothing(sd):
    r = rig(sd)
    trk, M = r["trk"], r["M"]
    for paired in (False, True):
        upload(r, "mono", not paired, median=np.full(B, 1e6, np.float32))           # every slot's baseline gate shuts
        try:
            trk.search_for_triangulation(B, False, False)
            trk.triangulate(B, True)
            rows = AR.sentinel_rows(B, M, [5, 17, M])
            put_rows(trk, rows)
            trk.append_new_points(-1 if paired else 1, 0 if paired else B, True)
            pts, info = device_points(trk)
            assert pts == [] and info[0] == 0
            check_rows(trk, rows, np.array([[5, 0, 0], [17, 0, 0], [M, 0, 0]], np.int32), paired)
        finally:
            trk.set_current_broadcast(-1)


# ------------------------------------------------------------------------------------------------ 2. the chain
def chain_rows(r):
    rows = AR.sentinel_rows(B, r["M"], [5, 0, 0], seed=11)
    rows["cand"][:, :5] = 0                                    # the five sentinel points before the base are no candidates
    return rows


def test_chain_equals_the_host_round_trip(sd):
    r = rig(sd)
    trk, m = r["trk"], r["stereo"]
    upload(r, "stereo", True)
    try:
        rows = chain_rows(r)
        put_rows(trk, rows)
        trk.search_for_triangulation(B, False, False)          # the device chain: nothing between the calls waits
        trk.triangulate(B, False)
        trk.append_new_points(0, B, False)
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)
        dev = trk.get_fuse(0, B)
        pts, _ = device_points(trk)                            # the host path: download, rebuild the rows, upload, search
        want, result, pos = AR.append(rows, pts, 0, B, m["u1"], m["u2"], 0, B)
        put_rows(trk, want)
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)
        host = trk.get_fuse(0, B)
    finally:
        trk.set_current_broadcast(-1)
    for k in ("best_idx", "best_dist", "n_found"):
        assert np.array_equal(dev[k], host[k]), k
    assert result[0].tolist() == [5, len(pts), 0] and len(pts) >= 150
    found = []
    for f in range(B):
        own = np.array([pos[g] for g, p in enumerate(pts) if p["slot"] == f])
        other = np.array([pos[g] for g, p in enumerate(pts) if p["slot"] != f])
        assert (dev["best_idx"][f, own] == -1).all() and (dev["best_dist"][f, own] == 256).all()
        found.append(int((dev["best_idx"][f, other] >= 0).sum()))
        assert (dev["best_idx"][f, :5] == -1).all() and (dev["best_idx"][f, 5 + len(pts):] == -1).all()
    print("appended points found in a neighbour other than their own:", found, "n_found", dev["n_found"])
    assert all(n >= 1 for n in found), found                   # the coverage tests/test_append_points_cpu.py finds on the oracle's keypoints


# ------------------------------------------------------------------------------------------------ 3. mark_flags
@pytest.mark.parametrize("paired", [False, True])
def test_mark_flags_equals_host_point_flags(sd, paired):
    r = rig(sd)
    trk = r["trk"]
    rng = np.random.default_rng(8)
    has = ((rng.random((B, r["cap"])) < 0.1).astype(np.uint8), (rng.random((B, r["cap"])) < 0.1).astype(np.uint8))
    if not paired:
        has = (np.stack([has[0][0]] * B), has[1])              # the one KF1's flags, in every slot's row
    bc = -1 if paired else 0
    upload(r, "mono", not paired, has=has)
    try:
        trk.search_for_triangulation(B, False, False)
        trk.triangulate(B, True)
        M = r["M"]
        base = np.array([M - 40, M - 40, M - 40]) if paired else np.array([0, M - 120, 0])      # some points are dropped: not flagged
        rows = AR.sentinel_rows(B, M, base)
        put_rows(trk, rows)
        trk.append_new_points(-1 if paired else 1, 0 if paired else B, True)
        trk.search_for_triangulation(B, False, False)          # queued behind the append: it reads the flags the kernel wrote
        dev = trk.get_triangulation_matches(0, B)
        pts, _ = device_points(trk)                            # still readable: the append's own record
        _, result, pos = AR.append(rows, pts, bc, B, r["mono"]["u1"], r["mono"]["u2"], -1 if paired else 1, 0 if paired else B)
        assert (pos >= 0).sum() >= 40 and (pos < 0).sum() >= 40
        h1, h2 = AR.mark_flags(has[0], has[1], pts, pos, bc, B)
        trk.set_point_flags(0, h1, h2)
        trk.search_for_triangulation(B, False, False)
        host = trk.get_triangulation_matches(0, B)
    finally:
        trk.set_current_broadcast(-1)
    assert np.array_equal(dev["matches12"], host["matches12"]) and np.array_equal(dev["n_matches"], host["n_matches"])
    assert dev["n_matches"].sum() > 0
    for p, i in zip(pts, pos):
        if i >= 0:
            slots = range(B) if not paired else [p["slot"]]
            assert all(dev["matches12"][f, p["kp1"]] == -1 for f in slots), p["kp1"]
            assert not (dev["matches12"][p["slot"]] == p["idx2"]).any()
    dropped = [p for p, i in zip(pts, pos) if i < 0]
    assert any(dev["matches12"][p["slot"], p["kp1"]] >= 0 for p in dropped)       # a dropped point's keypoints stay free


# ------------------------------------------------------------------------------------------------ 4. lifetime and errors
def test_lifetime_and_errors(sd):
    r = rig(sd)
    trk = r["trk"]

    def refused(call, code=1):
        with pytest.raises(sd.SdError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        return str(e.value)
    upload(r, "mono", True)
    try:
        put_rows(trk, chain_rows(r))
        refused(lambda: trk.append_new_points(0, B, False))    # no triangulation: upload() ended the search's result
        refused(lambda: trk.get_appended(0, B))                # no append since sd_track_set_local
        trk.search_for_triangulation(B, False, False)
        refused(lambda: trk.append_new_points(0, B, False))    # searched, not triangulated
        trk.triangulate(B, True)
        put_rows(trk, chain_rows(r))
        for bad in (lambda: trk.append_new_points(-2, B, False), lambda: trk.append_new_points(B, B, False),
                    lambda: trk.append_new_points(0, -1, False), lambda: trk.append_new_points(0, B + 1, False),
                    lambda: trk.append_new_points(0, B, 2)):
            refused(bad)
        assert "broadcast" in refused(lambda: trk.append_new_points(-1, 0, False))      # a broadcast result has no paired rows
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)
        trk.get_fuse(0, B)
        trk.append_new_points(0, B, False)                     # none of the refusals above spent the result
        refused(lambda: trk.get_fuse(0, B))                    # the rows it searched have changed
        assert "already" in refused(lambda: trk.append_new_points(0, B, False))         # a second append would duplicate the points
        pts, info = device_points(trk)                         # the list stays: kp1, slot, idx2, id for the caller's objects
        ap = trk.get_appended(0, B)
        assert len(pts) == info[0] == ap["appended"][0] > 0 and ap["base"].tolist() == [5, 0, 0] and ap["dropped"].sum() == 0
        trk.get_triangulated(0, B)                             # the triangulation's own result lives on
        refused(lambda: trk.get_appended(0, B + 1), 3)
        refused(lambda: trk.get_appended(B, 1), 3)
        refused(lambda: trk.get_local_points(B), 3)
        refused(lambda: trk.get_local_points(-1), 3)
        L = trk.L
        assert L.sd_track_get_local_points(trk.h, 0, None, np.zeros(4, np.uint8).ctypes.data, *[None] * 7, 4) == 3
        n = np.zeros(1, np.int32)
        assert L.sd_track_get_local_points(trk.h, 0, n.ctypes.data, *[None] * 8, 0) == 0 and n[0] == 5 + len(pts)
        put_rows(trk, chain_rows(r))                           # sd_track_set_local ends the append's result
        refused(lambda: trk.get_appended(0, B))
        trk.get_new_points()                                   # ... but not the triangulation
        refused(lambda: trk.append_new_points(0, B, False))    # (still the appended one)
        trk.triangulate(B, True)
        trk.append_new_points(0, B, True)                      # mark_flags: the search's result goes, the list stays
        refused(lambda: trk.get_triangulated(0, B))
        refused(lambda: trk.get_triangulation_matches(0, B))
        refused(lambda: trk.triangulate(B, True))
        assert device_points(trk)[1][0] == len(pts)
        trk.get_appended(0, B)
        trk.search_for_triangulation(B, False, False)
        trk.triangulate(B, True)                               # a new triangulation overwrites the list: the append's result ends
        refused(lambda: trk.get_appended(0, B))
        trk.get_new_points()
    finally:
        trk.set_current_broadcast(-1)
    assert trk.L.sd_track_append_new_points(None, 0, 0, 0) == 1


# ------------------------------------------------------------------------------------------------ 5. queued = synchronised
def test_queued_equals_synchronised(sd):
    r = rig(sd)
    trk = r["trk"]

    def run(sync):
        upload(r, "stereo", True)
        try:
            steps = [lambda: put_rows(trk, chain_rows(r)), lambda: trk.search_for_triangulation(B, False, False),
                     lambda: trk.triangulate(B, False), lambda: trk.append_new_points(0, B, True),
                     lambda: trk.fuse(B, kf_side=1, point_row=0, th=3.0), lambda: trk.search_for_triangulation(B, False, False),
                     lambda: trk.triangulate(B, False), lambda: trk.append_new_points(0, B, False),
                     lambda: trk.fuse(B, kf_side=1, point_row=0, th=3.0)]
            for s in steps:
                s()
                if sync:
                    trk.get_stereo(0, B)                       # a synchronising getter
            out = [a for row in read_rows(trk) for a in row.values()] + list(trk.get_fuse(0, B).values())
            out += list(trk.get_appended(0, B).values()) + list(trk.get_new_points().values())
            return b"".join(np.ascontiguousarray(a).tobytes() for a in out)
        finally:
            trk.set_current_broadcast(-1)
    queued = run(False)
    assert len(queued) > 0 and run(True) == queued
