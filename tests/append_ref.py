"""k_append_points / k_append_commit (sdslam_amd/csrc/track_append.hip) restated in numpy: the state of the local-map rows in,
the points of new_points_ref.resolve in, the state of the rows out; and the toy map on which the rule for `cand` and `obs` is
held to the reference's IsInKeyFrame / nObs (MapPoint::AddObservation src/MapPoint.cc:98-108, LocalMapping::CreateNewMapPoints
src/LocalMapping.cc:401-417).  Written from reading the reference; nothing here runs on a GPU."""
import numpy as np

import fuse_ref as FR

F32 = np.float32
FIELDS = (("cand", (), np.uint8), ("Xw", (3,), np.float64), ("normal", (3,), np.float64), ("min_dist", (), np.float32),
          ("max_dist", (), np.float32), ("mf_max_dist", (), np.float32), ("desc", (32,), np.uint8), ("obs", (), np.int32))


def sentinel_rows(B, M, n_local, seed=3):
    """Rows [B, M, ...] filled with bytes no append writes by accident (random, position-dependent), n = n_local."""
    rng = np.random.default_rng(seed)
    rows = dict(n=np.array(n_local, np.int32).copy())
    for k, tail, dt in FIELDS:
        raw = rng.integers(0, 256, (B, M) + tail + (np.dtype(dt).itemsize,), dtype=np.uint8)
        a = raw.view(dt).reshape((B, M) + tail)
        if dt in (np.float32, np.float64):
            a = np.where(np.isfinite(a), a, dt(1.5)).astype(dt)     # keep NaN payloads out: they need not survive a copy through numpy
        if k == "cand":
            a = (a & 1).astype(np.uint8) | 2                        # 2 or 3: neither value an append writes
        rows[k] = np.ascontiguousarray(a)
    return rows


def copy_rows(rows):
    return {k: v.copy() for k, v in rows.items()}


def n_obs(ur1_kp1, ur2_idx2):
    """nObs after AddObservation(KF1, kp1) and AddObservation(KF2, idx2): 2 for a keypoint with mvuRight >= 0, else 1."""
    return (2 if F32(ur1_kp1) >= 0 else 1) + (2 if F32(ur2_idx2) >= 0 else 1)


def append(rows, pts, bcast, n_slots, ur1, ur2, point_row, n_cand_rows):
    """rows: dict(n [B], cand [B, M], Xw, normal, min_dist, max_dist, mf_max_dist, desc, obs); pts: the point dicts of
    new_points_ref.resolve in creation order; bcast: the cur frame every slot pairs with, or -1; ur1 [frames, cap] / ur2 [B, cap]:
    mvuRight of the cur frames / the ref frames.  Returns (rows after, result [B, 3] = base | appended | dropped, position of every
    point in its row or -1 where it was dropped)."""
    out = copy_rows(rows)
    B, M = rows["cand"].shape
    base = np.clip(rows["n"], 0, M).astype(np.int64)
    arriving = np.zeros(B, np.int64)
    pos = np.full(len(pts), -1, np.int64)
    assert point_row >= 0 or bcast < 0
    for g, p in enumerate(pts):
        slot = int(p["slot"])
        row = point_row if point_row >= 0 else slot
        j = int(arriving[row])
        arriving[row] += 1
        if j >= M - base[row]:
            continue                                            # dropped: the first points stay, in order
        i = int(base[row]) + j
        pos[g] = i
        out["Xw"][row, i], out["normal"][row, i] = p["Xw"], p["normal"]
        out["mf_max_dist"][row, i] = F32(p["max_dist"])
        out["max_dist"][row, i] = F32(F32(1.2) * F32(p["max_dist"]))
        out["min_dist"][row, i] = F32(F32(0.8) * F32(p["min_dist"]))
        out["desc"][row, i] = p["desc"]
        fc = bcast if bcast >= 0 else slot
        out["obs"][row, i] = n_obs(ur1[fc][p["kp1"]], ur2[slot][p["idx2"]])
        if point_row >= 0:
            for f in range(n_cand_rows):
                out["cand"][f, i] = f != slot
        else:
            out["cand"][row, i] = 1
    appended = np.minimum(arriving, M - base)
    out["n"] = np.where(appended > 0, base + appended, rows["n"]).astype(np.int32)
    result = np.stack([base, appended, arriving - appended], 1).astype(np.int32)
    return out, result, pos


def mark_flags(has1, has2, pts, pos, bcast, n_slots):
    """AddMapPoint on both keyframes as the flags of sd_track_set_point_flags ([B, cap] each), for the appended points."""
    h1, h2 = np.array(has1, np.uint8).copy(), np.array(has2, np.uint8).copy()
    for p, i in zip(pts, pos):
        if i < 0:
            continue
        h2[p["slot"], p["idx2"]] = 1
        if bcast >= 0:
            h1[:n_slots, p["kp1"]] = 1
        else:
            h1[p["slot"], p["kp1"]] = 1
    return h1, h2


def rows_equal(got, want):
    """Byte for byte, every array and n; returns the name of the first field that differs, or None."""
    if int(got["n"]) != int(want["n"]):
        return "n"
    for k, _, _ in FIELDS:
        if np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(want[k]).tobytes():
            return k
    return None


def row_of(rows, r):
    return dict(n=int(rows["n"][r]), **{k: rows[k][r] for k, _, _ in FIELDS})


def as_set_local(rows, r):
    """Row r as the dict Tracker.set_local takes (all M entries: the bytes beyond n are uploaded too)."""
    return {k: rows[k][r] for k, _, _ in FIELDS}


# ---------------------------------------------------------------------------------------------------------------- toy map
class StereoMapPoint(FR.MapPoint):
    """fuse_ref's toy point with the reference's nObs: AddObservation counts 2 for a keypoint with mvuRight >= 0."""

    def __init__(self, name):
        super().__init__(name)
        self.nObs = 0

    def AddObservation(self, kf, idx):
        if kf in self.obs:
            return
        self.obs[kf] = idx
        self.nObs += 2 if F32(kf.mvuRight[idx]) >= 0 else 1


class StereoKeyFrame(FR.KeyFrame):
    def __init__(self, name, mvuRight):
        super().__init__(name, len(mvuRight))
        self.mvuRight = np.asarray(mvuRight, F32)


def toy_create(pts, kf1, neigh):
    """:401-417 on the toy map for the point dicts of create_new_map_points, in creation order."""
    made = []
    for p in pts:
        mp = StereoMapPoint(p["id"])
        kf2 = neigh[p["slot"]]
        mp.AddObservation(kf1, p["kp1"])
        mp.AddObservation(kf2, p["idx2"])
        kf1.AddMapPoint(mp, p["kp1"])
        kf2.AddMapPoint(mp, p["idx2"])
        made.append(mp)
    return made
