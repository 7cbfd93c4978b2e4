"""LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:580-634) and the erasure of observations, restated with small
Python objects whose methods are the reference's statements one for one:

    KeyFrame.SetBadFlag           src/KeyFrame.cc:430-446 (the map-point part; the covisibility graph is the caller's)
    KeyFrame.EraseMapPointMatch   src/KeyFrame.cc
    MapPoint.EraseObservation     src/MapPoint.cc:110-134
    MapPoint.SetBadFlag           src/MapPoint.cc:146-161

A problem is the dict sd_debug_cull_keyframes takes: off [P + 1], and per entry kf (an index into n_kf keyframes, -1 the current
keyframe, -2 not resident), octave, stereo (mvuRight >= 0), depth (mvDepth at its keypoint); per point ref_obs (the position of
mpRefKF in its list) and point_bad or None; n_kf.  A keyframe appears at most once in a point's list (mObservations is a map),
and the list's order is the map's iteration order.  A point whose point_bad is set is a point SetBadFlag() has already been called
on: it has no observations and is nobody's match, so its entries take part in nothing and are reported as uploaded.

The thresholds the reference writes as literals are arguments here (th_obs = 3, ratio = 0.9, oct_slack = 1, bad_at = 2), so a test
can move each gate by one and see the stated output change."""
import numpy as np

OK, NOT_RESIDENT, BAD_INDEX = 0, 1, 2
SKIPPED_ID0, KEPT, CULLED, TO_BE_ERASED = 0, 1, 2, 3
CUR = -1


class KeyFrame:
    def __init__(self, index, mnId=1, mbNotErase=False):
        self.index, self.mnId, self.mbNotErase = index, mnId, mbNotErase
        self.mbToBeErased = self.mbBad = False
        self.mvpMapPoints, self.octave, self.mvuRight, self.mvDepth, self.entry = [], [], [], [], []

    def add_keypoint(self, pMP, octave, stereo, depth, entry):
        self.mvpMapPoints.append(pMP)
        self.octave.append(int(octave))
        self.mvuRight.append(1.0 if stereo else -1.0)
        self.mvDepth.append(np.float32(depth))
        self.entry.append(entry)
        return len(self.mvpMapPoints) - 1

    def EraseMapPointMatch(self, idx):
        self.mvpMapPoints[idx] = None

    def SetBadFlag(self):
        if self.mnId == 0:
            return
        elif self.mbNotErase:
            self.mbToBeErased = True
            return
        for i in range(len(self.mvpMapPoints)):
            if self.mvpMapPoints[i] is not None:
                self.mvpMapPoints[i].EraseObservation(self, how=1)
        self.mbBad = True


class MapPoint:
    def __init__(self, world, bad_at):
        self.world, self.bad_at = world, bad_at
        self.mObservations = {}          # KeyFrame -> idx, in list order
        self.nObs, self.mpRefKF, self.mbBad = 0, None, False

    def AddObservation(self, pKF, idx):
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx
        self.nObs += 2 if pKF.mvuRight[idx] >= 0 else 1

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs

    def EraseObservation(self, pKF, how=1):
        bBad = False
        if pKF in self.mObservations:
            idx = self.mObservations[pKF]
            self.nObs -= 2 if pKF.mvuRight[idx] >= 0 else 1
            del self.mObservations[pKF]
            self.world.dead[pKF.entry[idx]] = how
            if self.mpRefKF is pKF:
                self.mpRefKF = next(iter(self.mObservations), None)      # begin()->first; None where the reference reads end()
            if self.nObs <= self.bad_at:
                bBad = True
        if bBad:
            self.SetBadFlag()

    def SetBadFlag(self):
        self.mbBad = True
        obs, self.mObservations = self.mObservations, {}
        for pKF, idx in obs.items():
            pKF.EraseMapPointMatch(idx)
            self.world.dead[pKF.entry[idx]] = 2
        self.world.went_bad.append(self)


class World:
    """The objects of a problem.  status != OK: a refusal, nothing was built."""

    def __init__(self, q, bad_at=2):
        self.q = q
        off, kf = np.asarray(q["off"]), np.asarray(q["kf"])
        self.P, self.E, self.n_kf = len(off) - 1, int(off[-1]), int(q["n_kf"])
        self.input_bad = np.zeros(self.P, bool) if q.get("point_bad") is None else np.asarray(q["point_bad"]).astype(bool)
        self.dead = np.zeros(self.E, np.uint8)
        self.went_bad = []
        live = np.repeat(~self.input_bad, np.diff(off))
        self.status = NOT_RESIDENT if (kf[live] == -2).any() else BAD_INDEX if ((kf[live] < -2) | (kf[live] >= self.n_kf)).any() else OK
        if self.status != OK:
            return
        self.kfs = {c: KeyFrame(c) for c in list(range(self.n_kf)) + [CUR]}
        self.points, self.where = [], {}
        for p in range(self.P):
            pMP = MapPoint(self, bad_at)
            self.points.append(pMP)
            if self.input_bad[p]:
                pMP.mbBad = True
                continue
            for e in range(off[p], off[p + 1]):
                pKF = self.kfs[int(kf[e])]
                idx = pKF.add_keypoint(pMP, q["octave"][e], q["stereo"][e], q["depth"][e], e)
                pMP.AddObservation(pKF, idx)
                self.where[e] = (pKF, idx)
                if e - off[p] == q["ref_obs"][p]:
                    pMP.mpRefKF = pKF

    def weights(self):
        return np.where(np.asarray(self.q["stereo"]).astype(bool), 2, 1)

    def position_of_ref(self, p, among=None):
        """mpRefKF of point p as a position in its uploaded list (among None) or among the surviving entries"""
        off, pMP = self.q["off"], self.points[p]
        if self.input_bad[p]:
            return int(self.q["ref_obs"][p])
        es = [e for e in range(off[p], off[p + 1]) if among is None or among[e]]
        for j, e in enumerate(es):
            if self.where[e][0] is pMP.mpRefKF:
                return j
        return -1


def cull(q, cand_kf, cand_flags, monocular, th_depth, th_obs=3, ratio=0.9, oct_slack=1, bad_at=2):
    """KeyFrameCulling over the candidates in order.  dict(verdict, counts2, obs_dead, point_bad, ref_obs, n_obs, info8), all
    integers; on a refusal only info8 is meaningful (the others are zeros, as the caller's buffers were)."""
    w = World(q, bad_at)
    C = len(cand_kf)
    out = dict(verdict=np.zeros(C, np.uint8), counts2=np.zeros((C, 2), np.int32), obs_dead=np.zeros(w.E, np.uint8),
               point_bad=np.zeros(w.P, np.uint8), ref_obs=np.zeros(w.P, np.int32), n_obs=np.zeros(w.P, np.int32),
               info8=np.zeros(8, np.int32))
    if w.status != OK:
        out["info8"][0] = w.status
        return out
    th_depth = np.float32(th_depth)
    for c, (f, fl) in enumerate(zip(cand_kf, cand_flags)):
        pKF = w.kfs[int(f)]
        pKF.mnId, pKF.mbNotErase = (0 if fl & 1 else 1), bool(fl & 2)
        if pKF.mnId == 0:
            out["verdict"][c] = SKIPPED_ID0
            continue
        vpMapPoints = list(pKF.mvpMapPoints)
        thObs = th_obs
        nRedundantObservations = nMPs = 0
        for i, pMP in enumerate(vpMapPoints):
            if pMP is not None:
                if not pMP.isBad():
                    if not monocular:
                        if pKF.mvDepth[i] > th_depth or pKF.mvDepth[i] < 0:
                            continue
                    nMPs += 1
                    if pMP.Observations() > thObs:
                        scaleLevel = pKF.octave[i]
                        nObs = 0
                        for pKFi, idx in pMP.mObservations.items():
                            if pKFi is pKF:
                                continue
                            if pKFi.octave[idx] <= scaleLevel + oct_slack:
                                nObs += 1
                                if nObs >= thObs:
                                    break
                        if nObs >= thObs:
                            nRedundantObservations += 1
        out["counts2"][c] = (nRedundantObservations, nMPs)
        if float(nRedundantObservations) > ratio * float(nMPs):
            pKF.SetBadFlag()
            out["verdict"][c] = TO_BE_ERASED if pKF.mbToBeErased else CULLED
        else:
            out["verdict"][c] = KEPT
    wt = w.weights()
    for p, pMP in enumerate(w.points):
        out["ref_obs"][p] = w.position_of_ref(p)
        out["n_obs"][p] = wt[q["off"][p]:q["off"][p + 1]].sum() if w.input_bad[p] else pMP.nObs
        out["point_bad"][p] = pMP.mbBad and not w.input_bad[p]
    out["obs_dead"] = w.dead
    out["info8"][:5] = (OK, (out["verdict"] == CULLED).sum(), (out["verdict"] == TO_BE_ERASED).sum(), (w.dead != 0).sum(), len(w.went_bad))
    return out


def erase(q, obs_erase, bad_at=2):
    """EraseMapPointMatch + EraseObservation on every flagged entry, in entry order (any order gives the same: nObs only falls),
    then the lists compacted in the caller's order.  dict(obs_off, obs_map, point_bad, ref_obs, n_obs, info8); q needs off, kf,
    stereo, ref_obs, point_bad, n_kf (octave and depth are not read)."""
    q = dict(q)
    q.setdefault("octave", np.zeros(len(q["kf"]), np.int32))
    q.setdefault("depth", np.zeros(len(q["kf"]), np.float32))
    w = World(q, bad_at)
    assert w.status == OK
    off = np.asarray(q["off"])
    for e in np.flatnonzero(obs_erase):
        if e in w.where:                                  # (an entry of a bad point is nobody's)
            pKF, idx = w.where[e]
            pMP = pKF.mvpMapPoints[idx]
            if pMP is not None:
                pKF.EraseMapPointMatch(idx)
                pMP.EraseObservation(pKF, how=1)
    alive = w.dead == 0
    new_off = np.concatenate([[0], np.cumsum([alive[off[p]:off[p + 1]].sum() for p in range(w.P)])]).astype(np.int32)
    obs_map = np.where(alive, np.cumsum(alive) - 1, -1).astype(np.int32)
    out = dict(obs_off=new_off, obs_map=obs_map, point_bad=np.zeros(w.P, np.uint8), ref_obs=np.zeros(w.P, np.int32),
               n_obs=np.zeros(w.P, np.int32), info8=np.zeros(8, np.int32))
    wt = w.weights()
    for p, pMP in enumerate(w.points):
        out["point_bad"][p] = pMP.mbBad
        out["ref_obs"][p] = max(w.position_of_ref(p, among=alive), 0) if new_off[p + 1] > new_off[p] else 0
        out["n_obs"][p] = wt[off[p]:off[p + 1]].sum() if w.input_bad[p] else (0 if pMP.mbBad else pMP.nObs)
    out["info8"][:4] = (0, (~alive).sum(), len(w.went_bad), alive.sum())
    return out


def apply_erase(obs, ref_obs, point_bad, er):
    """The caller's mirror: per-point lists (any tuples), ref_obs and point_bad after the erasure `er` (erase()'s or the getter's dict)"""
    flat = [t for o in obs for t in o]
    keep = [t for t, m in zip(flat, er["obs_map"]) if m >= 0]
    new = [keep[er["obs_off"][p]:er["obs_off"][p + 1]] for p in range(len(obs))]
    return new, er["ref_obs"].copy(), er["point_bad"].copy()


def problem(points, n_kf, ref_obs=None, point_bad=None, kf_bad=None):
    """points: per point a list of (kf, octave, stereo, depth) -> the problem dict"""
    flat = [t for o in points for t in o]
    off = np.concatenate([[0], np.cumsum([len(o) for o in points])]).astype(np.int32)
    P = len(points)
    return dict(off=off, kf=np.array([t[0] for t in flat], np.int32), octave=np.array([t[1] for t in flat], np.int32),
                stereo=np.array([t[2] for t in flat], np.uint8), depth=np.array([t[3] for t in flat], np.float32),
                ref_obs=np.zeros(P, np.int32) if ref_obs is None else np.asarray(ref_obs, np.int32),
                point_bad=None if point_bad is None else np.asarray(point_bad, np.uint8), n_kf=n_kf,
                kf_bad=np.zeros(len(flat), np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8))


FIELDS = ("verdict", "counts2", "obs_dead", "point_bad", "ref_obs", "n_obs", "info8")
ERASE_FIELDS = ("obs_off", "obs_map", "point_bad", "ref_obs", "n_obs", "info8")


def differing(got, want, fields=FIELDS):
    """The fields in which two results differ (exactly: they are all integers); after a refusal only info8 counts"""
    if want["info8"][0] != OK:
        return [] if np.array_equal(got["info8"], want["info8"]) else ["info8"]
    return [k for k in fields if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]))]
