"""Optimizer::BundleAdjustment / GlobalBundleAdjustemnt restated in numpy float64 (reference src/Optimizer.cc:46-219), on the parts of
g2o that tests/ba_ref.py restates for LocalBundleAdjustment: the graph, the Levenberg driver (ba_ref.levenberg) and its solvers are
that file's, run here ONCE as optimize(nIterations) on level 0 = every edge.  This file holds what differs: the constants, the
SD_BA_NO_VERTEX refusal and the packing of the outputs.

A problem is the dict of ba_ref (the inputs of sd_debug_global_ba); the roles are read as 1 = a free vertex, 2 = a fixed vertex
(mnId == 0, :81), 0 = not a keyframe of vpKFs: a live observation of such a camera refuses the call (SD_BA_NO_VERTEX).
Differences from the local run: thHuber2D = sqrt(5.99) (sic, :87) against sqrt(5.991); robust or not by bRobust; no classification;
a point that is bad or has no edge is vbNotIncludedMP and keeps its position."""
import numpy as np

import ba_ref
from ba_ref import SD_BA_OK, SD_BA_TOO_MANY_KF, POINT_OPTIMISED, se3_to_T
from ba_ref import PANEL, blocked_ldlt_solve           # the factorisation of more than LDS_FREE_KF free cameras: the tests read them here

SD_BA_NO_VERTEX = 4
MAX_FREE_KF, MAX_ITERATIONS = 256, 20
LDS_FREE_KF = ba_ref.MAX_FREE_KF                       # up to here the device factorises in LDS (k_ba_solve)
DELTA_MONO = float(np.float32(np.sqrt(5.99)))          # thHuber2D, :87
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))       # thHuber3D, :88


def _setup(p):
    s = ba_ref._setup(p)
    live_ok = s.live & (s.kf >= 0) & (s.kf < s.n_kf)
    no_vertex = live_ok & (s.roles[np.clip(s.kf, 0, s.n_kf - 1)] == 0)
    if s.status in (SD_BA_OK, SD_BA_TOO_MANY_KF):     # local BA's refusals in its order with this call's capacity, NO_VERTEX last
        s.status = SD_BA_TOO_MANY_KF if s.n_free > MAX_FREE_KF else SD_BA_NO_VERTEX if no_vertex.any() else SD_BA_OK
    return s


def run(p, n_iterations, robust, solver="schur", delta_mono=DELTA_MONO):
    """The whole call.  Returns dict(status, T [n_kf, 4, 4], Xw, point_status, info16, trace); trace is that of ba_ref.levenberg,
    which also names the solvers."""
    assert 1 <= n_iterations <= MAX_ITERATIONS and robust in (0, 1, False, True)
    s = _setup(p)
    out = dict(status=s.status, T=np.array(p["poses"], np.float64), Xw=np.array(p["Xw"], np.float64), point_status=s.point_status,
               info16=np.zeros(16, np.int32), trace=[])
    info16 = out["info16"]
    info16[0] = s.status
    if s.status != SD_BA_OK:
        return out
    ba_ref._load(p, s)
    act = np.flatnonzero(s.live)
    a_pt = np.zeros(s.P, bool)
    a_pt[s.pt[act]] = True
    a_kf = np.zeros(s.n_kf, bool)
    a_kf[s.cam[act]] = True
    a_kf &= s.free
    s.point_status[a_pt] = POINT_OPTIMISED
    info16[1:6] = [s.Kf, int((s.roles == 2).sum()), int(a_pt.sum()), int((~s.stereo[act]).sum()), int(s.stereo[act].sum())]
    delta = np.where(s.stereo, DELTA_STEREO, delta_mono)
    info16[6:9] = ba_ref.levenberg(s, act, n_iterations, robust, delta, solver, out["trace"])
    for c in np.flatnonzero(a_kf):
        out["T"][c] = se3_to_T(s.Q[c], s.Tt[c])
    out["Xw"][a_pt] = s.X[a_pt]
    return out
