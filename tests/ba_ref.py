"""Optimizer::LocalBundleAdjustment restated in numpy float64 (reference src/Optimizer.cc:417-714), with the parts of g2o it runs:

    OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale   core/optimization_algorithm_levenberg.cpp:61-189
    BlockSolver::buildSystem / setLambda (Hpp AND Hll) / solve (Schur) / restoreDiagonal   core/block_solver.hpp
    SparseOptimizer::initializeOptimization(level): a vertex without an edge of the level is not active
    BaseBinaryEdge::constructQuadraticForm, robustInformation = rho[1] * information, RobustKernelHuber
    EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (computeError, linearizeOplus, isDepthPositive), SE3Quat, VertexSE3Expmap::oplus

A problem is a dict of host arrays, the inputs of sd_debug_local_ba:
    off [P + 1] CSR offsets; kf [E] camera of every observation (-2: not resident, any other value outside [0, n_kf): a bad index);
    uv [E, 2], ur [E], inv_sigma2 [E] float32; kf_bad [E], point_bad [P] uint8; poses [n_kf, 4, 4] Tcw; roles [n_kf] (1 local,
    2 local and fixed, 0 fixed if observed); Xw [P, 3]; cam (fx, fy, cx, cy) and bf, float32 values.
Quirks kept: lambda re-initialised at iteration 0 of each optimize(); Terminate on rho == 0, ten trials or _nBad >= 3; chi2() in
the two classification loops is the error of the LAST computeActiveErrors (after a rejected last trial that of the rejected step;
for a level-1 edge in round 2, round 1's last value) while isDepthPositive() is taken at the estimate.
A zero pivot in the reduced system's LDL^T (the only way Eigen's SimplicialLDLT reports failure) fails the trial with x = 0.

levenberg() is the one Levenberg driver: run() calls it twice (5 robust iterations, classify(), 10 plain ones on level 0, classify()),
tests/gba_ref.py (Optimizer::BundleAdjustment) once on every edge.  Its solvers of the reduced system, ldlt_solve and
blocked_ldlt_solve (the order the device takes for more than MAX_FREE_KF free cameras), are at the end of the file.
"""
import numpy as np

SD_BA_OK, SD_BA_NOT_RESIDENT, SD_BA_TOO_MANY_KF, SD_BA_BAD_INDEX = 0, 1, 2, 3
POINT_OPTIMISED, POINT_SKIPPED, POINT_BAD_INDEX = 1, 0, 2
MAX_FREE_KF = 32
EXIT_NOT_RUN, EXIT_NBAD, EXIT_QMAX, EXIT_RHO_ZERO, EXIT_ITERATIONS = 0, 1, 2, 3, 4
DELTA_MONO, DELTA_STEREO = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))
CHI2_MONO, CHI2_STEREO = 5.991, 7.815


# ---- SE3Quat: q = (x, y, z, w), t ----
def q_normalize(q):
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def q_from_R(m):
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3], q[j], q[k] = (m[k, j] - m[j, k]) * t, (m[j, i] + m[i, j]) * t, (m[k, i] + m[i, k]) * t
    return q


def q_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def q_to_R(q):
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def q_rotate(q, v):
    """Eigen's quaternion * vector on [..., 3] arrays of v"""
    u = q[:3]
    uv = 2 * np.cross(u, v)
    return v + q[3] * uv + np.cross(u, uv)


def se3_from_T(T):
    return q_normalize(q_from_R(T[:3, :3])), T[:3, 3].copy()


def se3_to_T(q, t):
    T = np.eye(4)
    T[:3, :3] = q_to_R(q)
    T[:3, 3] = t
    return T


def se3_exp(u):
    om, up = u[:3], u[3:]
    th = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    Om2 = Om @ Om
    if th < 0.00001:
        R = V = (np.eye(3) + Om) + Om2
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / th ** 3
        R = (np.eye(3) + a * Om) + b * Om2
        V = (np.eye(3) + b * Om) + c * Om2
    return q_normalize(q_from_R(R)), V @ up


def se3_mul(qa, ta, qb, tb):
    return q_normalize(q_mul(qa, qb)), ta + q_rotate(qa, tb)


# ---- the edges, vectorised over an index set ----
def map_points(Q, T, X, cam, pt):
    """estimate().map(Xw) of edges (cam[i], pt[i]): [n, 3]"""
    q, v = Q[cam], X[pt]
    u = q[:, :3]
    uv = 2 * np.cross(u, v)
    return v + q[:, 3:4] * uv + np.cross(u, uv) + T[cam]


def edge_errors(pc, stereo, meas, K):
    fx, fy, cx, cy, bf = K
    err = np.zeros((len(pc), 3))
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        invz = np.where(stereo, (1.0 / z).astype(np.float32).astype(np.float64), 1.0)          # const float invz = 1.0f / z
        px = np.where(stereo, pc[:, 0] * invz, pc[:, 0] / z)
        py = np.where(stereo, pc[:, 1] * invz, pc[:, 1] / z)
        r0, r1 = px * fx + cx, py * fy + cy
        err[:, 0] = meas[:, 0] - r0
        err[:, 1] = meas[:, 1] - r1
        err[:, 2] = np.where(stereo, meas[:, 2] - (r0 - bf * invz), 0.0)
    return err


def edge_jacobians(pc, R, stereo, K):
    """(Jl [n, 3, 3] = _jacobianOplusXi, Jp [n, 3, 6] = _jacobianOplusXj); row 2 is zero for a mono edge"""
    fx, fy, cx, cy, bf = K
    n = len(pc)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    z2 = z * z
    Jp = np.zeros((n, 3, 6))
    Jp[:, 0, 0] = x * y / z2 * fx
    Jp[:, 0, 1] = -(1 + (x * x / z2)) * fx
    Jp[:, 0, 2] = y / z * fx
    Jp[:, 0, 3] = -1. / z * fx
    Jp[:, 0, 5] = x / z2 * fx
    Jp[:, 1, 0] = (1 + y * y / z2) * fy
    Jp[:, 1, 1] = -x * y / z2 * fy
    Jp[:, 1, 2] = -x / z * fy
    Jp[:, 1, 4] = -1. / z * fy
    Jp[:, 1, 5] = y / z2 * fy
    Jl = np.zeros((n, 3, 3))
    a, t02, t12 = -1. / z, -x / z * fx, -y / z * fy             # EdgeSE3ProjectXYZ: -1. / z * tmp * R
    for c in range(3):
        Jl[:, 0, c] = np.where(stereo, -fx * R[:, 0, c] / z + fx * x * R[:, 2, c] / z2, (a * fx) * R[:, 0, c] + (a * t02) * R[:, 2, c])
        Jl[:, 1, c] = np.where(stereo, -fy * R[:, 1, c] / z + fy * y * R[:, 2, c] / z2, (a * fy) * R[:, 1, c] + (a * t12) * R[:, 2, c])
        Jl[:, 2, c] = np.where(stereo, Jl[:, 0, c] - bf * R[:, 2, c] / z2, 0.0)
    s = stereo
    Jp[:, 2, 0] = np.where(s, Jp[:, 0, 0] - bf * y / z2, 0.0)
    Jp[:, 2, 1] = np.where(s, Jp[:, 0, 1] + bf * x / z2, 0.0)
    Jp[:, 2, 2] = np.where(s, Jp[:, 0, 2], 0.0)
    Jp[:, 2, 3] = np.where(s, Jp[:, 0, 3], 0.0)
    Jp[:, 2, 5] = np.where(s, Jp[:, 0, 5] - bf / z2, 0.0)
    return Jl, Jp


def huber(e2, delta):
    """rho[0], rho[1] of RobustKernelHuber::robustify"""
    d2 = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e2)
        inl = e2 <= d2
        return np.where(inl, e2, 2 * sq * delta - d2), np.where(inl, 1.0, delta / sq)


class _State:
    pass


def _setup(p):
    s = _State()
    off = np.asarray(p["off"], np.int64)
    P, E = len(off) - 1, int(off[-1])
    kf = np.asarray(p["kf"], np.int64)
    n_kf = len(p["roles"])
    roles = np.asarray(p["roles"], np.uint8)
    kf_bad = np.zeros(E, bool) if p.get("kf_bad") is None else np.asarray(p["kf_bad"]).astype(bool)
    pbad = np.zeros(P, bool) if p.get("point_bad") is None else np.asarray(p["point_bad"]).astype(bool)
    pt = np.repeat(np.arange(P), np.diff(off))
    live = ~kf_bad & ~pbad[pt]                       # observations that would give an edge
    s.P, s.E, s.n_kf, s.off, s.kf, s.pt, s.roles, s.live = P, E, n_kf, off, kf, pt, roles, live
    not_res = live & (kf == -2)
    bad_idx = live & ~not_res & ((kf < 0) | (kf >= n_kf))
    s.point_status = np.zeros(P, np.uint8)
    s.point_status[np.unique(pt[bad_idx])] = POINT_BAD_INDEX
    s.n_free = int((roles == 1).sum())
    s.status = SD_BA_NOT_RESIDENT if not_res.any() else SD_BA_BAD_INDEX if bad_idx.any() else \
        SD_BA_TOO_MANY_KF if s.n_free > MAX_FREE_KF else SD_BA_OK
    return s


def _load(p, s):
    """The graph of an accepted problem on s: the edges' data, full length and indexed by observation (cam, pt of _setup, stereo, meas,
    info, and err = the error of the last computeActiveErrors), the free cameras' slots and the estimate (Q, Tt, X)."""
    s.K = tuple(float(np.float32(v)) for v in p["cam"]) + (float(np.float32(p["bf"])),)
    s.cam = np.where(s.live, s.kf, 0)
    uv, ur = np.asarray(p["uv"], np.float32), np.asarray(p["ur"], np.float32)
    s.stereo = ~(ur < 0)
    s.meas = np.stack([uv[:, 0], uv[:, 1], np.where(s.stereo, ur, 0)], 1).astype(np.float64)
    s.info = np.asarray(p["inv_sigma2"], np.float32).astype(np.float64)
    s.err = np.zeros((s.E, 3))
    s.free = s.roles == 1
    free_ids = np.flatnonzero(s.free)
    s.slot = -np.ones(s.n_kf, np.int64)
    s.slot[free_ids] = np.arange(len(free_ids))
    s.Kf = len(free_ids)
    T_in = np.asarray(p["poses"], np.float64)
    s.Q, s.Tt = np.zeros((s.n_kf, 4)), np.zeros((s.n_kf, 3))
    for c in range(s.n_kf):
        s.Q[c], s.Tt[c] = se3_from_T(T_in[c])
    s.X = np.asarray(p["Xw"], np.float64).copy()


def _chi2_of(s, idx):
    return (s.err[idx] * (s.info[idx, None] * s.err[idx])).sum(1)


def levenberg(s, act, iterations, robust, delta, solver, trace):
    """One optimize(iterations) of OptimizationAlgorithmLevenberg on the edges `act` (indices into the observations) of the graph that
    _load put on s; delta [E] is each edge's Huber width, read if robust.  solver: "schur" (ldlt_solve on the reduced system), "blocked"
    (blocked_ldlt_solve on it) or "dense" (np.linalg.solve on the whole system).  Appends one dict(chi2, lambda0, trials=[dict(lam,
    rho, accept, temp_chi, scale)]) per iteration to trace, leaves s.Q, s.Tt, s.X and s.err[act] updated and returns (iterations done,
    trials, exit taken)."""
    P, Kf, slot, K = s.P, s.Kf, s.slot, s.K
    a_pt = np.zeros(P, bool)
    a_pt[s.pt[act]] = True
    a_kf = np.zeros(s.n_kf, bool)
    a_kf[s.cam[act]] = True
    a_kf &= s.free
    if not (a_pt.any() or a_kf.any()):
        return 0, 0, EXIT_NOT_RUN
    e_cam, e_pt, e_st = s.cam[act], s.pt[act], s.stereo[act]
    e_slot = slot[e_cam]
    fe = np.flatnonzero(a_kf[e_cam])                    # the edges of a free camera
    a_slots = slot[np.flatnonzero(a_kf)]
    info, meas, delta = s.info[act], s.meas[act], delta[act]

    def active_errors():
        s.err[act] = edge_errors(map_points(s.Q, s.Tt, s.X, e_cam, e_pt), e_st, meas, K)
        c2 = _chi2_of(s, act)
        return float((huber(c2, delta)[0] if robust else c2).sum())

    lam, ni, n_bad, done, trials, exit_taken = -1.0, 2.0, 0, 0, 0, EXIT_NOT_RUN
    for it in range(iterations):
        cur_chi = active_errors()
        ini_chi = cur_chi
        pc = map_points(s.Q, s.Tt, s.X, e_cam, e_pt)
        Rall = np.stack([q_to_R(s.Q[c]) for c in range(s.n_kf)])
        Jl, Jp = edge_jacobians(pc, Rall[e_cam], e_st, K)
        c2 = _chi2_of(s, act)
        rho1 = huber(c2, delta)[1] if robust else np.ones(len(act))
        w = rho1 * info
        wr = -(info * rho1)[:, None] * s.err[act]                         # omega_r = -omega * error * rho[1]
        Hll, bl = np.zeros((P, 3, 3)), np.zeros((P, 3))
        np.add.at(Hll, e_pt, np.einsum("nda,n,ndb->nab", Jl, w, Jl))
        np.add.at(bl, e_pt, np.einsum("nda,nd->na", Jl, wr))
        Hpp, bp = np.zeros((Kf, 6, 6)), np.zeros((Kf, 6))
        np.add.at(Hpp, e_slot[fe], np.einsum("nda,n,ndb->nab", Jp[fe], w[fe], Jp[fe]))
        np.add.at(bp, e_slot[fe], np.einsum("nda,nd->na", Jp[fe], wr[fe]))
        Hpl = np.einsum("nda,n,ndb->nab", Jp, w, Jl)                      # [n, 6, 3], used where fe
        if it == 0:
            diag = [np.abs(np.diagonal(Hll[a_pt], axis1=1, axis2=2)).ravel(), np.abs(np.diagonal(Hpp[a_slots], axis1=1, axis2=2)).ravel()]
            lam, ni, n_bad = 1e-5 * float(np.concatenate(diag + [np.zeros(1)]).max()), 2.0, 0
        it_rec = dict(chi2=cur_chi, lambda0=lam, trials=[])
        trace.append(it_rec)
        rho, qmax = 0.0, 0
        while True:
            backup = (s.Q.copy(), s.Tt.copy(), s.X.copy())
            xp, xl, ok = np.zeros((Kf, 6)), np.zeros((P, 3)), True
            if solver in REDUCED_SOLVERS:
                Dinv = np.zeros((P, 3, 3))
                Dinv[a_pt] = np.linalg.inv(Hll[a_pt] + lam * np.eye(3))
                db = np.einsum("pab,pb->pa", Dinv, bl)
                S = np.zeros((Kf, 6, Kf, 6))
                for k in a_slots:
                    S[k, :, k, :] = Hpp[k] + lam * np.eye(6)
                bs = bp.copy()
                np.subtract.at(bs, e_slot[fe], np.einsum("nab,nb->na", Hpl[fe], db[e_pt[fe]]))
                order = np.argsort(e_pt[fe], kind="stable")
                fes = fe[order]
                for grp in np.split(fes, np.flatnonzero(np.diff(e_pt[fes])) + 1):
                    if len(grp) == 0:
                        continue
                    D = Dinv[e_pt[grp[0]]]
                    for a in grp:
                        BD = Hpl[a] @ D
                        for b in grp:
                            S[e_slot[a], :, e_slot[b], :] -= BD @ Hpl[b].T
                idx = (a_slots[:, None] * 6 + np.arange(6)).ravel()
                if len(idx):
                    ok, sol = REDUCED_SOLVERS[solver](S.reshape(Kf * 6, Kf * 6)[np.ix_(idx, idx)], bs.reshape(-1)[idx])
                    if ok:
                        xp.reshape(-1)[idx] = sol
                if ok:
                    cl = bl.copy()
                    np.subtract.at(cl, e_pt[fe], np.einsum("nab,na->nb", Hpl[fe], xp[e_slot[fe]]))
                    xl[a_pt] = np.einsum("pab,pb->pa", Dinv, cl)[a_pt]
                else:
                    xp[:] = 0
            else:                                    # the same system, solved densely at once
                assert solver == "dense"
                pi = np.flatnonzero(a_pt)
                n = 6 * len(a_slots) + 3 * len(pi)
                col_k = -np.ones(Kf, np.int64)
                col_k[a_slots] = np.arange(len(a_slots)) * 6
                col_p = -np.ones(P, np.int64)
                col_p[pi] = 6 * len(a_slots) + np.arange(len(pi)) * 3
                H, b = np.zeros((n, n)), np.zeros(n)
                for k in a_slots:
                    H[col_k[k]:col_k[k] + 6, col_k[k]:col_k[k] + 6] = Hpp[k]
                    b[col_k[k]:col_k[k] + 6] = bp[k]
                for q in pi:
                    H[col_p[q]:col_p[q] + 3, col_p[q]:col_p[q] + 3] = Hll[q]
                    b[col_p[q]:col_p[q] + 3] = bl[q]
                for a in fe:
                    r, c = col_k[e_slot[a]], col_p[e_pt[a]]
                    H[r:r + 6, c:c + 3] += Hpl[a]
                    H[c:c + 3, r:r + 6] += Hpl[a].T
                H[np.arange(n), np.arange(n)] += lam
                sol = np.linalg.solve(H, b)
                for k in a_slots:
                    xp[k] = sol[col_k[k]:col_k[k] + 6]
                for q in pi:
                    xl[q] = sol[col_p[q]:col_p[q] + 3]
            for c in np.flatnonzero(a_kf):
                s.Q[c], s.Tt[c] = se3_mul(*se3_exp(xp[slot[c]]), s.Q[c], s.Tt[c])
            s.X[a_pt] = s.X[a_pt] + xl[a_pt]
            temp_chi = active_errors()
            if not ok:
                temp_chi = np.finfo(np.float64).max
            rho = cur_chi - temp_chi
            scale = 0.0
            for k in a_slots:
                scale += float((xp[k] * (lam * xp[k] + bp[k])).sum())
            scale += float((xl[a_pt] * (lam * xl[a_pt] + bl[a_pt])).sum())
            rho /= scale + 1e-3
            accept = bool(rho > 0 and np.isfinite(temp_chi))
            it_rec["trials"].append(dict(lam=lam, rho=rho, accept=accept, temp_chi=temp_chi, scale=scale))
            if accept:
                alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                cur_chi = temp_chi
            else:
                lam *= ni
                ni *= 2
                s.Q, s.Tt, s.X = backup
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        done += 1
        exit_taken = EXIT_ITERATIONS
        if qmax == 10 or rho == 0:
            exit_taken = EXIT_QMAX if qmax == 10 else EXIT_RHO_ZERO
            break
        n_bad = n_bad + 1 if (ini_chi - cur_chi) * 1e3 < ini_chi else 0
        if n_bad >= 3:
            exit_taken = EXIT_NBAD
            break
    return done, trials, exit_taken


def run(p, solver="schur"):
    """The whole call.  Returns dict(status, T [n_kf, 4, 4], Xw, point_status, obs_erase, info16, trace); trace[r] is the trace of
    levenberg() in round r."""
    s = _setup(p)
    out = dict(status=s.status, T=np.array(p["poses"], np.float64), Xw=np.array(p["Xw"], np.float64), point_status=s.point_status,
               obs_erase=np.zeros(s.E, np.uint8), info16=np.zeros(16, np.int32), trace=[[], []])
    info16 = out["info16"]
    info16[0] = s.status
    if s.status != SD_BA_OK:
        return out
    _load(p, s)
    E, edge, stereo, cam, pt = s.E, s.live.copy(), s.stereo, s.cam, s.pt
    delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
    has_edge_pt = np.zeros(s.P, bool)
    has_edge_pt[pt[edge]] = True
    s.point_status[has_edge_pt] = POINT_OPTIMISED
    has_edge_kf = np.zeros(s.n_kf, bool)
    has_edge_kf[cam[edge]] = True
    n_fixed = int(((s.roles == 2) | ((s.roles == 0) & has_edge_kf)).sum())
    level = np.zeros(E, np.int8)
    info16[1:6] = [s.Kf, n_fixed, int(has_edge_pt.sum()), int((edge & ~stereo).sum()), int((edge & stereo).sum())]

    def optimize(iterations, robust, trace):
        return levenberg(s, np.flatnonzero(edge & (level == 0)), iterations, robust, delta, solver, trace)

    def classify():
        """(the edges the test puts aside, the chi2 and the depth it read) -- chi2 from `err` as it stands, depth at the estimate"""
        idx = np.flatnonzero(edge)
        chi2, z = np.zeros(E), np.ones(E)
        chi2[idx] = _chi2_of(s, idx)
        z[idx] = map_points(s.Q, s.Tt, s.X, cam[idx], pt[idx])[:, 2]
        return edge & ((chi2 > np.where(stereo, CHI2_STEREO, CHI2_MONO)) | ~(z > 0.0)), chi2, z

    info16[6:9] = optimize(5, True, out["trace"][0])
    bad, out["chi2_r1"], out["depth_r1"] = classify()
    level[bad] = 1
    info16[12] = int(bad.sum())
    info16[9:12] = optimize(10, False, out["trace"][1])
    erase, out["chi2"], out["depth"] = classify()
    out["obs_erase"][erase] = 1
    out["level1"] = (level == 1).astype(np.uint8)
    out["stereo"], out["edge"] = stereo, edge
    info16[13] = int(erase.sum())
    for c in np.flatnonzero(s.free & has_edge_kf):
        out["T"][c] = se3_to_T(s.Q[c], s.Tt[c])
    out["Xw"][has_edge_pt] = s.X[has_edge_pt]
    return out


def ldlt_solve(A, b):
    """LDL^T without pivoting in index order; (False, None) on a zero pivot"""
    n = len(b)
    L, d = np.eye(n), np.zeros(n)
    A = A.copy()
    for k in range(n):
        d[k] = A[k, k]
        if d[k] == 0:
            return False, None
        L[k + 1:, k] = A[k + 1:, k] / d[k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], A[k + 1:, k])
    y = np.linalg.solve(L, b) if n else b
    return True, np.linalg.solve(L.T, y / d)


PANEL = 48


def blocked_ldlt_solve(A, b, panel=PANEL):
    """LDL^T without pivoting in index order, in panels: (ok, x); (False, None) on a zero pivot.  The factorisation the device runs
    for more than MAX_FREE_KF free cameras (sdslam_amd/csrc/track_ba.hip, k_gba_*): the same sums as ldlt_solve taken panel by panel,
    and the right-hand side carried as one more row of the triangle."""
    n = len(b)
    M = np.zeros((n + 1, n))
    M[:n] = np.tril(A)
    M[n] = b                                           # the right-hand side rides along as row n
    d = np.zeros(n)
    for c0 in range(0, n, panel):
        c1 = min(n, c0 + panel)
        w = c1 - c0
        W = np.zeros((n + 1, w))                       # L D of the panel's columns
        for k in range(w):                             # the diagonal block
            d[c0 + k] = M[c0 + k, c0 + k]
            if d[c0 + k] == 0:
                return False, None
            col = M[c0 + k + 1:c1, c0 + k].copy()
            W[c0 + k + 1:c1, k] = col
            l = col / d[c0 + k]
            M[c0 + k + 1:c1, c0 + k] = l
            M[c0 + k + 1:c1, c0 + k + 1:c1] -= np.tril(np.outer(l, col))
        for j in range(w):                             # the rows below it
            v = M[c1:, c0 + j].copy()
            for k in range(j):
                v -= M[c1:, c0 + k] * W[c0 + j, k]
            W[c1:, j] = v
            M[c1:, c0 + j] = v / d[c0 + j]
        for k in range(w):                             # the trailing triangle (row n has no entry right of column n - 1)
            M[c1:, c1:] -= np.outer(M[c1:, c0 + k], W[c1:n, k])
    x = M[n].copy()                                    # y = D^-1 L^-1 b
    for k in range(n - 1, 0, -1):
        x[:k] -= M[k, :k] * x[k]
    return True, x


REDUCED_SOLVERS = dict(schur=ldlt_solve, blocked=blocked_ldlt_solve)     # levenberg()'s solvers of the reduced (Schur) system
