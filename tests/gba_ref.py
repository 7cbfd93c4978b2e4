"""Optimizer::BundleAdjustment / GlobalBundleAdjustemnt restated in numpy float64 (reference src/Optimizer.cc:46-219), on the parts of
g2o that tests/ba_ref.py restates for LocalBundleAdjustment: the SE3, edge, Jacobian, Huber and ldlt_solve helpers are imported from
there, the Levenberg driver is written out again for ONE optimize(nIterations) on level 0 = every edge.

A problem is the dict of ba_ref (the inputs of sd_debug_global_ba); the roles are read as 1 = a free vertex, 2 = a fixed vertex
(mnId == 0, :81), 0 = not a keyframe of vpKFs: a live observation of such a camera refuses the call (SD_BA_NO_VERTEX).
Differences from the local run: thHuber2D = sqrt(5.99) (sic, :87) against sqrt(5.991); robust or not by bRobust; no classification;
a point that is bad or has no edge is vbNotIncludedMP and keeps its position.

blocked_ldlt_solve is the factorisation the device runs for more than 32 free cameras (sdslam_amd/csrc/track_ba.hip, k_gba_*): the
same sums as ba_ref.ldlt_solve taken panel by panel, and the right-hand side carried as one more row of the triangle."""
import numpy as np

import ba_ref
from ba_ref import (SD_BA_OK, SD_BA_NOT_RESIDENT, SD_BA_TOO_MANY_KF, SD_BA_BAD_INDEX, POINT_OPTIMISED, POINT_SKIPPED, POINT_BAD_INDEX,
                    EXIT_NOT_RUN, EXIT_NBAD, EXIT_QMAX, EXIT_RHO_ZERO, EXIT_ITERATIONS, se3_from_T, se3_to_T, se3_exp, se3_mul, q_to_R,
                    map_points, edge_errors, edge_jacobians, huber, ldlt_solve)

SD_BA_NO_VERTEX = 4
MAX_FREE_KF, MAX_ITERATIONS = 256, 20
LDS_FREE_KF = ba_ref.MAX_FREE_KF                       # up to here the device factorises in LDS (k_ba_solve)
PANEL = 48
DELTA_MONO = float(np.float32(np.sqrt(5.99)))          # thHuber2D, :87
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))       # thHuber3D, :88


def blocked_ldlt_solve(A, b, panel=PANEL):
    """LDL^T without pivoting in index order, in panels: (ok, x); (False, None) on a zero pivot"""
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


def _setup(p):
    s = ba_ref._setup(p)
    live_ok = s.live & (s.kf >= 0) & (s.kf < s.n_kf)
    no_vertex = live_ok & (s.roles[np.clip(s.kf, 0, s.n_kf - 1)] == 0)
    if s.status in (SD_BA_OK, SD_BA_TOO_MANY_KF):     # local BA's refusals in its order with this call's capacity, NO_VERTEX last
        s.status = SD_BA_TOO_MANY_KF if s.n_free > MAX_FREE_KF else SD_BA_NO_VERTEX if no_vertex.any() else SD_BA_OK
    return s


def run(p, n_iterations, robust, solver="schur", delta_mono=DELTA_MONO):
    """The whole call.  Returns dict(status, T [n_kf, 4, 4], Xw, point_status, info16, trace); trace is a list of iterations, each
    dict(chi2, lambda0, trials=[dict(lam, rho, accept, temp_chi, scale)]).  solver: "schur" (ldlt_solve on the reduced system),
    "blocked" (blocked_ldlt_solve on it) or "dense" (np.linalg.solve on the whole system)."""
    assert 1 <= n_iterations <= MAX_ITERATIONS and robust in (0, 1, False, True)
    s = _setup(p)
    T_in, X_in = np.asarray(p["poses"], np.float64), np.asarray(p["Xw"], np.float64)
    out = dict(status=s.status, T=T_in.copy(), Xw=X_in.copy(), point_status=s.point_status, info16=np.zeros(16, np.int32), trace=[])
    info16 = out["info16"]
    info16[0] = s.status
    if s.status != SD_BA_OK:
        return out
    K = tuple(float(np.float32(v)) for v in p["cam"]) + (float(np.float32(p["bf"])),)
    E, P, n_kf = s.E, s.P, s.n_kf
    act = np.flatnonzero(s.live)
    e_cam, e_pt = s.kf[act], s.pt[act]
    uv, ur = np.asarray(p["uv"], np.float32)[act], np.asarray(p["ur"], np.float32)[act]
    e_st = ~(ur < 0)
    meas = np.stack([uv[:, 0], uv[:, 1], np.where(e_st, ur, 0)], 1).astype(np.float64)
    info = np.asarray(p["inv_sigma2"], np.float32).astype(np.float64)[act]
    delta = np.where(e_st, DELTA_STEREO, delta_mono)
    a_pt = np.zeros(P, bool)
    a_pt[e_pt] = True
    has_kf = np.zeros(n_kf, bool)
    has_kf[e_cam] = True
    free = s.roles == 1
    a_kf = has_kf & free
    s.point_status[a_pt] = POINT_OPTIMISED
    free_ids = np.flatnonzero(free)
    slot = -np.ones(n_kf, np.int64)
    slot[free_ids] = np.arange(len(free_ids))
    Kf = len(free_ids)
    info16[1:6] = [Kf, int((s.roles == 2).sum()), int(a_pt.sum()), int((~e_st).sum()), int(e_st.sum())]
    Q, Tt = np.zeros((n_kf, 4)), np.zeros((n_kf, 3))
    for c in range(n_kf):
        Q[c], Tt[c] = se3_from_T(T_in[c])
    X = X_in.copy()
    if len(act) == 0:
        return out
    e_slot, e_free = slot[e_cam], a_kf[e_cam]
    fe = np.flatnonzero(e_free)
    a_slots = slot[np.flatnonzero(a_kf)]
    err = np.zeros((len(act), 3))

    def active_errors():
        err[:] = edge_errors(map_points(Q, Tt, X, e_cam, e_pt), e_st, meas, K)
        c2 = (err * (info[:, None] * err)).sum(1)
        return float((huber(c2, delta)[0] if robust else c2).sum())

    lam, ni, n_bad, done, trials, exit_taken = -1.0, 2.0, 0, 0, 0, EXIT_NOT_RUN
    for it in range(n_iterations):
        cur_chi = active_errors()
        ini_chi = cur_chi
        pc = map_points(Q, Tt, X, e_cam, e_pt)
        Rall = np.stack([q_to_R(Q[c]) for c in range(n_kf)])
        Jl, Jp = edge_jacobians(pc, Rall[e_cam], e_st, K)
        c2 = (err * (info[:, None] * err)).sum(1)
        rho1 = huber(c2, delta)[1] if robust else np.ones(len(act))
        w = rho1 * info
        wr = -(info * rho1)[:, None] * err
        Hll, bl = np.zeros((P, 3, 3)), np.zeros((P, 3))
        np.add.at(Hll, e_pt, np.einsum("nda,n,ndb->nab", Jl, w, Jl))
        np.add.at(bl, e_pt, np.einsum("nda,nd->na", Jl, wr))
        Hpp, bp = np.zeros((Kf, 6, 6)), np.zeros((Kf, 6))
        np.add.at(Hpp, e_slot[fe], np.einsum("nda,n,ndb->nab", Jp[fe], w[fe], Jp[fe]))
        np.add.at(bp, e_slot[fe], np.einsum("nda,nd->na", Jp[fe], wr[fe]))
        Hpl = np.einsum("nda,n,ndb->nab", Jp, w, Jl)
        if it == 0:
            diag = [np.abs(np.diagonal(Hll[a_pt], axis1=1, axis2=2)).ravel(), np.abs(np.diagonal(Hpp[a_slots], axis1=1, axis2=2)).ravel()]
            lam, ni, n_bad = 1e-5 * float(np.concatenate(diag + [np.zeros(1)]).max()), 2.0, 0
        it_rec = dict(chi2=cur_chi, lambda0=lam, trials=[])
        out["trace"].append(it_rec)
        rho, qmax = 0.0, 0
        while True:
            backup = (Q.copy(), Tt.copy(), X.copy())
            xp, xl, ok = np.zeros((Kf, 6)), np.zeros((P, 3)), True
            if solver in ("schur", "blocked"):
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
                    Sm, rhs = S.reshape(Kf * 6, Kf * 6)[np.ix_(idx, idx)], bs.reshape(-1)[idx]
                    ok, sol = ldlt_solve(Sm, rhs) if solver == "schur" else blocked_ldlt_solve(Sm, rhs)
                    if ok:
                        xp.reshape(-1)[idx] = sol
                if ok:
                    cl = bl.copy()
                    np.subtract.at(cl, e_pt[fe], np.einsum("nab,na->nb", Hpl[fe], xp[e_slot[fe]]))
                    xl[a_pt] = np.einsum("pab,pb->pa", Dinv, cl)[a_pt]
                else:
                    xp[:] = 0
            else:
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
                Q[c], Tt[c] = se3_mul(*se3_exp(xp[slot[c]]), Q[c], Tt[c])
            X[a_pt] = X[a_pt] + xl[a_pt]
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
                Q, Tt, X = backup
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
    info16[6:9] = [done, trials, exit_taken]
    for c in np.flatnonzero(a_kf):
        out["T"][c] = se3_to_T(Q[c], Tt[c])
    out["Xw"][a_pt] = X[a_pt]
    return out
