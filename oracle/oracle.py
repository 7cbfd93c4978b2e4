"""ctypes binding of the CPU ORACLE (oracle/build/liboracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg -- never by the product package (sdslam_amd)."""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


def build(fast: bool = False) -> str:
    target = "build/liboracle_fast.so" if fast else "build/liboracle.so"
    subprocess.check_call(["make", "-s", "-C", _HERE, target])
    return os.path.join(_HERE, target)


_libs = {}


def lib(fast: bool = False):
    if fast not in _libs:
        path = os.path.join(_HERE, "build", "liboracle_fast.so" if fast else "liboracle.so")
        if os.environ.get("SD_ORACLE_LIB"):      # the sanitizer build (make -C oracle asan), tests/test_oracle_asan.py
            path = os.environ["SD_ORACLE_LIB"]
        elif not os.path.exists(path):
            build(fast)
        L = C.CDLL(path)
        L.orc_orb_create.restype = C.c_void_p
        L.orc_orb_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int]
        L.orc_orb_destroy.argtypes = [C.c_void_p]
        L.orc_fast_atan2.restype = C.c_float
        L.orc_fast_atan2.argtypes = [C.c_float, C.c_float]
        L.orc_ic_angle.restype = C.c_float
        L.orc_ic_angle.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float]
        L.orc_brief.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
        _libs[fast] = L
    return _libs[fast]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OrbOracle:
    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, th_fast=20, fast_build=False):
        self.L = lib(fast_build)
        self.nlevels = nlevels
        self.h = C.c_void_p(self.L.orc_orb_create(nfeatures, scale_factor, nlevels, th_fast))
        self.cap = max(4 * nfeatures, 64)

    def __del__(self):
        try:
            self.L.orc_orb_destroy(self.h)
        except Exception:
            pass

    def tables(self):
        n = self.nlevels
        sf, isf, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        quota = np.zeros(n, np.int32)
        umax = np.zeros(16, np.int32)
        self.L.orc_orb_tables(self.h, _p(sf), _p(isf), _p(s2), _p(is2), _p(quota), _p(umax))
        return dict(sf=sf, inv_sf=isf, sigma2=s2, inv_sigma2=is2, quota=quota, umax=umax)

    def extract(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = self.L.orc_orb_extract(self.h, _p(img), img.shape[1], img.shape[0], img.strides[0],
                                   _p(kps), _p(desc), self.cap)
        assert n <= self.cap
        return kps[:n].copy(), desc[:n].copy()

    def stage_ns(self):
        """Wall-clock ns of the last extract() per stage: pyramid, FAST+NMS, select, IC_Angle, blur, rBRIEF."""
        out = np.zeros(6)
        self.L.orc_orb_stage_ns.argtypes = [C.c_void_p, C.c_void_p]
        self.L.orc_orb_stage_ns(self.h, _p(out))
        return out

    def level(self, l, padded=False):
        w, h = C.c_int(), C.c_int()
        assert self.L.orc_orb_level_info(self.h, l, C.byref(w), C.byref(h)) == 0
        W, H = (w.value + 38, h.value + 38) if padded else (w.value, h.value)
        out = np.zeros((H, W), np.uint8)
        self.L.orc_orb_level_copy(self.h, l, int(padded), _p(out), W)
        return out

    def blurred(self, l):
        w, h = C.c_int(), C.c_int()
        self.L.orc_orb_level_info(self.h, l, C.byref(w), C.byref(h))
        out = np.zeros((h.value, w.value), np.uint8)
        if self.L.orc_orb_blurred_copy(self.h, l, _p(out), w.value) != 0:
            return None
        return out

    def level_keypoints(self, l):
        kps = np.zeros(self.cap, KP_DTYPE)
        n = self.L.orc_orb_level_keypoints(self.h, l, _p(kps), self.cap)
        return kps[:n].copy()

    def cell_totals(self, l):
        out = np.zeros(4096, np.int32)
        n = self.L.orc_orb_cell_totals(self.h, l, _p(out), 4096)
        return out[:n].copy()

    def ic_angle(self, img, x, y):
        img = np.ascontiguousarray(img, np.uint8)
        return float(self.L.orc_ic_angle(self.h, _p(img), img.strides[0], float(x), float(y)))

    def brief(self, blurred, x, y, angle):
        blurred = np.ascontiguousarray(blurred, np.uint8)
        d = np.zeros(32, np.uint8)
        self.L.orc_brief(self.h, _p(blurred), blurred.strides[0], float(x), float(y), float(angle), _p(d))
        return d


# ---- stage-level helpers -------------------------------------------------------------
def fast(img, threshold=20, nonmax=True):
    img = np.ascontiguousarray(img, np.uint8)
    cap = img.size
    kps = np.zeros(max(cap, 1), KP_DTYPE)
    n = lib().orc_fast(_p(img), img.shape[1], img.shape[0], img.strides[0], threshold, int(nonmax), _p(kps), cap)
    return kps[:n].copy()


def fast_score(img, x, y, threshold=20):
    img = np.ascontiguousarray(img, np.uint8)
    ptr = C.c_void_p(img.ctypes.data + y * img.strides[0] + x)
    return lib().orc_fast_score(ptr, img.strides[0], threshold)


def resize_linear(src, dw, dh):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.zeros((dh, dw), np.uint8)
    lib().orc_resize_linear(_p(src), src.shape[1], src.shape[0], src.strides[0], _p(dst), dw, dh, dw)
    return dst


def border101(src, b=19):
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape
    dst = np.zeros((h + 2 * b, w + 2 * b), np.uint8)
    lib().orc_border101(_p(src), w, h, src.strides[0], _p(dst), w + 2 * b, b)
    return dst


def blur7(src):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.zeros_like(src)
    lib().orc_blur7(_p(src), src.shape[1], src.shape[0], src.strides[0], _p(dst), dst.strides[0])
    return dst


def gauss_taps():
    k = np.zeros(7, np.int32)
    lib().orc_gauss_taps(_p(k))
    return k


def fast_atan2(y, x):
    return float(lib().orc_fast_atan2(float(y), float(x)))


def retain_best(kps, n_points):
    buf = np.ascontiguousarray(kps.copy())
    n = lib().orc_retain_best(_p(buf), len(buf), n_points)
    return buf[:n].copy()


# ---- ImageAlign / matcher / PnP oracles -------------------------------------------------
def _cm(T):
    """4x4 numpy (row-major math) -> 16 doubles column-major (Eigen::Matrix4d::data())."""
    return np.ascontiguousarray(np.asarray(T, np.float64).T).ravel().copy()


def _from_cm(v):
    return np.asarray(v, np.float64).reshape(4, 4).T.copy()


ALIGN_COUNTERFACTUALS = ("none", "reset_visible", "keep_h", "border2", "clear_stop", "gate_last", "stale_chi2")
ALIGN_DECISIONS = ("none", "accept", "rollback_chi2", "rollback_stop", "small", "converged", "iterations")   # orc_align_trace's codes
ALIGN_TRACE_LEVELS = (4, 3, 2)                   # the level of trace slot 0, 1, 2


def align(cur_levels, ref_levels, inv_sf, sf, Xw, T_ref, T_cur_init, K, mode=0, trace=False, counterfactual=0, h_order=0):
    """ImageAlign::ComputePose on explicit pyramids (lists of 2-D uint8 arrays, index = level).
    Returns dict(ok, T (4x4), error, iters (per level), chi2).  With trace=True (orc_align_trace, the same code path) also `trace`: a list
    with one dict per level that ran, in the order 4, 3, 2: level, exit (a name of ALIGN_DECISIONS), iters, gate (the error_ that mode 2 /
    3 compared after the level, or None), chi2 (chi2_ after the level) and `its`, one dict per iteration: n_meas, chi2_sum (the float
    sum), new_chi2, chi2_before, error (error_ after the decision), x[6], pose (the trial pose), decision, and the per-point flags has_jac, visible, measured
    over the points taken.  counterfactual (trace only): 0 is the reference, ALIGN_COUNTERFACTUALS names the deliberately wrong variants
    that test cases are shown to notice; h_order=1 (trace only) forms H and Jres in the device's order, to certify cases."""
    counterfactual = ALIGN_COUNTERFACTUALS.index(counterfactual) if isinstance(counterfactual, str) else int(counterfactual)
    assert trace or (counterfactual == 0 and h_order == 0)
    L = lib()
    n = len(cur_levels)
    cur = [np.ascontiguousarray(a, np.uint8) for a in cur_levels]
    ref = [np.ascontiguousarray(a, np.uint8) for a in ref_levels]
    PtrArr = C.c_void_p * n
    cp = PtrArr(*[a.ctypes.data for a in cur])
    rp = PtrArr(*[a.ctypes.data for a in ref])
    w = np.array([a.shape[1] for a in cur], np.int32)
    h = np.array([a.shape[0] for a in cur], np.int32)
    sc = np.array([a.strides[0] for a in cur], np.int32)
    sr = np.array([a.strides[0] for a in ref], np.int32)
    inv_sf = np.ascontiguousarray(inv_sf, np.float32)
    sf = np.ascontiguousarray(sf, np.float32)
    Xw = np.ascontiguousarray(Xw, np.float64)
    Tr = _cm(T_ref)
    Tc = _cm(T_cur_init)
    err = C.c_double()
    chi2 = C.c_double()
    iters = np.zeros(n, np.int32)
    L.orc_align.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                            C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    args = (n, cp, rp, _p(w), _p(h), _p(sc), _p(sr), _p(inv_sf), _p(sf), _p(Xw), len(Xw), _p(Tr), _p(Tc),
            float(K[0]), float(K[1]), float(K[2]), float(K[3]), mode, C.byref(err), _p(iters), C.byref(chi2))
    if not trace:
        ok = L.orc_align(*args)
        return dict(ok=bool(ok), T=_from_cm(Tc), error=err.value, iters=iters, chi2=chi2.value)
    npts = len(Xw)
    lv_i, lv_d = np.zeros((3, 4), np.int32), np.zeros((3, 2))
    it_i, it_d, flags = np.zeros((3, 30, 2), np.int32), np.zeros((3, 30, 28)), np.zeros((3, 30, max(npts, 1)), np.uint8)
    L.orc_align_trace.argtypes = L.orc_align.argtypes + [C.c_void_p] * 5 + [C.c_int, C.c_int]
    ok = L.orc_align_trace(*args, _p(lv_i), _p(lv_d), _p(it_i), _p(it_d), _p(flags), counterfactual, int(h_order))
    taken = min(npts, 100 if mode in (2, 3) else 300)
    levels = []
    for s in range(3):
        if not lv_i[s, 0]:
            continue
        its = []
        for i in range(lv_i[s, 2]):
            f = flags[s, i, :taken]
            its.append(dict(n_meas=int(it_i[s, i, 0]), decision=ALIGN_DECISIONS[it_i[s, i, 1]], chi2_sum=it_d[s, i, 0], new_chi2=it_d[s, i, 1],
                            chi2_before=it_d[s, i, 2], error=it_d[s, i, 3], x=it_d[s, i, 4:10].copy(), pose=it_d[s, i, 12:28].reshape(4, 4).copy(), has_jac=(f & 1) != 0,
                            visible=(f & 2) != 0, measured=(f & 4) != 0))
        levels.append(dict(level=ALIGN_TRACE_LEVELS[s], exit=ALIGN_DECISIONS[lv_i[s, 1]], iters=int(lv_i[s, 2]),
                           gate=float(lv_d[s, 0]) if lv_i[s, 3] else None, chi2=float(lv_d[s, 1]), its=its))
    return dict(ok=bool(ok), T=_from_cm(Tc), error=err.value, iters=iters, chi2=chi2.value, trace=levels)


def se3_exp(update6):
    out = np.zeros(16)
    u = np.ascontiguousarray(update6, np.float64)
    lib().orc_se3_exp(_p(u), _p(out))
    return _from_cm(out)


def ldlt_solve6(H, b):
    H = np.ascontiguousarray(H, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(6)
    lib().orc_ldlt_solve6(_p(H), _p(b), _p(x))
    return x


def search_by_projection(kps_un, desc, sf, bounds, K, T_cw, T_lw, last, th=8.0, mono=True, check_ori=True,
                         u_right=None, mbf=0.0, mb=0.0, cur_match=None):
    """ORBmatcher::SearchByProjection(Frame&, const Frame&).  `last` = dict(valid, Xw, desc, octave,
    angle, obs).  Returns (nmatches, cur_match[N])."""
    L = lib()
    kps_un = np.ascontiguousarray(kps_un)
    desc = np.ascontiguousarray(desc, np.uint8)
    N = len(kps_un)
    cm = np.full(N, -1, np.int32) if cur_match is None else np.ascontiguousarray(cur_match, np.int32).copy()
    sf = np.ascontiguousarray(sf, np.float32)
    Tc, Tl = _cm(T_cw), _cm(T_lw)
    valid = np.ascontiguousarray(last["valid"], np.uint8)
    Xw = np.ascontiguousarray(last["Xw"], np.float64)
    md = np.ascontiguousarray(last["desc"], np.uint8)
    oc = np.ascontiguousarray(last["octave"], np.int32)
    an = np.ascontiguousarray(last["angle"], np.float32)
    ob = np.ascontiguousarray(last["obs"], np.int32)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    L.orc_search_by_projection.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_float] * 10 + \
        [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_int, C.c_int, C.c_void_p]
    n = L.orc_search_by_projection(N, _p(kps_un), _p(desc), _p(ur) if ur is not None else None, _p(sf),
                                   float(bounds[0]), float(bounds[1]), float(bounds[2]), float(bounds[3]),
                                   float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(mbf), float(mb),
                                   _p(Tc), _p(Tl), len(valid), _p(valid), _p(Xw), _p(md), _p(oc), _p(an), _p(ob),
                                   float(th), int(mono), int(check_ori), _p(cm))
    return n, cm


def search_local_points(kps_un, desc, sf, log_sf, bounds, K, mbf, T_cw, pts, th=1.0, nnratio=0.8, u_right=None, kp_claimed=None,
                        cos_limit=0.5):
    """TrackLocalMap search: isInFrustum + PredictScale + SearchByProjection(F, vpMapPoints, th).  `pts` = dict(cand, Xw,
    normal, min_dist, max_dist, mf_max_dist, desc, obs).  Returns dict(n, match[N], in_view[M], proj[M,3], level[M], cos[M])."""
    L = lib()
    kps_un = np.ascontiguousarray(kps_un)
    desc = np.ascontiguousarray(desc, np.uint8)
    N, M = len(kps_un), len(pts["cand"])
    sf = np.ascontiguousarray(sf, np.float32)
    Tc = _cm(T_cw)
    cand = np.ascontiguousarray(pts["cand"], np.uint8)
    Xw = np.ascontiguousarray(pts["Xw"], np.float64)
    nr = np.ascontiguousarray(pts["normal"], np.float64)
    mn = np.ascontiguousarray(pts["min_dist"], np.float32)
    mx = np.ascontiguousarray(pts["max_dist"], np.float32)
    mf = np.ascontiguousarray(pts["mf_max_dist"], np.float32)
    md = np.ascontiguousarray(pts["desc"], np.uint8)
    ob = np.ascontiguousarray(pts["obs"], np.int32)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    kc = None if kp_claimed is None else np.ascontiguousarray(kp_claimed, np.uint8)
    match = np.zeros(N, np.int32)
    inv = np.zeros(M, np.uint8)
    proj = np.zeros((M, 3), np.float32)
    lvl = np.zeros(M, np.int32)
    cs = np.zeros(M, np.float32)
    L.orc_search_local_points.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_float] * 10 + \
        [C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_float] * 3 + [C.c_void_p] * 5
    n = L.orc_search_local_points(N, _p(kps_un), _p(desc), _p(ur) if ur is not None else None, _p(sf), len(sf), float(log_sf),
                                  float(bounds[0]), float(bounds[1]), float(bounds[2]), float(bounds[3]),
                                  float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(mbf), _p(Tc), M, _p(cand), _p(Xw), _p(nr),
                                  _p(mn), _p(mx), _p(mf), _p(md), _p(ob), _p(kc) if kc is not None else None, float(th), float(nnratio),
                                  float(cos_limit), _p(match), _p(inv), _p(proj), _p(lvl), _p(cs))
    return dict(n=n, match=match, in_view=inv.astype(bool), proj=proj, level=lvl, cos=cs)


COUNTERFACTUALS = ("none", "classify_at_est", "huber_off_early", "huber_round4", "no_restart", "stereo_delta", "gate_le10")
LM_EXITS = ("not_run", "nbad", "qmax", "rho_zero", "iterations")     # the exit codes of orc_pose_optimization_trace


def pose_optimization(kps_un, has_mp, Xw, inv_sigma2, K, T_cw, u_right=None, bf=0.0, trace=False, counterfactual=0):
    """Optimizer::PoseOptimization (g2o Levenberg, Huber, 4 x 10 iterations).  Returns dict(n_inliers, T, outlier[N], info[5]);
    with trace=True (orc_pose_optimization_trace, the same code path) also round_outlier[4][N], round_its[4], round_trials[4],
    round_exit[4] (names of LM_EXITS) and chi2[N], the float chi2 of every edge at the last classification.  counterfactual (trace only): 0 is
    the reference; COUNTERFACTUALS names the deliberately wrong variants that test cases are shown to notice."""
    counterfactual = COUNTERFACTUALS.index(counterfactual) if isinstance(counterfactual, str) else int(counterfactual)
    assert trace or counterfactual == 0
    L = lib()
    kps_un = np.ascontiguousarray(kps_un)
    N = len(kps_un)
    xy = np.ascontiguousarray(np.stack([kps_un["x"], kps_un["y"]], 1), np.float32)
    oc = np.ascontiguousarray(kps_un["octave"], np.int32)
    hm = np.ascontiguousarray(has_mp, np.uint8)
    X = np.ascontiguousarray(Xw, np.float64)
    ur = np.full(N, -1, np.float32) if u_right is None else np.ascontiguousarray(u_right, np.float32)
    isg = np.ascontiguousarray(inv_sigma2, np.float32)
    Tc = _cm(T_cw)
    To = np.zeros(16)
    out = np.zeros(N, np.uint8)
    info = np.zeros(5, np.int32)
    args = (N, _p(hm), _p(xy), _p(oc), _p(ur), _p(isg), _p(X), float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(bf), _p(Tc), _p(To),
            _p(out), _p(info))
    L.orc_pose_optimization.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_float] * 5 + [C.c_void_p] * 4
    if not trace:
        n = L.orc_pose_optimization(*args)
        return dict(n_inliers=n, T=_from_cm(To), outlier=out.astype(bool), info=info)
    ro, ri, chi2 = np.zeros((4, max(N, 1)), np.uint8), np.zeros((4, 3), np.int32), np.zeros(max(N, 1), np.float32)
    L.orc_pose_optimization_trace.argtypes = L.orc_pose_optimization.argtypes + [C.c_void_p] * 3 + [C.c_int]
    n = L.orc_pose_optimization_trace(*args, _p(ro), _p(ri), _p(chi2), counterfactual)
    return dict(n_inliers=n, T=_from_cm(To), outlier=out.astype(bool), info=info, round_outlier=ro[:, :N].astype(bool), round_its=ri[:, 0],
                round_trials=ri[:, 1], round_exit=[LM_EXITS[e] for e in ri[:, 2]], chi2=chi2[:N])


def stereo_from_rgbd(kps, kps_un, depth, mbf):
    """Frame::ComputeStereoFromRGBD -> (mvuRight, mvDepth)."""
    L = lib()
    kps, kps_un = np.ascontiguousarray(kps), np.ascontiguousarray(kps_un)
    d = np.ascontiguousarray(depth, np.float32)
    ur, dd = np.zeros(len(kps), np.float32), np.zeros(len(kps), np.float32)
    L.orc_stereo_from_rgbd.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.orc_stereo_from_rgbd(len(kps), _p(kps), _p(kps_un), _p(d), d.shape[1], float(mbf), _p(ur), _p(dd))
    return ur, dd


def features_in_area(kps_un, bounds, x, y, r, min_level=-1, max_level=-1):
    L = lib()
    kps_un = np.ascontiguousarray(kps_un)
    out = np.zeros(len(kps_un) + 1, np.int32)
    L.orc_features_in_area.argtypes = [C.c_int, C.c_void_p] + [C.c_float] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = L.orc_features_in_area(len(kps_un), _p(kps_un), *[float(b) for b in bounds], float(x), float(y), float(r),
                               min_level, max_level, _p(out), len(out))
    return out[:n].copy()


def search_by_points(kps_un1, desc1, has_mp1, kps_un2, desc2, has_mp2, nnratio=0.75, check_ori=True):
    """ORBmatcher::SearchByPoints(currentKF, pKF, matches) -> (nmatches, matches12[N1] = pKF keypoint index or -1)."""
    L = lib()
    k1, k2 = np.ascontiguousarray(kps_un1), np.ascontiguousarray(kps_un2)
    d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
    h1, h2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
    m = np.zeros(len(k1), np.int32)
    L.orc_search_by_points.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_float, C.c_int, C.c_void_p]
    n = L.orc_search_by_points(len(k1), _p(k1), _p(d1), _p(h1), len(k2), _p(k2), _p(d2), _p(h2), float(nnratio), int(check_ori), _p(m))
    return n, m


def descriptor_distance(a, b):
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    return int(lib().orc_descriptor_distance(_p(a), _p(b)))


class PnPOracle:
    """SD_SLAM::PnPsolver(F, vpMapPointMatches) + SetRansacParameters + iterate."""

    def __init__(self, valid, kp_xy, kp_octave, level_sigma2, Xw, K):
        self.L = lib()
        self.n = len(valid)
        valid = np.ascontiguousarray(valid, np.uint8)
        kp_xy = np.ascontiguousarray(kp_xy, np.float32)
        kp_octave = np.ascontiguousarray(kp_octave, np.int32)
        level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
        Xw = np.ascontiguousarray(Xw, np.float64)
        self.L.orc_pnp_create.restype = C.c_void_p
        self.L.orc_pnp_create.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 4
        self.h = C.c_void_p(self.L.orc_pnp_create(self.n, _p(valid), _p(kp_xy), _p(kp_octave), _p(level_sigma2), _p(Xw),
                                                  float(K[0]), float(K[1]), float(K[2]), float(K[3])))
        self.L.orc_pnp_destroy.argtypes = [C.c_void_p]
        self.L.orc_pnp_set_ransac.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        self.L.orc_pnp_iterate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        self.L.orc_pnp_params.argtypes = [C.c_void_p] * 4

    def __del__(self):
        try:
            self.L.orc_pnp_destroy(self.h)
        except Exception:
            pass

    def set_ransac(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        self.L.orc_pnp_set_ransac(self.h, probability, min_inliers, max_iterations, min_set, epsilon, th2)

    def params(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self.L.orc_pnp_params(self.h, C.byref(a), C.byref(b), C.byref(c))
        return dict(N=a.value, min_inliers=b.value, max_its=c.value)

    def iterate(self, n_iterations, rand_stream=None):
        T = np.zeros(16, np.float32)
        inl = np.zeros(self.n, np.uint8)
        nin, nomore, done = C.c_int(), C.c_int(), C.c_int()
        rs = None if rand_stream is None else np.ascontiguousarray(rand_stream, np.int32)
        ok = self.L.orc_pnp_iterate(self.h, n_iterations, _p(rs) if rs is not None else None, 0 if rs is None else len(rs),
                                    _p(T), _p(inl), C.byref(nin), C.byref(nomore), C.byref(done))
        return dict(ok=bool(ok), T=T.reshape(4, 4).copy(), inliers=inl.astype(bool), n_inliers=nin.value,
                    no_more=bool(nomore.value), iterations=done.value)


def epnp(Xw, uv, K):
    Xw = np.ascontiguousarray(Xw, np.float64)
    uv = np.ascontiguousarray(uv, np.float64)
    R = np.zeros(9)
    t = np.zeros(3)
    L = lib()
    L.orc_epnp.restype = C.c_double
    L.orc_epnp.argtypes = [C.c_int, C.c_void_p, C.c_void_p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p]
    e = L.orc_epnp(len(Xw), _p(Xw), _p(uv), float(K[0]), float(K[1]), float(K[2]), float(K[3]), _p(R), _p(t))
    return R.reshape(3, 3), t, e


def svd_square(A):
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[0]
    W, Ut, Vt = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    lib().orc_svd_square(_p(A), n, _p(W), _p(Ut), _p(Vt))
    return W, Ut, Vt


def glibc_rand_stream(n, seed=1):
    """n raw rand() values of glibc's TYPE_3 additive-feedback generator seeded with `seed`
    (the reference never seeds: SD_SLAM::Random draws from the default seed-1 state,
    reference src/extra/utils.cc:23-26).  Restated, so tests do not perturb the process RNG."""
    r = [0] * 34
    r[0] = seed
    for i in range(1, 31):
        hi, lo = divmod(r[i - 1], 127773)
        w = 16807 * lo - 2836 * hi
        if w < 0:
            w += 2147483647
        r[i] = w
    for i in range(31, 34):
        r[i] = r[i - 31]
    out = []
    state = r[:]
    k = 34
    buf = state
    for i in range(34, 344 + n):
        v = (buf[i - 31] + buf[i - 3]) & 0xFFFFFFFF
        buf.append(v)
        if i >= 344:
            out.append(v >> 1)
    return np.array(out, np.int32)


def undistort_points(xy, K, dist5):
    """Frame::UndistortKeyPoints / cv::undistortPoints(pts, pts, K, dist, Mat(), K)."""
    L = lib()
    xy = np.ascontiguousarray(xy, np.float32)
    d = np.ascontiguousarray(dist5, np.float32)
    out = np.zeros_like(xy)
    L.orc_undistort_points.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.orc_undistort_points(len(xy), _p(xy), float(K[0]), float(K[1]), float(K[2]), float(K[3]), _p(d), _p(out))
    return out


def track_with_motion_model(pyr_cur, pyr_ref, tab, kps_un, desc, bounds, K, T_last, T_pred, last, th, mono=True, align_mode=0,
                            u_right=None, mbf=0.0, mb=0.0, min_matches=20, min_inliers=10, T_aligned=None):
    """Tracking::TrackWithMotionModel (reference src/Tracking.cc:654-718) composed from the oracle's stages, decision by
    decision: align (failure keeps the predicted pose, :668-672) -> SearchByProjection(th) (:676-678) -> < 20: pose :=
    predicted, SearchByProjection(2 th) (:681-686) -> < 20: return false (:688-691) -> PoseOptimization (:694) -> discard
    outliers, count nmatchesMap (:697-711) -> nmatchesMap >= 10 (:713-718).  align_mode 1 = TrackReferenceKeyFrame's
    ComputePose(frame, keyframe) (:583-644); -1 = align_image_ off.  T_aligned (optional) replaces the aligner's pose by a
    given one (tests pass the device's, so that the matcher is compared on identical input).
    Returns dict(status 0 few matches / 1 few inliers / 2 tracked, nmatches, nmatches_map, retried, T, match[N], align)."""
    ra = None
    T = np.array(T_pred, np.float64)
    if align_mode >= 0:
        Xw = last["Xw"][np.asarray(last["valid"]) != 0]
        ra = align(pyr_cur, pyr_ref, tab["inv_sf"], tab["sf"], Xw, T_last, T_pred, K, mode=align_mode)
        if ra["ok"]:
            T = ra["T"] if T_aligned is None else np.array(T_aligned, np.float64)
    kw = dict(mono=mono, check_ori=True, u_right=u_right, mbf=mbf, mb=mb)
    nm, cm = search_by_projection(kps_un, desc, tab["sf"], bounds, K, T, T_last, last, th=th, **kw)
    retried = 0
    if nm < min_matches:
        T = np.array(T_pred, np.float64)
        nm, cm = search_by_projection(kps_un, desc, tab["sf"], bounds, K, T, T_last, last, th=2 * th, **kw)
        retried = 1
    if nm < min_matches:
        return dict(status=0, nmatches=nm, nmatches_map=0, retried=retried, T=T, match=cm, align=ra)
    has = cm >= 0
    rp = pose_optimization(kps_un, has, np.asarray(last["Xw"])[np.maximum(cm, 0)], tab["inv_sigma2"], K, T, u_right=u_right, bf=mbf)
    cm = cm.copy()
    nmap = 0
    for i in range(len(cm)):
        if cm[i] >= 0:
            if rp["outlier"][i]:
                cm[i] = -1
                nm -= 1
            elif last["obs"][cm[i]] > 0:
                nmap += 1
    return dict(status=2 if nmap >= min_inliers else 1, nmatches=nm, nmatches_map=nmap, retried=retried, T=rp["T"], match=cm, align=ra)


def track_local_map(kps_un, desc, tab, log_sf, bounds, K, T_cw, frame_match, last, local, th=1.0, nnratio=0.8, cos_limit=0.5,
                    min_inliers=30, u_right=None, mbf=0.0):
    """Tracking::TrackLocalMap (reference src/Tracking.cc:720-751) composed from the oracle's stages: SearchLocalPoints
    (:898-939; keypoints whose frame match has observations are closed to the search, src/ORBmatcher.cc:81-83) ->
    PoseOptimization over the union of frame matches and local matches (:729) -> mnMatchesInliers (:733-742) -> >= 30.
    frame_match[N]: indices into `last` (-1 none); `local`: dict for search_local_points.  Returns dict(status 1 failed /
    2 tracked, n_points, n_inliers, n_local, match[N] with local points as index + len(last arrays' capacity M), T, outlier, search)."""
    frame_match = np.asarray(frame_match, np.int32)
    N = len(kps_un)
    claimed = np.array([frame_match[i] >= 0 and last["obs"][frame_match[i]] > 0 for i in range(N)], np.uint8)
    sr = search_local_points(kps_un, desc, tab["sf"], log_sf, bounds, K, mbf, T_cw, local, th=th, nnratio=nnratio, cos_limit=cos_limit,
                             u_right=u_right, kp_claimed=claimed)
    lm = sr["match"]
    has = (lm >= 0) | (frame_match >= 0)
    Xw = np.zeros((N, 3))
    obs = np.zeros(N, np.int64)
    for i in range(N):
        if lm[i] >= 0:
            Xw[i], obs[i] = local["Xw"][lm[i]], local["obs"][lm[i]]
        elif frame_match[i] >= 0:
            Xw[i], obs[i] = last["Xw"][frame_match[i]], last["obs"][frame_match[i]]
    rp = pose_optimization(kps_un, has, Xw, tab["inv_sigma2"], K, T_cw, u_right=u_right, bf=mbf)
    ninl = int(sum(1 for i in range(N) if has[i] and not rp["outlier"][i] and obs[i] > 0))
    return dict(status=2 if ninl >= min_inliers else 1, n_points=int(has.sum()), n_inliers=ninl, n_local=int((lm >= 0).sum()),
                local_match=lm, frame_match=frame_match, has=has, T=rp["T"], outlier=rp["outlier"], search=sr)
