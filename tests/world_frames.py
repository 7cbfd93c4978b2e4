"""World frames far from the identity, shared by the frame-sweep tests (helper, no tests).

Every tracking parity test plants its data around synth.make_scene's poses: T_ref = I, T_cur half a degree and three
centimetres away.  A rigid change of world frame G leaves images and keypoints untouched and moves everything else:

    X' = R_G X + t_G        n' = R_G n        T' = T G^-1    for every pose T (camera <- world)

so every stage must take the same decisions and return pose' = pose G^-1.  The table below holds the frames that reach
what R ~ I, t ~ 0 never reaches: the three `trace <= 0` branches of the matrix -> quaternion conversion (Eigen's
QuaternionBase::operator=(MatrixBase)), its `t > 0` boundary and its strict `>` ties, and a translation that cancels
against R X.  The two tie frames are written down entry by entry (0, 1 and -1 only), not computed from cos / sin, so
that the ties are ties; the asserts at the bottom of the module pin that."""
import numpy as np

import cameras as CM
import sweep_rig as SR
from sdslam_amd import synth
from sweep_rig import MOTIONS, POSE_BOUND, START, matched_points, planted_case, planted_uright      # noqa: F401  (named WF.* by the tests)


def _rot(omega_deg, t=(0.0, 0.0, 0.0)):
    G = synth.se3_exp((0.0, 0.0, 0.0), omega_deg)
    G[:3, 3] = t
    return G


def _exact(R, t=(0.0, 0.0, 0.0)):
    G = np.eye(4)
    G[:3, :3] = np.asarray(R, np.float64)
    G[:3, 3] = t
    return G


_OBLIQUE = np.array([2.0, -1.0, 2.0]) / 3.0         # a unit vector with rational entries

# name -> G (4x4, new world <- old world)
FRAMES = {
    "id": np.eye(4),                                            # control: today's results
    "rx170": _rot((170.0, 0.0, 0.0)),                           # trace < 0, largest diagonal x
    "ry170": _rot((0.0, 170.0, 0.0)),                           # ... y
    "rz170": _rot((0.0, 0.0, 170.0)),                           # ... z
    "perm120": _exact([[0, 0, 1], [1, 0, 0], [0, 1, 0]]),       # 120 deg about (1,1,1)/sqrt 3: trace 0, diagonals tied
    "r180xy": _exact([[0, 1, 0], [1, 0, 0], [0, 0, -1]]),       # 180 deg about (1,1,0)/sqrt 2: m00 == m11 == 0, m22 = -1
    "far": _rot(35.0 * _OBLIQUE, (400.0, -300.0, 150.0)),       # t' cancels against R' X'; EPnP centroid; lever arm
    # 170 deg about axes with no small component: in rx170 ... rz170 two of the three vector components of the
    # quaternion are ~ 0, so mixing them up moves the start pose by half a degree, which the optimiser absorbs
    "ox170": _rot(170.0 * np.array([0.8, 0.48, 0.36])),         # trace < 0, largest diagonal x, every component large
    "oy170": _rot(170.0 * np.array([0.36, 0.8, 0.48])),         # ... y
    "oz170": _rot(170.0 * np.array([0.48, 0.36, 0.8])),         # ... z
}
NAMES = list(FRAMES)
EXACT_TIES = ("perm120", "r180xy")      # frames in which the old-frame identity becomes an exact tie matrix


def inverse(G):
    """G^-1 of a rigid transform, from the transpose (exact where G's entries are 0 / +-1)."""
    Gi = np.eye(4)
    Gi[:3, :3] = G[:3, :3].T
    Gi[:3, 3] = -(G[:3, :3].T @ G[:3, 3])
    return Gi


def move_pose(T, G):
    """Camera <- world pose T of the old frame, in the new one: T G^-1."""
    return np.asarray(T, np.float64) @ inverse(G)


def back_pose(Tp, G):
    """The inverse of move_pose: a pose of the new frame, in the old one."""
    return np.asarray(Tp, np.float64) @ G


def move_points(X, G):
    return np.ascontiguousarray(np.asarray(X, np.float64) @ G[:3, :3].T + G[:3, 3])


def move_dirs(n, G):
    return np.ascontiguousarray(np.asarray(n, np.float64) @ G[:3, :3].T)


def move_last(last, G):
    """A Tracker.set_last / synth.tracking_case / synth.planted_matches dict in the new frame: Xw is its only
    world-frame field."""
    out = dict(last)
    out["Xw"] = move_points(last["Xw"], G)
    return out


def move_local(case, G):
    """A Tracker.set_local / synth.local_map_case dict in the new frame: Xw and the viewing normals are world-frame
    fields; the distance interval and mfMaxDistance are lengths, which a rigid motion keeps."""
    out = dict(case)
    out["Xw"] = move_points(case["Xw"], G)
    out["normal"] = move_dirs(case["normal"], G)
    return out


def quat_branch(R):
    """The branch Eigen's matrix -> quaternion conversion takes for R: "w" (trace > 0) or the largest diagonal entry
    "x" / "y" / "z", ties resolved to the lower index by the strict `>`.  Restated here so that tests can assert which
    branch a pose reaches."""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return "w"
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return "xyz"[i]


def round_trip_longdouble(R):
    """matrix -> unit quaternion -> matrix by the textbook formulas in numpy longdouble, independent of Eigen's branch
    order: the component of largest magnitude comes from the diagonal (4 q_i^2 = 1 + 2 m_ii - trace, 4 w^2 = 1 + trace),
    the other three from the off-diagonal sums and differences divided by it."""
    m = np.asarray(R, np.longdouble)
    one, two, four = np.longdouble(1), np.longdouble(2), np.longdouble(4)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    sq = np.array([one + two * m[0, 0] - tr, one + two * m[1, 1] - tr, one + two * m[2, 2] - tr, one + tr], np.longdouble)
    k = int(np.argmax(sq))
    q = np.zeros(4, np.longdouble)       # x, y, z, w
    q[k] = np.sqrt(sq[k]) / two
    d = four * q[k]
    if k == 3:
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) / d, (m[0, 2] - m[2, 0]) / d, (m[1, 0] - m[0, 1]) / d
    else:
        j, l = (k + 1) % 3, (k + 2) % 3
        q[3] = (m[l, j] - m[j, l]) / d
        q[j] = (m[j, k] + m[k, j]) / d
        q[l] = (m[l, k] + m[k, l]) / d
    q /= np.sqrt((q * q).sum())
    x, y, z, w = q
    out = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                    [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                    [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], np.longdouble)
    return out


# ---- the cases of the sweep: built once in the scenes' own frame, moved into a frame by the helpers above -----------
K = (synth.FX, synth.FY, synth.CX, synth.CY)
CFG = (300, 1.2, 8, 20)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
MP = 300                                           # the tracker's max_points


def _cut_to_max_points(O, rig):
    for f in rig["fr"]:
        f["last"] = {k: v[:MP] for k, v in f["last"].items()}
        f["local"] = {k: v[:MP] for k, v in f["local"].items()}


def oracle_rig(oracle):
    """The two VGA scenes of the sweep through synth's camera with the oracle's extraction, pyramids and tables, and the
    last-frame and local-map cases (30 points beside the keypoints' own, the rows the tracker has room for) in the scenes'
    own frame."""
    return SR.oracle_rig(oracle, "world_frames", CM.CAMERAS["synth"], 640, 480, CFG, MP, n_extra=30, extend=_cut_to_max_points)


def pose_error(T_est, T_true, G):
    """max |entry| of T_est - T_true G^-1, and of the same difference moved back into the scene's frame.  The two agree
    where t_G = 0.  Where it is not, a rotation error dR of the estimate shows up in the new frame's translation as
    dR R_true R_G^T t_G -- the lever arm |t_G| times an error that the data fix no better in one frame than in
    another -- so the accuracy bound of the old frame can only be asked for there."""
    T_est = np.asarray(T_est, np.float64)
    return np.abs(T_est - move_pose(T_true, G)).max(), np.abs(back_pose(T_est, G) - T_true).max()


def assert_converged(T_est, T_true, G, what):
    new, old = pose_error(T_est, T_true, G)
    assert old <= POSE_BOUND, (what, old)
    assert np.abs(T_est[:3, :3] - move_pose(T_true, G)[:3, :3]).max() <= POSE_BOUND, what
    if not G[:3, 3].any():
        assert new <= POSE_BOUND, (what, new)


def epnp_trials(G):
    """The twelve trials of tests/test_track_gpu.py::test_epnp_device_vs_oracle (eight rank-deficient 4-point sets, four
    n-point sets; same generator, same draws) with the world points moved into the frame before they are rounded to
    float: (Xw', uv, T') per trial."""
    rng = np.random.default_rng(11)
    out = []
    for trial in range(12):
        n = 4 if trial < 8 else int(rng.integers(6, 80))
        T = synth.se3_exp(rng.normal(size=3) * 0.1, rng.normal(size=3) * 5.0)
        Xc = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(1.0, 5.0, n)], 1)
        Xw = move_points((Xc - T[:3, 3]) @ T[:3, :3], G).astype(np.float32).astype(np.float64)
        Tp = move_pose(T, G)
        Xc = Xw @ Tp[:3, :3].T + Tp[:3, 3]
        uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)
        uv = (uv + rng.normal(size=uv.shape) * 0.3).astype(np.float32).astype(np.float64)
        out.append((Xw, uv, Tp))
    return out


def exact_three_edges(T0p):
    """Three keypoints at integer pixels and the world points that project onto them exactly under T0p (worked out in
    longdouble, rounded once): PoseOptimization's optimum on them is T0p itself, so what it returns is T0p after the
    matrix -> quaternion -> matrix round trip, plus Levenberg steps of rounding size."""
    kp = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                               ("class_id", "<i4")]))
    kp["x"], kp["y"] = [100, 500, 300], [120, 200, 400]
    z = np.array([2.0, 3.0, 4.0], np.longdouble)
    R, t = T0p[:3, :3].astype(np.longdouble), T0p[:3, 3].astype(np.longdouble)
    Xc = np.stack([(kp["x"].astype(np.longdouble) - K[2]) / K[0] * z, (kp["y"].astype(np.longdouble) - K[3]) / K[1] * z, z], 1)
    return kp, ((Xc - t) @ R).astype(np.float64)


# ---- the table is what its comments say ---------------------------------------------------------------------------
for _n, _G in FRAMES.items():
    _R = _G[:3, :3]
    assert np.abs(_R @ _R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(_R) - 1.0) < 1e-15, _n
    assert np.array_equal(_G[3], [0.0, 0.0, 0.0, 1.0]), _n
for _n in EXACT_TIES:
    _R = FRAMES[_n][:3, :3]
    assert np.isin(_R, (0.0, 1.0, -1.0)).all() and np.array_equal(_R @ _R.T, np.eye(3)) and not FRAMES[_n][:3, 3].any(), _n
# T0 = I of the old frame is G^-1 in the new one
_P, _X = inverse(FRAMES["perm120"])[:3, :3], inverse(FRAMES["r180xy"])[:3, :3]
assert np.trace(_P) == 0.0 and _P[0, 0] == _P[1, 1] == _P[2, 2] == 0.0 and quat_branch(_P) == "x"
assert _X[0, 0] == 0.0 and _X[1, 1] == 0.0 and _X[2, 2] == -1.0 and quat_branch(_X) == "x"
assert [quat_branch(inverse(FRAMES[n])[:3, :3]) for n in ("id", "rx170", "ry170", "rz170", "far")] == ["w", "x", "y", "z", "w"]
assert [quat_branch(inverse(FRAMES[n])[:3, :3]) for n in ("ox170", "oy170", "oz170")] == ["x", "y", "z"]
