"""Seeded cases for the map-point refresh (k_refresh_points): lists of points, each dict(desc [N, 32], centre [N, 3], octave [N],
ref_obs, X [3], kf_bad [N], bad), and their CSR form as sd_debug_refresh_points and refresh_ref.refresh_points take it.

The shapes are the smallest at which the kernel can go wrong: a lane owns rows i, i + 64, i + 128, i + 192, a wave one point, a
workgroup four points, the capacity is 256 observations."""
import numpy as np

NLEVELS = 8
SF = np.cumprod(np.r_[np.float32(1), np.full(NLEVELS - 1, np.float32(1.2))]).astype(np.float32)   # mvScaleFactors of (1.2, 8)
SIZES = (1, 2, 3, 4, 63, 64, 65, 128, 255, 256)


def flipped(rng, base, bits):
    """`base` with `bits` distinct random bits flipped."""
    d = np.unpackbits(np.asarray(base, np.uint8))
    d[rng.choice(256, int(bits), replace=False)] ^= 1
    return np.packbits(d)


def cluster(rng, N, lo=5, hi=120):
    """N descriptors around one random base, every one a different number of bits away: rows with well-spread medians."""
    base = rng.integers(0, 256, 32).astype(np.uint8)
    return np.stack([flipped(rng, base, rng.integers(lo, hi + 1)) for _ in range(N)])


def point(rng, desc, ref_obs=None, kf_bad=None, bad=False, octave=None):
    N = len(desc)
    return dict(desc=np.asarray(desc, np.uint8).reshape(N, 32), centre=rng.uniform(-1, 1, (N, 3)),
                octave=rng.integers(0, NLEVELS, N).astype(np.int32) if octave is None else np.asarray(octave, np.int32),
                ref_obs=int(rng.integers(0, N)) if ref_obs is None and N else int(ref_obs or 0),
                X=rng.uniform(-2, 2, 3) + np.array([0.0, 0.0, 6.0]), kf_bad=np.zeros(N, np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8),
                bad=bool(bad))


def csr(points):
    """The arrays of the debug entry / the restatement."""
    off = np.zeros(len(points) + 1, np.int32)
    off[1:] = np.cumsum([len(p["desc"]) for p in points])
    cat = lambda k, tail, dt: (np.concatenate([np.asarray(p[k], dt).reshape((-1,) + tail) for p in points])
                               if points else np.zeros((0,) + tail, dt))
    return dict(obs_off=off, obs_desc=cat("desc", (32,), np.uint8), obs_centre=cat("centre", (3,), np.float64),
                obs_octave=cat("octave", (), np.int32), obs_kf_bad=cat("kf_bad", (), np.uint8),
                ref_obs=np.array([p["ref_obs"] for p in points], np.int32), Xw=np.array([p["X"] for p in points], np.float64).reshape(-1, 3),
                point_bad=np.array([p["bad"] for p in points], np.uint8))


def sized(seed=1):
    """One point of every size in SIZES."""
    rng = np.random.default_rng(seed)
    return [point(rng, cluster(rng, N)) for N in SIZES]


def too_many(seed=2):
    """257 observations between two ordinary points."""
    rng = np.random.default_rng(seed)
    return [point(rng, cluster(rng, 7)), point(rng, cluster(rng, 257)), point(rng, cluster(rng, 64))]


def complementary(seed=3):
    """Rows whose median is the distance 256 of complementary descriptors, placed BEFORE the rows that should win: a row kept in
    bytes reads 256 as 0, gives such a row the median 0 and lets it win by order.  `a_row` is that row, `winner` the right one.
      N = 3: a, ~a, ~a                      -> medians 256, 0, 0: row 1
      N = 41 / 70 / 200: a, then ~a N - 1 times: the same
      N = 140: 64 far-flung descriptors, a at row 64 (a lane's second row), ~a 75 times: a's row sorted is 0, 64 distances
               around 128, 75 times 256, rank 69 reads 256; the ~a rows read 0: row 65
      N = 2: a, ~a: both medians are the diagonal, row 0
    (256 as the WINNER's rank element is impossible for N >= 2: more than half the list would be one descriptor, median 0.)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, 32).astype(np.uint8)
    pts = [dict(point(rng, np.stack([a, ~a, ~a])), a_row=0, winner=1)]
    for N in (41, 70, 200):
        pts.append(dict(point(rng, np.stack([a] + [~a] * (N - 1))), a_row=0, winner=1))
    far = [flipped(rng, rng.integers(0, 256, 32).astype(np.uint8), 0) for _ in range(64)]
    pts.append(dict(point(rng, np.stack(far + [a] + [~a] * 75)), a_row=64, winner=65))
    pts.append(dict(point(rng, np.stack([a, ~a])), a_row=0, winner=0))
    return pts


def identical(seed=4):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, 32).astype(np.uint8)
    return [point(rng, np.tile(d, (N, 1))) for N in (5, 64, 70, 256)]


def tied(seed=5):
    """Two identical descriptors (identical rows, equal medians) close to the base of a far-flung cluster, at rows (first,
    second): the first wins.  Pairs across a lane's first and later rows, and across the 64-row groups."""
    rng = np.random.default_rng(seed)
    pts = []
    for N, first, second in ((100, 10, 80), (100, 80, 90), (65, 0, 64), (128, 63, 64), (256, 1, 255), (256, 130, 200), (200, 70, 5 + 64)):
        first, second = min(first, second), max(first, second)
        base = rng.integers(0, 256, 32).astype(np.uint8)
        d = np.stack([flipped(rng, base, rng.integers(90, 121)) for _ in range(N)])
        d[first] = d[second] = flipped(rng, base, 3)
        pts.append(dict(point(rng, d), winner=first))
    return pts


def bad_keyframes(seed=6):
    """Observations of bad keyframes: some, all, the winner's neighbours (best_obs is a position in the CALLER's list), the first
    64, and a bad reference keyframe (UpdateNormalAndDepth uses it all the same)."""
    rng = np.random.default_rng(seed)
    pts = []
    for N in (6, 70, 256):
        pts.append(point(rng, cluster(rng, N), kf_bad=rng.random(N) < 0.4))
    pts.append(point(rng, cluster(rng, 9), kf_bad=np.ones(9)))
    for N, w in ((12, 5), (140, 100)):                           # the tight pair of `tied` at w, its neighbours in the list bad
        base = rng.integers(0, 256, 32).astype(np.uint8)
        d = np.stack([flipped(rng, base, rng.integers(90, 121)) for _ in range(N)])
        d[w] = flipped(rng, base, 2)
        kb = np.zeros(N, np.uint8)
        kb[[w - 2, w - 1, w + 1]] = 1
        pts.append(dict(point(rng, d, kf_bad=kb), winner=w))
    kb = np.zeros(130, np.uint8)
    kb[:64] = 1
    pts.append(point(rng, cluster(rng, 130), kf_bad=kb))
    kb = np.zeros(5, np.uint8)
    kb[2] = 1
    pts.append(point(rng, cluster(rng, 5), ref_obs=2, kf_bad=kb))
    return pts


def skipped(seed=7):
    """A bad point and a point without observations between ordinary ones."""
    rng = np.random.default_rng(seed)
    return [point(rng, cluster(rng, 3)), point(rng, cluster(rng, 4), bad=True), point(rng, np.zeros((0, 32), np.uint8)),
            point(rng, cluster(rng, 66), bad=True), point(rng, cluster(rng, 2))]


def ref_octaves(seed=8):
    """The reference keyframe's keypoint at octave 0 and at nlevels - 1."""
    rng = np.random.default_rng(seed)
    pts = []
    for N, r, o in ((4, 0, 0), (4, 3, NLEVELS - 1), (70, 65, 0), (70, 1, NLEVELS - 1)):
        oct_ = rng.integers(1, NLEVELS - 1, N)
        oct_[r] = o
        pts.append(point(rng, cluster(rng, N), ref_obs=r, octave=oct_))
    return pts


def mixed(n_points, seed=9):
    """n_points points of mixed sizes: mostly short lists, every tenth long, some bad keyframes, a bad point and an empty list in
    between (workgroup tails, wave-to-point indexing)."""
    rng = np.random.default_rng(seed + n_points)
    pts = []
    for i in range(n_points):
        N = int(rng.integers(1, 12)) if i % 10 else int(rng.choice([63, 64, 65, 129, 256]))
        if n_points >= 5 and i == 3:
            N = 0
        pts.append(point(rng, cluster(rng, N) if N else np.zeros((0, 32), np.uint8), kf_bad=rng.random(N) < 0.15,
                         bad=(n_points >= 5 and i % 97 == 4)))
    return pts


ALL = dict(sized=sized, too_many=too_many, complementary=complementary, identical=identical, tied=tied, bad_keyframes=bad_keyframes,
           skipped=skipped, ref_octaves=ref_octaves)
