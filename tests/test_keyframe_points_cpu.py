"""CPU (no GPU): known-answer tests of the numpy restatement the GPU tests compare the device against
(tests/keyframe_points_ref.py: CreateNewKeyFrame's RGB-D loop, StereoInitialization, UnprojectStereo, NeedNewKeyFrame), and
the new entry points: declared in the C ABI, exported, bound in Python, refusing a NULL handle."""
import os
import re

import numpy as np
import pytest

import keyframe_points_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1000
TH = np.float32(2.0)
NEW_CALLS = ("sd_track_set_next_map_id", "sd_track_stereo_init", "sd_track_set_keyframe_state", "sd_track_need_keyframe",
             "sd_track_set_keyframe_flags", "sd_track_get_keyframe_flags", "sd_track_create_keyframe_points", "sd_track_get_created")


def run(depth, match=None, last_obs=None, th=TH):
    depth = np.asarray(depth, np.float32)
    n = len(depth)
    match = np.full(n, -1, np.int32) if match is None else np.asarray(match, np.int32)
    last_obs = np.ones(M, np.int32) if last_obs is None else last_obs
    return R.create_new_keyframe(depth, th, match, M, last_obs, np.zeros(M, np.int32))


def test_a_many_close_points_end_at_first_far_point_past_100():
    depth = np.concatenate([np.linspace(1.0, 1.9, 150), np.linspace(2.1, 3.0, 50)]).astype(np.float32)
    created, P, cand = run(depth[::-1])                     # reversed: the sort decides, not the index
    assert (P, cand) == (151, 200)
    assert created == [199 - j for j in range(151)]


def test_b_few_close_points_take_the_100_closest_plus_one():
    depth = np.concatenate([np.linspace(1.0, 1.9, 30), np.linspace(2.1, 3.0, 170)]).astype(np.float32)
    created, P, cand = run(depth)
    assert (P, cand) == (101, 200) and created == list(range(101))


def test_c_fewer_than_101_candidates_are_all_processed():
    depth = np.linspace(2.5, 3.0, 100).astype(np.float32)   # all far: nPoints never exceeds 100
    created, P, cand = run(depth)
    assert (P, cand) == (100, 100) and created == list(range(100))
    assert run(np.zeros(50, np.float32)) == ([], 0, 0)


def test_d_a_point_at_exactly_th_depth_does_not_end_the_loop():
    depth = np.concatenate([np.linspace(1.0, 1.9, 120), [2.0, 2.0, 2.5, 2.6]]).astype(np.float32)
    _, P, _ = run(depth)
    assert P == 123                                          # both 2.0 entries pass; 2.5 ends it
    assert R.prefix_closed_form(depth, TH) == 123


def test_e_equal_depths_are_ordered_by_index():
    depth = np.full(150, 2.5, np.float32)
    created, P, _ = run(depth)
    assert P == 101 and created == list(range(101))
    depth[:3] = [1.5, 1.5, 1.5]
    created, _, _ = run(depth[::-1])
    assert created[:3] == [147, 148, 149]


def test_f_obs0_point_is_replaced_inside_the_prefix_only():
    depth = np.linspace(2.1, 3.0, 150).astype(np.float32)   # P = 101
    match = np.arange(150, dtype=np.int32)
    obs = np.ones(M, np.int32)
    obs[[5, 120]] = 0
    created, P, _ = run(depth, match, obs)
    assert P == 101 and created == [5]                       # 120 holds an Observations() < 1 point too, outside the prefix
    # a local-map point (m >= M) with Observations() < 1
    match[7] = M + 3
    created, _, _ = R.create_new_keyframe(depth, TH, match, M, obs, np.zeros(M, np.int32))
    assert created == [5, 7]


def test_g_a_kept_point_flagged_outlier_is_not_replaced():
    """The restatement takes no outlier flags at all: :861-867 run before the discard of :272-275."""
    depth = np.linspace(1.0, 1.5, 20).astype(np.float32)
    match = np.full(20, -1, np.int32)
    match[4] = 9                                             # Observations() = 1, whatever mvbOutlier[4] says
    created, _, _ = run(depth, match)
    assert 4 not in created and len(created) == 19
    assert "outlier" not in R.create_new_keyframe.__code__.co_varnames


def test_h_nan_zero_and_negative_depths_are_no_candidates():
    depth = np.array([1.0, np.nan, 0.0, -1.0, 1.2, -0.0, np.inf], np.float32)
    created, P, cand = run(depth)
    assert created == [0, 4, 6] and (P, cand) == (3, 3)
    assert R.stereo_initialization(depth, min_keypoints=3) == [0, 4, 6]
    assert R.stereo_initialization(depth, min_keypoints=7) is None     # N > min_keypoints is strict


def test_i_closed_form_prefix_equals_the_serial_loop():
    rng = np.random.Generator(np.random.PCG64(7))
    for case in range(1000):
        n = int(rng.integers(0, 400))
        depth = rng.uniform(1.6, 2.4, n).astype(np.float32)
        depth[rng.random(n) < rng.uniform(0, 0.6)] = 0.0
        if case % 3 == 0:
            depth = np.round(depth * 8) / np.float32(8)      # many ties, some exactly at the threshold
        th = np.float32(rng.choice([1.5, 1.75, 2.0, 2.125, 2.5]))
        match = rng.integers(-1, 50, n).astype(np.int32)
        obs = rng.integers(0, 2, M).astype(np.int32)
        _, P, cand = R.create_new_keyframe(depth, th, match, M, obs, obs)
        assert P == R.prefix_closed_form(depth, th), case
        assert cand == int((depth > 0).sum())


def test_unproject_stereo_order():
    K = (520.9, 521.0, 325.1, 249.7)
    assert np.array_equal(R.unproject_stereo(400.5, 100.25, 2.0, K, np.eye(4)),
                          [np.float32(400.5 - np.float32(325.1)) * np.float32(2.0) * (np.float32(1) / np.float32(520.9)),
                           np.float32(100.25 - np.float32(249.7)) * np.float32(2.0) * (np.float32(1) / np.float32(521.0)), 2.0])
    from sdslam_amd import synth
    T = synth.se3_exp((0.1, -0.2, 0.05), (0.3, -0.1, 0.2))
    X = R.unproject_stereo(400.5, 100.25, 2.0, K, T)
    xc = T[:3, :3] @ X + T[:3, 3]                            # back into the camera frame
    assert abs(xc[2] - 2.0) < 1e-12 and abs(xc[0] / xc[2] * 520.9 + 325.1 - 400.5) < 1e-3


def nk(inl, tc, ntc, state, rgbd=1, fid=100, mn=0, mx=30, tracked=True):
    return R.need_new_keyframe(tracked, inl, tc, ntc, state, rgbd, fid, mn, mx)


def test_need_new_keyframe_conditions():
    IDLE, STOP, Q3 = 1, 2, 4
    # c1a: MaxFrames passed; c2 by the float ratio (100 < 200 * 0.75)
    assert nk(100, 150, 0, (5, 200, 70, 0, 0), mn=50) == 2           # mapper busy, queue full: wanted only
    assert nk(100, 150, 0, (5, 200, 70, 0, Q3), mn=50) == 3          # KeyframesInQueue() < 3: inserted all the same
    assert nk(100, 150, 0, (5, 200, 70, 0, Q3), mn=50, rgbd=0) == 2  # not RGB-D: never with a busy mapper
    assert nk(100, 150, 0, (5, 200, 70, 0, IDLE), mn=50) == 1
    assert nk(100, 150, 0, (5, 200, 71, 0, 0), mn=50) == 0           # c1a fails (100 < 71 + 30), not idle: c1b fails
    # c1b: MinFrames passed and idle
    assert nk(100, 150, 0, (5, 200, 95, 0, IDLE), mn=5) == 1
    assert nk(100, 150, 0, (5, 200, 96, 0, IDLE), mn=5) == 0
    # c1c through the double comparison, c2 through the float one: inliers 49 < 200 * 0.25
    assert nk(49, 150, 0, (5, 200, 99, 0, IDLE), mn=50) == 1
    assert nk(50, 150, 0, (5, 200, 99, 0, IDLE), mn=50) == 0
    # c1c / c2 through bNeedToInsertClose (strict on both sides)
    assert nk(190, 99, 71, (5, 200, 99, 0, IDLE), mn=50) == 1
    assert nk(190, 100, 71, (5, 200, 99, 0, IDLE), mn=50) == 0
    assert nk(190, 99, 70, (5, 200, 99, 0, IDLE), mn=50) == 0
    assert nk(190, 99, 71, (5, 200, 99, 0, IDLE), mn=50, rgbd=0) == 0   # the counts are RGB-D only
    # c2 needs more than 15 inliers
    assert nk(15, 0, 100, (5, 200, 0, 0, IDLE)) == 0
    assert nk(16, 0, 100, (5, 200, 0, 0, IDLE)) == 1
    # thRefRatio: 0.4f below two keyframes, 0.9f when not RGB-D
    assert nk(79, 150, 0, (1, 200, 0, 0, IDLE)) == 1 and nk(80, 150, 0, (1, 200, 0, 0, IDLE)) == 0
    assert nk(179, 0, 0, (5, 200, 0, 0, IDLE), rgbd=0) == 1 and nk(180, 0, 0, (5, 200, 0, 0, IDLE), rgbd=0) == 0
    # mapper stopped; too soon after a relocalisation (only with more than MaxFrames keyframes); not tracked
    assert nk(100, 150, 0, (5, 200, 0, 0, IDLE | STOP)) == 0
    assert nk(100, 150, 0, (31, 200, 0, 80, IDLE)) == 0 and nk(100, 150, 0, (30, 200, 0, 80, IDLE)) == 1
    assert nk(100, 150, 0, (5, 200, 0, 0, IDLE), tracked=False) == 0


def test_need_new_keyframe_float_and_double_comparisons_differ():
    """nRefMatches * 0.4f: in float 25 * 0.4f rounds to 10.0 (10 < 10 false); in double 25 * (double)0.4f = 10.00000015 would
    be true.  nRefMatches * 0.25 in double is exact either way, so pin the float side against the double one directly."""
    assert np.float32(25) * np.float32(0.4) == np.float32(10) and 25 * float(np.float32(0.4)) > 10
    assert nk(10, 150, 0, (1, 25, 0, 0, 1)) == 0            # c2 false in float (and 10 > 15 is false anyway) ...
    # ... a case with more than 15 inliers: 40 * 0.4f = 16.000000238 in double, 16.0 in float
    assert np.float32(40) * np.float32(0.4) == np.float32(16) and 40 * float(np.float32(0.4)) > 16
    assert nk(16, 150, 0, (1, 40, 0, 0, 1)) == 0            # float: 16 < 16.0 false; a double product would say true
    # 0.75f is exact; 0.9f: 20 * 0.9f = 18.0 in float, 17.99999952 in double
    assert np.float32(20) * np.float32(0.9) == np.float32(18) and 20 * float(np.float32(0.9)) < 18
    assert nk(17, 0, 0, (5, 20, 0, 0, 1), rgbd=0) == 1
    # the 0.25 comparison is in double: 2^24 + 1 inliers against nRefMatches = 4 * (2^24 + 1) + 3 -- as floats the inliers
    # round down to 2^24 and nRefMatches * 0.25 rounds to 2^24 + 2
    inl, ref = 2 ** 24 + 1, 4 * (2 ** 24 + 1) + 3
    assert float(inl) < ref * 0.25 and nk(inl, 150, 0, (5, ref, 99, 0, 1), mn=50) == 1
    assert nk(inl, 150, 0, (5, 4 * inl, 99, 0, 1), mn=50) == 0          # equal in double: c1c false, nothing else holds


def test_handoff_carries_created_points_over_outlier_flags():
    kps = np.zeros(4, [("octave", "<i4"), ("angle", "<f4")])
    kps["octave"] = [0, 1, 2, 3]
    last = dict(Xw=np.arange(12.0).reshape(4, 3), desc=np.full((4, 32), 7, np.uint8), obs=np.array([1, 0, 2, 1], np.int32))
    ids = np.array([10, 11, 12, 13], np.int32)
    cur_desc = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    created = dict(kp_index=[1, 3], Xw=np.array([[1.0, 2, 3], [4, 5, 6]]), ids=[50, 51])
    h = R.handoff(8, kps, 4, np.array([0, 1, 2, -1]), np.array([0, 1, 1, 1], bool), last, ids, None, None, created, cur_desc)
    assert h["valid"][:4].tolist() == [1, 1, 0, 1] and h["ids"][:4].tolist() == [10, 50, -1, 51]
    assert np.array_equal(h["desc"][1], cur_desc[1]) and h["obs"][:4].tolist() == [1, 1, 0, 1]
    assert np.array_equal(h["Xw"][3], [4, 5, 6]) and h["octave"][:4].tolist() == [0, 1, 2, 3]
    h = R.handoff(8, kps, 4, None, None, None, None, None, None, created, cur_desc)            # after StereoInitialization
    assert h["valid"][:4].tolist() == [0, 1, 0, 1]


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return sdslam_amd


def test_new_calls_declared_exported_and_bound(sd):
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    L = sd.lib()
    for name in NEW_CALLS:
        assert re.search(rf"^int {name}\(sd_track\* h,", hdr, re.M), name
        assert hasattr(L, name), name
        assert callable(getattr(sd.Tracker, name[len("sd_track_"):])), name
    assert re.search(r"^#define SD_KF_KEEP INT32_MIN\b", hdr, re.M) and sd.Tracker.KF_KEEP == -2 ** 31


def test_new_calls_refuse_a_null_handle(sd):
    L = sd.lib()
    protos = {"sd_track_set_next_map_id": (None, 0, 1, None), "sd_track_stereo_init": (None, 1, 500),
              "sd_track_set_keyframe_state": (None, 0, 1, None),
              "sd_track_need_keyframe": (None, 1, 1, 0, 0, 30),
              "sd_track_set_keyframe_flags": (None, 0, 1, None),
              "sd_track_get_keyframe_flags": (None, 0, 1, None),
              "sd_track_create_keyframe_points": (None, 1, 1, 2.0, 0, 0),
              "sd_track_get_created": (None, 0, 1, None, None, None, None, 0)}
    assert set(protos) == set(NEW_CALLS)
    for name, args in protos.items():
        assert getattr(L, name)(*args) == 1, name


def test_oracle_odometry_loop_sustains_itself(oracle):
    """The oracle-only RGB-D odometry loop of tests/keyframe_loop.py (2 streams x 12 frames from StereoInitialization on frame
    0, TrackWithMotionModel + TrackLocalMap with an empty local map + the restatement): every stream stays tracked, keyframes
    are inserted at frames 3, 6 and 9, and creation branch (a) is taken.  Measured here, on the oracle: the largest
    translation error against seq["T"] is 4.01e-3 m, so the bound is 9e-3 (twice that, rounded up to one digit).
    Branch (f) cannot occur in this loop, and is not asserted: every point the loop holds was created by it with
    Observations() = 1, and nothing within its scope lowers that count (LocalMapping's culling and the temporal VO points of
    UpdateLastFrame stay with the caller); the GPU creation test takes (f) on a static map instead.
    sd_track_local_map with n_local = 0 is usable: the local search finds nothing and PoseOptimization runs on the frame
    matches, which is what the oracle's track_local_map does with empty arrays."""
    import keyframe_loop as KL
    seqs, views, depth = KL.sequences()
    rec = KL.oracle_loop(oracle, seqs, views, depth, [0, 100000])
    worst, branches = 0.0, set()
    for b, rs in enumerate(rec):
        assert len(rs) == KL.T_FRAMES >= 12 and len(rs[0]["created"]) > 500
        assert [t for t in range(1, len(rs)) if rs[t]["flag"] & 1] == [3, 6, 9], b
        for t in range(1, len(rs)):
            r = rs[t]
            assert (r["status_mm"], r["status"]) == (2, 2), (b, t)
            worst = max(worst, float(np.abs(r["T"][:3, 3] - seqs[b]["T"][t][:3, 3]).max()))
            if r["flag"] & 1:
                assert len(r["created"]) > 100 and r["ids"][0] == rs[0]["ids"][-1] + 1 + sum(len(rs[k]["created"]) for k in range(1, t))
                if r["n_close"] >= 100 and r["P"] == r["n_close"] + 1 < r["candidates"]:
                    branches.add("a")
            else:
                assert r["created"] == []
    print("largest translation error of the oracle loop:", worst)
    assert worst <= 9e-3, worst
    assert "a" in branches
