"""The cases of tests/match_cases.py without a GPU: for every case the oracle returns exactly the hand answer, and every claim is
real -- within each twin pair the two answers differ, and what the claim names (a descriptor distance, u, er, a bin, the bin counts,
a viewing cosine) is re-derived here and sits exactly on or beside its boundary.  The `crowd` case is checked for the path it is
there for: its window's grid entries and candidates against the limits of the kernels' key lists, read from their sources."""
import os
import re

import numpy as np
import pytest

import match_cases as MC
from match_cases import F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return MC.all_cases()


def _by_name(group, name):
    return next(c for c in group if c["name"] == name)


def _projection(oracle, c, check_ori=True):
    stereo = not c["mono"]
    return oracle.search_by_projection(c["kps"], c["desc"], MC.SF, MC.BOUNDS, MC.K, c["T_cur"], c["T_ref"], c["last"], th=MC.TH, mono=c["mono"],
                                       check_ori=check_ori, u_right=c["uright"] if stereo else None, mbf=MC.BF if stereo else 0.0,
                                       mb=MC.MB if stereo else 0.0)


def _local(oracle, c, th):
    return oracle.search_local_points(c["kps"], c["desc"], MC.SF, MC.LOG_SF, MC.BOUNDS, MC.K, MC.BF, c["T_cur"], c["pts"], th=th,
                                      nnratio=MC.NNRATIO, u_right=c["uright"], kp_claimed=c["kp_claimed"], cos_limit=MC.COS_LIMIT)


def _points(oracle, c, ori):
    return oracle.search_by_points(c["k1"], c["d1"], c["h1"], c["k2"], c["d2"], c["h2"], MC.NNRATIO_POINTS, ori)


def _dist(oracle, a, b):
    return oracle.descriptor_distance(a, b)


def _project(X):
    """u, v of a camera-frame point the way both matchers compute them (float32, one operation at a time)"""
    xc, yc, invz = F32(X[0]), F32(X[1]), F32(1.0 / X[2])
    return F32(F32(F32(MC.K[0]) * xc) * invz) + F32(MC.K[2]), F32(F32(F32(MC.K[1]) * yc) * invz) + F32(MC.K[3])


def _three_maxima(counts):
    """ComputeThreeMaxima on {bin: count} -> the bins that stay"""
    m, ind = [0, 0, 0], [-1, -1, -1]
    for i in range(30):
        s = counts.get(i, 0)
        if s > m[0]:
            m, ind = [s, m[0], m[1]], [i, ind[0], ind[1]]
        elif s > m[1]:
            m, ind = [m[0], s, m[1]], [ind[0], i, ind[1]]
        elif s > m[2]:
            m[2], ind[2] = s, i
    if F32(m[1]) < F32(0.1) * F32(m[0]):
        ind[1] = ind[2] = -1
    elif F32(m[2]) < F32(0.1) * F32(m[0]):
        ind[2] = -1
    return tuple(sorted(i for i in ind if i >= 0))


# ------------------------------------------------------------------------------------------------ the hand answers
def test_oracle_gives_the_hand_answers(oracle, cases):
    for c in cases["projection"] + cases["stereo"]:
        n, m = _projection(oracle, c)
        assert (n, m.tolist()) == (c["expect"]["n"], c["expect"]["match"]), c["name"]
    for c in cases["local"]:
        for th in MC.LOCAL_THS:
            r, e = _local(oracle, c, th), c["expect"][th]
            assert (r["n"], r["match"].tolist()) == (e["n"], e["match"]), (c["name"], th)
            assert r["in_view"].tolist() == e["in_view"] and r["level"].tolist() == e["level"], (c["name"], th)
    for c in cases["points"]:
        for ori in (True, False):
            n, m = _points(oracle, c, ori)
            assert (n, m.tolist()) == (c["expect"][ori]["n"], c["expect"][ori]["match"]), (c["name"], ori)


def test_every_claim_is_made_and_every_twin_differs(cases):
    want = dict(projection={"th_high", "ties", "window", "levels", "bounds", "claims", "rot_bins", "three_maxima", "sparse"},
                stereo={"stereo"}, local={"depth", "cand", "dist", "angle", "bounds", "predict_scale", "radius", "level_window", "th_high",
                                          "ratio", "claimed", "stereo"},
                points={"th_low", "ratio", "given_away", "flags", "rot_bins", "three_maxima"})
    for group, claims in want.items():
        assert set().union(*[c["claims"] for c in cases[group]]) == claims, group
    # both outcomes occur in every case with twins: a point that takes its keypoint, and one that a gate stops or the check cuts
    for c in cases["projection"] + cases["stereo"]:
        m = c["expect"]["match"]
        if c["name"].startswith("sparse") or c["name"] == "ties":
            continue
        assert any(v >= 0 for v in m) and c["expect"]["n"] < len(c["last"]["valid"]), c["name"]
    for c in cases["local"]:
        if c["name"] != "predict_scale":
            assert any(0 <= e["n"] < len(c["pts"]["cand"]) and any(v >= 0 for v in e["match"]) for e in c["expect"].values()), c["name"]
    for c in cases["points"]:
        if c["name"] != "single":
            assert 0 < c["expect"][True]["n"] < len(c["k1"]), c["name"]


# ------------------------------------------------------------------------------------------------ SearchByProjection
def test_projection_claims_sit_on_their_boundaries(oracle, cases):
    P = cases["projection"]
    c = _by_name(P, "th_high")
    d = [_dist(oracle, c["last"]["desc"][i], c["desc"][i]) for i in range(2)]
    assert d == [MC.TH_HIGH, MC.TH_HIGH + 1] and c["expect"]["match"] == [0, -1]

    c = _by_name(P, "ties")
    t, m, pd = c["ties"], c["expect"]["match"], c["last"]["desc"]
    for i, (win, lose) in enumerate((("early", "late"), ("first", "second"), ("near", "far"), ("high", "low"), ("left_down", "right_up"))):
        dw, dl = _dist(oracle, pd[i], c["desc"][t[win]]), _dist(oracle, pd[i], c["desc"][t[lose]])
        assert (dw < dl) if win == "near" else (dw == dl), win
        assert m[t[win]] == i and m[t[lose]] == -1
    cell = lambda k: (int(np.floor(F32(c["kps"]["x"][k] * F32(0.1)) + 0.5)), int(np.floor(F32(c["kps"]["y"][k] * F32(0.1)) + 0.5)))
    assert t["early"] > t["late"] and cell(t["early"])[0] < cell(t["late"])[0]                  # the larger index, walked first
    assert t["first"] < t["second"] and cell(t["first"]) == cell(t["second"])
    assert t["high"] > t["low"] and cell(t["high"])[0] == cell(t["low"])[0] and cell(t["high"])[1] < cell(t["low"])[1]
    assert t["left_down"] > t["right_up"] and cell(t["left_down"])[0] < cell(t["right_up"])[0] and cell(t["left_down"])[1] > cell(t["right_up"])[1]
    assert cell(t["far"])[0] < cell(t["near"])[0]

    c = _by_name(P, "window")
    uv = np.array([_project(X) for X in c["last"]["Xw"]])
    dx, dy = c["kps"]["x"] - uv[:, 0], c["kps"]["y"] - uv[:, 1]
    assert dx[:4].tolist() == [8.0, 7.5, 0.0, 0.0] and dy[:4].tolist() == [0.0, 0.0, 8.0, 7.5] and F32(MC.TH) * MC.SF[0] == 8.0
    assert c["r1"] == F32(9.600000381469727) and dx[4] == c["r1"] and dx[5] == np.nextafter(c["r1"], F32(0)) and dy[4] == dy[5] == 0
    assert c["expect"]["match"] == [-1, 1, -1, 3, -1, 5]

    c = _by_name(P, "bounds")
    uv = [_project(X) for X in c["last"]["Xw"][:8]]
    assert [float(u) for u, _ in uv[:4]] == [0.0, -2.0 ** -15, 640.0, float(np.nextafter(F32(640), F32(700)))]
    assert [float(v) for _, v in uv[4:]] == [0.0, -2.0 ** -16, 480.0, float(np.nextafter(F32(480), F32(500)))]
    assert c["last"]["Xw"][9, 2] == -2.0 and (c["last"]["Xw"][:, 2] != 0).all()
    assert [v >= 0 for v in c["expect"]["match"]] == [True, False] * 5

    c = _by_name(P, "levels")
    ok = [abs(int(o) - int(n)) <= 1 for o, n in zip(c["kps"]["octave"], c["last"]["octave"])]
    assert [v >= 0 for v in c["expect"]["match"]] == ok and ok == [False, True, True, True, False, True, True, False, True, True, False]

    c = _by_name(P, "claims")
    assert c["last"]["obs"].tolist() == [1, 1, 1, 1, 0, 1, 1] and c["expect"] == dict(match=[0, 1, 2, 5], n=5)
    assert [_dist(oracle, c["last"]["desc"][1], c["desc"][k]) for k in (0, 1)] == [2, 8]        # its first choice is the taken one


def _bins_of(la, ka, match):
    counts = {}
    for k, p in enumerate(match):
        if p >= 0:
            b = MC.rot_bin(F32(la[p]) - F32(ka[k]))
            counts[b] = counts.get(b, 0) + 1
    return counts


def test_rotation_claims(oracle, cases):
    f = MC.FACTOR
    assert F32(MC.ROT_BELOW * f) < 3.5 and F32(MC.ROT_ON * f) == 3.5 and F32(MC.ROT_ABOVE * f) > 3.5
    assert [MC.rot_bin(r) for r in (MC.ROT_BELOW, MC.ROT_ON, MC.ROT_ABOVE, 0.0, -10.0, 359.99)] == [3, 4, 4, 0, 12, 12]
    assert F32(0.1) * F32(20) == F32(2.0)                                   # max2 == 0.1f * max1 exactly
    for group, run in (("projection", lambda c: _projection(oracle, c, False)[1]), ("points", lambda c: _points(oracle, c, False)[1])):
        for c in cases[group]:
            if "bins" not in c:
                continue
            if group == "projection":
                counts = _bins_of(c["last"]["angle"], c["kps"]["angle"], run(c))
            else:
                m = run(c)
                counts = _bins_of(c["k1"]["angle"], c["k2"]["angle"], [int(np.flatnonzero(m == j)[0]) if (m == j).any() else -1
                                                                        for j in range(len(c["k2"]))])
            assert counts == c["bins"], (group, c["name"], counts)
            keep = _three_maxima(counts)
            if "keep" in c:
                assert keep == tuple(sorted(c["keep"])), c["name"]
            e = c["expect"] if group == "projection" else c["expect"][True]
            assert e["n"] == sum(v for b, v in counts.items() if b in keep), c["name"]
    assert _three_maxima(MC.ROT_BINS) == (0, 3, 5)


def test_stereo_claims(oracle, cases):
    S = cases["stereo"]
    c = _by_name(S, "stereo_gate")
    ur = np.array([_project(X)[0] - F32(MC.BF) * F32(0.5) for X in c["last"]["Xw"]], F32)
    er = np.abs(ur - c["uright"])
    assert er[0] == 8.0 and er[1] == np.nextafter(F32(8), F32(9)) and c["uright"][2:4].tolist() == [0.0, -1.0] and er[4] > 8
    assert [v >= 0 for v in c["expect"]["match"]] == [True, False, True, True, False]
    z = {c["name"]: c["tlc_z"] for c in S[1:]}
    assert z["stereo_forward"] > MC.MB == z["stereo_at_mb"] > z["stereo_below_mb"] > 0 > -MC.MB > z["stereo_backward"]
    assert z["stereo_forward"] - MC.MB == MC.MB - z["stereo_below_mb"] == MC.TLC_STEP
    got = {c["name"]: [v >= 0 for v in c["expect"]["match"]] for c in S[1:]}
    assert got == dict(stereo_forward=[True, False, True, False], stereo_at_mb=[False, False, True, True],
                       stereo_below_mb=[False, False, True, True], stereo_backward=[False, True, False, True])
    for c in S[1:]:
        assert ((c["last"]["Xw"] @ c["T_cur"][:3, :3].T + c["T_cur"][:3, 3])[:, 2] == 2.0).all()      # camera-frame depth exactly 2


def test_crowd_takes_the_slow_path(oracle, cases):
    c = cases["crowd"]
    lds = open(os.path.join(ROOT, "sdslam_amd", "csrc", "track_match_lds.h")).read()
    src = open(os.path.join(ROOT, "sdslam_amd", "csrc", "track_match.hip")).read()
    list_cap = int(re.search(r"#define MT_LIST_CAP (\d+)", lds).group(1))
    hbm_list = int(re.search(r"#define MT_HBM_LIST (\d+)", src).group(1))
    order_limit = int(re.search(r"seq >= (\d+)", src).group(1))
    max_kp = int(re.search(r"#define MT_MAXKP (\d+)", src).group(1))
    (u, v), r = c["centre"], c["radius"]
    cand = oracle.features_in_area(c["kps"], MC.BOUNDS, u, v, r, *c["levels"])
    entries = oracle.features_in_area(c["kps"], MC.BOUNDS, u, v, 1e3)            # every grid entry (all lie in the window's cells)
    cx = np.floor(c["kps"]["x"] * F32(0.1) + F32(0.5)).astype(int)
    cy = np.floor(c["kps"]["y"] * F32(0.1) + F32(0.5)).astype(int)
    lo, hi = int(np.floor((u - r) * 0.1)), int(np.ceil((u + r) * 0.1))
    assert ((cx >= lo) & (cx <= hi) & (cy >= lo) & (cy <= hi)).all() and len(entries) == len(c["kps"])
    m = len(c["last"]["valid"])
    print("crowd: %d grid entries, %d candidates per point, %d points; limits %d (LDS list) %d (HBM list) %d (order field)"
          % (len(entries), len(cand), m, list_cap, hbm_list, order_limit))
    assert len(cand) == len(c["kps"]) == 1500 and ((cx == 20) & (cy == 20)).sum() >= 1400
    assert len(c["kps"]) <= MC.CROWD_CAPACITY < max_kp and len(entries) < order_limit          # not the order-field word: the list-full one
    assert 2 * len(cand) <= list_cap < 3 * len(cand) and 5 * len(cand) <= hbm_list < 6 * len(cand) <= m * len(cand)
    n, match = _projection(oracle, c)
    taken = np.flatnonzero(match >= 0)
    assert n == m == len(taken) and sorted(match[taken].tolist()) == list(range(m))             # one keypoint each, all different
    d = [_dist(oracle, c["last"]["desc"][0], c["desc"][k]) for k in range(len(c["kps"]))]
    order = {int(k): i for i, k in enumerate(cand)}
    by_point = [int(np.flatnonzero(match == p)[0]) for p in range(m)]
    assert by_point == sorted(by_point, key=lambda k: (d[k], order[k])) and sum(x == 0 for x in d) > m   # each takes the first best one left


# ------------------------------------------------------------------------------------------------ the local-map search
def test_local_claims_sit_on_their_boundaries(oracle, cases):
    L = cases["local"]
    c = _by_name(L, "frustum")
    r = _local(oracle, c, 1.0)
    assert c["pts"]["Xw"][1, 2] == -2.0 and c["pts"]["cand"].tolist() == [1, 1, 0] + [1] * 6 and (c["pts"]["Xw"][:, 2] != 0).all()
    two = F32(2.0)
    assert (c["pts"]["min_dist"][3:5] == [two, np.nextafter(two, F32(3))]).all() and (c["pts"]["max_dist"][5:7] == [two, np.nextafter(two, F32(1))]).all()
    assert r["cos"][7] == F32(0.5) == F32(MC.COS_LIMIT) and F32(c["pts"]["normal"][8, 2]) == np.nextafter(F32(0.5), F32(0))
    assert r["in_view"].tolist() == [True, False, False, True, False, True, False, True, False]

    c = _by_name(L, "bounds")
    r = _local(oracle, c, 1.0)
    uv = [_project(X) for X in c["pts"]["Xw"]]
    assert [float(u) for u, _ in uv[:4]] == [640.0, float(np.nextafter(F32(640), F32(700))), 0.0, -2.0 ** -15]
    assert [float(v) for _, v in uv[4:]] == [480.0, float(np.nextafter(F32(480), F32(500))), 0.0, -2.0 ** -16]
    assert r["in_view"].tolist() == [True, False] * 4 and r["proj"][0, 0] == 640 and r["proj"][4, 1] == 480

    c = _by_name(L, "predict_scale")
    ratio = c["pts"]["mf_max_dist"] / np.array([F32(np.linalg.norm(X)) for X in c["pts"]["Xw"]], F32)
    assert c["expect"][1.0]["level"] == list(range(8)) + [0, 7] and ratio[0] < 1 and ratio[8] < 0.6 and ratio[9] > 1.2 ** 8
    assert np.allclose(np.log(ratio[:8]) / np.log(1.2), np.arange(8) - 0.5, atol=1e-4)

    c = _by_name(L, "radius")
    hi, lo = c["cos"]
    for th in MC.LOCAL_THS:
        r = _local(oracle, c, th)
        assert (np.abs(r["cos"][:4] / 0.998 - 1) < 2 * MC.COS_STEP).all() and ((r["cos"][:4] > 0.998) == [True, False, True, False]).all()
        assert r["in_view"].all() and r["level"].tolist() == [0] * 4 + [3] * 4
    off = np.abs(c["kps"]["x"][:4] - np.array([_project(X)[0] for X in c["pts"]["Xw"][:4]]))
    assert off.tolist() == [3, 3, 9, 9] and 2.5 < 3 < 4.0 and 3 * 2.5 < 9 < 3 * 4.0
    assert [c["expect"][1.0]["match"][k] >= 0 for k in range(4)] == [False, True, False, False]
    assert [c["expect"][3.0]["match"][k] >= 0 for k in range(4)] == [True, True, False, True]
    assert c["kps"]["octave"][4:].tolist() == [1, 2, 3, 4] and [v >= 0 for v in c["expect"][1.0]["match"][4:]] == [False, True, True, False]

    c = _by_name(L, "th_high")
    assert [_dist(oracle, c["pts"]["desc"][i], c["desc"][i]) for i in range(2)] == [100, 101]

    c = _by_name(L, "ratio")
    assert F32(MC.NNRATIO) * F32(50) == F32(40) and F32(MC.NNRATIO) * F32(40) == F32(32)
    k = 0
    for p, (cands, take) in enumerate(MC.RATIO_ROWS):
        got = [(_dist(oracle, c["pts"]["desc"][p], c["desc"][k + j]), int(c["kps"]["octave"][k + j])) for j in range(len(cands))]
        assert tuple(got) == cands and len({int(F32(x * F32(0.1)) + 0.5) for x in c["kps"]["x"][k:k + len(cands)]}) == 1     # one cell
        assert [c["expect"][1.0]["match"][k + j] for j in range(len(cands))] == [p if j == take else -1 for j in range(len(cands))]
        k += len(cands)
    assert [take is not None for _, take in MC.RATIO_ROWS] == [True, True, False, True, True, True, True, False]
    t, p = c["tie"], len(MC.RATIO_ROWS)
    assert t["early"] > t["late"] and c["kps"]["x"][t["early"]] * F32(0.1) < 6.5 < c["kps"]["x"][t["late"]] * F32(0.1)   # cells x = 6 and 7
    assert [_dist(oracle, c["pts"]["desc"][p], c["desc"][k]) for k in (t["early"], t["late"])] == [40, 40]
    assert c["expect"][1.0]["match"][t["early"]] == p and c["expect"][1.0]["match"][t["late"]] == -1

    c = _by_name(L, "claimed")
    assert c["kp_claimed"].tolist() == [1, 0, 0] and c["pts"]["obs"].tolist() == [1, 1, 1, 0, 1]
    assert c["expect"][1.0] == dict(match=[-1, 1, 4], n=3, in_view=[True] * 5, level=[2] * 5)

    c = _by_name(L, "stereo")
    r = _local(oracle, c, 1.0)
    er = np.abs(r["proj"][:, 2] - c["uright"])
    assert er[0] == 2.5 and er[1] == np.nextafter(F32(2.5), F32(3)) and er[2] == np.nextafter(F32(7.5), F32(8)) and c["uright"][3] == 0
    assert c["expect"][1.0]["match"] == [0, -1, -1, 3] and c["expect"][3.0]["match"] == [0, 1, -1, 3]


# ------------------------------------------------------------------------------------------------ SearchByPoints
def test_points_claims_sit_on_their_boundaries(oracle, cases):
    P = cases["points"]
    D = lambda c: np.array([[_dist(oracle, a, b) for b in c["d2"]] for a in c["d1"]])
    c = _by_name(P, "th_low")
    d = D(c)
    assert d[0, 0] == MC.TH_LOW - 1 and d[1, 1] == MC.TH_LOW and d[0, 1] > 80 and d[1, 0] > 80
    c = _by_name(P, "ratio")
    d = D(c)
    assert F32(MC.NNRATIO_POINTS) * F32(40) == F32(30)
    assert [sorted(d[i])[:3][:2] for i in range(3)] == [[30, 40], [29, 40], [30, 30]] and all(sorted(d[i])[2] > 80 for i in range(3))
    assert c["expect"][True]["match"] == [-1, 2, -1]
    c = _by_name(P, "single")
    assert len(c["k2"]) == 1 and D(c)[0, 0] == 49 and c["expect"][True]["match"] == [0]
    c = _by_name(P, "given_away")
    d = D(c)
    for i in range(6):
        assert sorted(np.argsort(d[i], kind="stable")[:4].tolist()) == [0, 1, 2, 3], i          # the same four nearest, for every row
    assert d[4].tolist()[:5] == [10, 10, 10, 10, 20] and d[5].tolist()[:5] == [60, 60, 60, 60, 70] and (d[:, 5:] >= MC.TH_LOW + 30).all()
    assert [d[i, i] for i in range(4)] == [2] * 4 and d[0, 1] == 18 and d[0, 4] == 28
    assert np.sort(d[5])[3] >= MC.TH_LOW                # its list of four ends beyond TH_LOW: nothing further can match
    assert c["expect"][True]["match"] == [0, 1, 2, 3, 4, -1]
    c = _by_name(P, "flags")
    d = D(c)
    assert c["h1"].tolist() == [0, 1, 1, 1] and c["h2"].tolist() == [1, 0, 1] and d[0, 0] == d[1, 1] == d[2, 2] == d[3, 0] == 0
    assert c["expect"][True]["match"] == [-1, -1, 2, 0]
