"""The problems of tests/align_cases.py without a GPU: every case does what its claim says, read from the oracle's per-iteration trace
(oracle.align(..., trace=True): the same ImageAlign struct with a report), and every case is certified -- the device forms H in
another order than the reference and sums it in a tree, so a case may only assert what survives both orders of forming H and five
re-orderings of its points, with every comparison a decision reads at least 1e-5 (relative) off equality.

Not forced, because nothing reaches it honestly: a level that runs all 30 iterations (200 seeded problems, the longest level took 10),
a NaN in x[0] (the pivoted LDLT of a finite H with the pseudo-inverse of D returns finite numbers, zeros for H = 0), and n_meas == 0 on
an iteration after the first of a level (the points measured before would all have to leave at once while chi2 fell)."""
import numpy as np
import pytest

import align_cases as AC
import geometries as G


@pytest.fixture(scope="module")
def cases(oracle):
    return AC.all_cases(oracle)


def pytest_generate_tests(metafunc):
    if "case_name" in metafunc.fixturenames:
        from oracle import oracle as O
        metafunc.parametrize("case_name", [c["name"] for c in AC.all_cases(O)])


def _level(r, level):
    return next(lv for lv in r["trace"] if lv["level"] == level)


def test_case_is_certified(oracle, case_name):
    c = AC.by_name(oracle, case_name)
    cert = AC.certify(oracle, c)
    r = cert["ref"]
    print(f"{c['name']}: mode {c['mode']} points {len(AC.taken(c))} ok {r['ok']} iters {r['iters'][2:5].tolist()} exits {[lv['exit'] for lv in r['trace']]} "
          f"pose spread {cert['spread']:.1e} margin {cert['margin']:.2e}")
    assert np.isfinite(c["Xw"]).all() and np.isfinite(c["T0"]).all() and len(AC.taken(c)) <= 300
    assert len(AC.taken(c)) <= 40 or c["group"] == "counts"
    assert cert["same"], "decisions depend on the order of the points or of forming H"
    assert cert["spread"] <= AC.CERT_TOL
    assert cert["margin"] >= AC.MARGIN
    plain = AC.solve(oracle, c, trace=False)                         # the traced entry is the plain one plus a report
    assert np.array_equal(plain["T"], r["T"]) and plain["ok"] == r["ok"] and np.array_equal(plain["iters"], r["iters"])
    assert plain["error"] == r["error"] and plain["chi2"] == r["chi2"]


def test_flags_are_the_clip_tests_restated(oracle, case_name):
    """has_jac is geometries.clip_visible at T_ref, measured is visible and clip_visible at the traced trial pose (plus uf, vf >= 0, which
    the border implies), visible is has_jac of this or an earlier level"""
    c = AC.by_name(oracle, case_name)
    r = AC.certify(oracle, c)["ref"]
    X, K = AC.taken(c), AC.camera(c["size"]).K
    seen = np.zeros(len(X), bool)
    for lv in r["trace"]:
        rows, cols = AC.level_shape(oracle, c, lv["level"])
        s = AC.level_scale(oracle, c, lv["level"])
        jac = G.clip_visible(X, c["T_ref"], K, s, cols, rows)
        seen |= jac
        for it in lv["its"]:
            assert np.array_equal(it["has_jac"], jac) and np.array_equal(it["visible"], seen), (c["name"], lv["level"])
            assert np.array_equal(it["measured"], seen & G.clip_visible(X, it["pose"], K, s, cols, rows)), (c["name"], lv["level"])
            assert it["n_meas"] == 16 * it["measured"].sum()


def test_noise_floor(oracle, cases):
    floor = max(AC.certify(oracle, c)["spread"] for c in cases)
    worst = max(cases, key=lambda c: AC.certify(oracle, c)["spread"])["name"]
    print(f"ImageAlign noise floor over H orders and point orders: {floor:.3e} ({worst}); recorded {AC.NOISE_FLOOR:.1e}")
    assert 0 < floor <= AC.NOISE_FLOOR <= AC.CERT_TOL


def test_same_image(oracle):
    r = AC.certify(oracle, AC.by_name(oracle, "same_image"))["ref"]
    assert r["ok"] and r["iters"][2:5].tolist() == [1, 1, 1] and r["chi2"] == 0.0 and r["error"] == 0.0
    for lv in r["trace"]:
        it = lv["its"][0]
        assert lv["exit"] == "converged" and it["chi2_sum"] == 0.0 and not it["x"].any() and it["measured"].all()
    assert np.array_equal(r["T"], np.eye(4))


def test_every_exit_at_every_level(oracle, cases):
    seen = {}
    for c in cases:
        for lv in AC.certify(oracle, c)["ref"]["trace"]:
            seen.setdefault((lv["level"], lv["exit"]), []).append(c["name"])
    print({k: v[:4] for k, v in sorted(seen.items())})
    for c in AC.exit_cases():
        r = AC.certify(oracle, c)["ref"]
        assert all(_level(r, l)["exit"] == e for l, e in c["exits"]), c["name"]
    named = {(l, e) for c in AC.exit_cases() for l, e in c["exits"]} | {(l, "converged") for l in (4, 3, 2)}
    for level in (4, 3, 2):
        for e in ("rollback_chi2", "small", "converged"):
            assert (level, e) in named and (level, e) in seen
    assert not any(e == "iterations" for _, e in seen)               # the 30-iteration exit: searched for, not reached (module docstring)
    assert max(max(AC.solve(oracle, AC.case("s", "exits", "", *AC.exit_problem(s)))["iters"]) for s in range(200)) < 30


def test_clip_cur_first(oracle):
    c = AC.by_name(oracle, "clip_cur_first")
    r = AC.certify(oracle, c)["ref"]
    n = 0
    for i, role in enumerate(c["roles"]):
        if role is None:
            continue
        level, side, measured = role
        it = _level(r, level)["its"][0]
        assert it["has_jac"][i] and it["measured"][i] == measured, (role, i)
        n += 1
    assert n == 24 and len(c["roles"]) == 40
    out = AC.taken_out(r)
    assert all(any(l == level and k == 0 and n_out >= 4 and acc for l, k, n_out, _, acc in out) for level in (4, 3, 2))


def test_clip_cur_later(oracle):
    r = AC.certify(oracle, AC.by_name(oracle, "clip_cur_later"))["ref"]
    leaves = enters = 0
    for lv in r["trace"]:
        for a, b in zip(lv["its"], lv["its"][1:]):
            if AC.accepted(b):
                leaves += int((a["measured"] & ~b["measured"] & b["has_jac"]).sum())
                enters += int((~a["measured"] & b["measured"] & b["has_jac"]).sum())
    print("clip_cur_later: points leaving on an accepted iteration", leaves, "entering", enters)
    assert leaves >= 1 and enters >= 1


@pytest.mark.parametrize("kind,n_out", [("few", 2), ("half", 20), ("most", 32)])
def test_clip_share(oracle, kind, n_out):
    c = AC.by_name(oracle, "clip_share_" + kind)
    out = AC.taken_out(AC.certify(oracle, c)["ref"])
    print(kind, out)
    assert len(AC.taken(c)) == 40
    assert any(n == n_out and jac == 40 and acc for _, _, n, jac, acc in out)
    assert all(n == n_out for l, _, n, _, _ in out if l == 4)


def test_sticky_and_late_visibility(oracle):
    c = AC.by_name(oracle, "sticky_stale_patch")
    assert AC.sticky_sizes()[0][:2] == (AC.STICKY_SIZE[0], AC.STICKY_LEVEL) and AC.sticky_sizes()[0][2] < AC.STICKY_U < AC.sticky_sizes()[0][3]
    r = AC.certify(oracle, c)["ref"]
    k = AC.N_STICKY
    for it in _level(r, AC.STICKY_LEVEL)["its"]:
        assert it["has_jac"][:k].all() and it["measured"][:k].all()
    fine = _level(r, AC.STICKY_LEVEL - 1)["its"]
    for it in fine:
        assert not it["has_jac"][:k].any() and it["visible"][:k].all() and it["measured"][:k].all() and it["has_jac"][k:].all()
    assert any(AC.accepted(it) for it in fine)
    c = AC.by_name(oracle, "late_visible")
    r = AC.certify(oracle, c)["ref"]
    for it in _level(r, 4)["its"]:
        assert not it["visible"][:6].any() and it["visible"][6:].all()
    for level in (3, 2):
        for it in _level(r, level)["its"]:
            assert it["has_jac"][:6].all() and it["measured"][:6].all()
    u, v, _ = AC.project(AC.taken(c)[:6], np.eye(4))
    assert all(5.2 < min(a, b) < 6.2 for a, b in zip(u, v))


def test_points_behind_the_camera(oracle):
    c = AC.by_name(oracle, "behind_ref")
    r = AC.certify(oracle, c)["ref"]
    z = AC.project(AC.taken(c), c["T_ref"])[2]
    assert (z[c["behind"]] < -1.0).all() and (z[~c["behind"]] > 1.0).all()
    for lv in r["trace"]:
        for it in lv["its"]:
            assert not it["visible"][c["behind"]].any() and it["measured"][~c["behind"]].all()
    c = AC.by_name(oracle, "behind_cur")
    r = AC.certify(oracle, c)["ref"]
    first = _level(r, 4)["its"][0]
    assert first["has_jac"][:4].all() and not first["measured"][:4].any() and AC.accepted(first)
    assert (AC.project(AC.taken(c)[:4], first["pose"])[2] < -0.1).all()
    for lv in r["trace"]:
        for it in lv["its"]:
            assert (np.abs(AC.project(AC.taken(c), it["pose"])[2]) >= 0.1).all()
    assert (AC.project(AC.taken(c), c["T_ref"])[2] >= 0.1).all()


def test_no_measurement(oracle):
    for c in AC.no_measurement_cases():
        r = AC.certify(oracle, c)["ref"]
        first = _level(r, 4)["its"][0]
        levels = 1 if c["mode"] in (2, 3) else 3                      # mode 2 leaves after level 4: error_ = 1e10 > 0.01
        assert first["n_meas"] == 0 and first["decision"] == "rollback_stop" and not first["x"].any(), c["name"]
        assert first["has_jac"].all() == c["has_jac"] and first["has_jac"].any() == c["has_jac"], c["name"]
        assert r["iters"][2:5].tolist() == ([1, 1, 1] if levels == 3 else [0, 0, 1]) and len(r["trace"]) == levels, c["name"]
        assert all(lv["exit"] == "rollback_stop" for lv in r["trace"])
        assert r["chi2"] == 1e10 and r["error"] == 1e10
        if c["mode"] == 0:
            assert r["ok"] and np.abs(r["T"] - (c["T0"] @ np.linalg.inv(c["T_ref"])) @ c["T_ref"]).max() <= 1e-15
        else:
            assert not r["ok"] and np.array_equal(r["T"], c["T0"])
    c = AC.by_name(oracle, "no_measurement_level4_only")
    r = AC.certify(oracle, c)["ref"]
    for level in (3, 2):                                             # everything could be measured: stop_ alone ends these levels
        it = _level(r, level)["its"][0]
        assert it["measured"].all() and it["has_jac"].all() and it["decision"] == "rollback_stop"


def test_gates(oracle):
    for c in AC.gate_cases():
        r = AC.certify(oracle, c)["ref"]
        g, thr = r["trace"][0]["gate"], 0.01 if c["mode"] == 2 else 0.03
        print(f"{c['name']}: error_ after level 4 = {g:.5f} against {thr}")
        assert abs(g - thr) / thr >= 1e-3 and (g > thr) == (c["side"] == "above") == (not r["ok"])
        assert len(r["trace"]) == (1 if c["mode"] == 3 or c["side"] == "above" else 3)
        if not r["ok"] or c["mode"] == 3:
            assert np.array_equal(r["T"], c["T0"])
        if not r["ok"]:
            assert r["error"] == 1e10


def test_counts(oracle):
    want = {"count_%d" % n: n for n in (3, 15, 16, 17, 64, 65)}
    want.update({"count_%d_m%d" % (n, m): 100 for n in (100, 101) for m in (2, 3)})
    want.update({"count_%d_m%d" % (n, m): 300 for n in (300, 301) for m in (0, 1)})
    want["tail_flags"] = 50
    cs = {c["name"]: c for c in AC.count_cases()}
    assert set(cs) == set(want)
    for name, n in want.items():
        c = cs[name]
        r = AC.certify(oracle, c)["ref"]
        assert len(AC.taken(c)) == n and r["ok"] and r["trace"][0]["its"][0]["n_meas"] == 16 * n, name
    for m in (2, 3):
        assert cs["count_101_m%d" % m]["n_valid"] == 101
    for m in (0, 1):
        a, b = cs["count_300_m%d" % m], cs["count_301_m%d" % m]
        for c in (a, b):
            assert c["n_last"] == 680 > 640 and len(c["valid"]) == 690 and c["valid"][680:].all()
        assert a["n_valid"] == 300 and np.flatnonzero(a["valid"][:680])[-1] >= 640
        idx = np.flatnonzero(b["valid"][:680])
        assert b["n_valid"] > 301 and 320 + 100 <= idx[299] < 640 - 100 and ((idx[300:] < 640).sum() >= 2) and ((idx[300:] >= 640).sum() >= 2)
    t = cs["tail_flags"]
    assert t["n_last"] == 50 and t["valid"][50:].all() and len(t["valid"]) == 120


def test_counterfactuals_are_noticed(oracle, cases):
    """One deliberately wrong oracle per quirk: which cases would fail on a device that got it wrong"""
    from oracle import oracle as O
    hits = {cf: [c["name"] for c in cases if AC.notices(oracle, c, cf)] for cf in O.ALIGN_COUNTERFACTUALS[1:]}
    for cf, names in hits.items():
        print(f"{cf:14s} {len(names):2d} {names}")
    for cf, names in hits.items():
        assert names, cf
    assert "sticky_stale_patch" in hits["reset_visible"] and "clip_share_most" in hits["keep_h"] and "clip_cur_later" in hits["stale_chi2"]
    assert "no_measurement_level4_only" in hits["clear_stop"] and "gate_m2_above" in hits["gate_last"] and "clip_cur_first" in hits["border2"]
    for c in cases:                                                  # the reference itself is no counterfactual
        assert not AC.notices(oracle, c, 0)


def test_oracle_call_does_not_depend_on_the_previous_one(oracle):
    a, b = AC.by_name(oracle, "clip_share_most"), AC.by_name(oracle, "no_measurement_behind_m0")
    ab = [AC.solve(oracle, c) for c in (a, b)]
    ba = [AC.solve(oracle, c) for c in (b, a)][::-1]
    for x, y in zip(ab, ba):
        assert np.array_equal(x["T"], y["T"]) and AC.decisions(x) == AC.decisions(y) and x["chi2"] == y["chi2"]
