"""The problems of tests/poseopt_cases.py without a GPU: every case is what it claims (the hand answers of the gate, information and
uright groups are the oracle's; the oracle's per-round trace shows the round behaviour and the Levenberg exits claimed), and every
case is certified under re-ordering of its edges -- the device sums the edges in another order than g2o, so only what survives
re-ordering may be asserted on it.

LM exits: all four exits of optimize() (`nBad >= 3`, ten rejected trials, `rho == 0`, ten iterations used) and a rejected trial occur,
each in a count-stable case.  Two things a 400-problem search did NOT produce, and which are therefore not forced: an edge whose
FINAL flag depends on Huber being off in the fourth round, and a case that notices classification at the current estimate instead of
with the errors of the last computeActiveErrors (the only trials that leave foreign errors behind are the last ones of a `qmax` or
`rho == 0` exit, whose steps are below anything a threshold at 64 x margin can see)."""
import numpy as np
import pytest

import poseopt_cases as PC

CASES = PC.all_cases()
IDS = [c["name"] for c in CASES]
EXITS = ("nbad", "qmax", "rho_zero", "iterations")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_is_certified_under_reordering(oracle, c):
    cert = PC.certify(oracle, c)
    r = cert["ref"]
    print(f"{c['name']}: (n, bad, rounds, its, trials) = {tuple(int(v) for v in r['info'])} exits {r['round_exit']} pose spread "
          f"{cert['pose_spread']:.1e} chi2 margin {cert['chi2_margin']:.2e} vs spread {cert['chi2_spread']:.1e} "
          f"count-stable {cert['count_stable']}")
    assert np.isfinite(c["Xw"]).all() and np.isfinite(c["uright"]).all() and np.isfinite(c["T0"]).all()
    assert cert["flags_stable"]
    assert cert["pose_spread"] <= PC.POSE_TOL / PC.MARGIN
    assert cert["chi2_ok"], (cert["chi2_margin"], cert["chi2_spread"])
    assert not r["outlier"][~c["has"]].any() and not r["round_outlier"][:, ~c["has"]].any()
    plain = PC.solve(oracle, c, trace=False)                          # the traced entry is the plain one plus a report
    assert np.array_equal(plain["T"], r["T"]) and np.array_equal(plain["outlier"], r["outlier"]) and np.array_equal(plain["info"], r["info"])


@pytest.mark.parametrize("c", [c for c in CASES if c["expect"]], ids=[c["name"] for c in CASES if c["expect"]])
def test_hand_answers_are_the_oracles(oracle, c):
    r, e = PC.certify(oracle, c)["ref"], c["expect"]
    assert np.array_equal(r["outlier"], e["outlier"]), (np.flatnonzero(r["outlier"]), np.flatnonzero(e["outlier"]))
    assert (r["info"][0], r["info"][2], r["n_inliers"], r["info"][1]) == (e["n"], e["rounds"], e["n_inliers"], int(e["outlier"].sum()))
    if e["untouched"]:
        assert np.array_equal(r["T"], c["T0"]) and r["info"][3] == r["info"][4] == 0
    else:
        assert not np.array_equal(r["T"], c["T0"])


def test_gate_twins(oracle):
    nine, ten = PC.by_name("gate_9"), PC.by_name("gate_10")
    extra = np.flatnonzero(ten["has"] & ~nine["has"])
    assert len(extra) == 1 and nine["has"].sum() == 9 and np.array_equal(nine["kps"], ten["kps"]) and np.array_equal(nine["Xw"], ten["Xw"])
    r9, r10 = PC.certify(oracle, nine)["ref"], PC.certify(oracle, ten)["ref"]
    assert r9["info"][2] == 1 and r10["info"][2] == 4 and not r10["outlier"][extra[0]]
    assert PC.notices(oracle, ten, "gate_le10") and not PC.notices(oracle, nine, "gate_le10")


def test_probes_sit_where_they_claim(oracle):
    """chi2 of every probe edge at the final classification against its hand value invSigma2 * |residual|^2: the pinned pose gives
    way by less than a tenth of the distance to the threshold"""
    c = PC.by_name("info_twins")
    r = PC.certify(oracle, c)["ref"]
    for name, octave, stereo, res, outl in PC.PROBES:
        i = c["probes"][name]
        want = float(PC.INV_SIGMA2[octave]) * sum(x * x for x in res)
        thr = float(PC.CHI2_STEREO if stereo else PC.CHI2_MONO)
        print(f"{name}: chi2 {r['chi2'][i]:.4f}, by hand {want:.4f}, threshold {thr}")
        assert (want > thr) == outl == bool(r["outlier"][i])
        assert (c["uright"][i] >= 0) == stereo and c["kps"]["octave"][i] == octave
        assert abs(r["chi2"][i] - want) <= 0.5 * abs(want - thr)
    assert r["outlier"][c["probes"]["between_mono"]] and not r["outlier"][c["probes"]["between_stereo"]]
    assert r["outlier"][c["probes"]["sum_stereo"]] and not r["outlier"][c["probes"]["sum_mono"]]


def test_uright_forms():
    c = PC.by_name("uright_bf40")
    ur = c["uright"]
    assert ur[11] == 0 and not np.signbit(ur[11]) and ur[20] == 0 and np.signbit(ur[20]) and ur[6] == -1 and ur[27] == 0 and np.signbit(ur[34])
    stereo = ~(ur < 0)
    assert stereo[[11, 20, 27, 34]].all() and not stereo[[6, 41]].any() and 20 < stereo.sum() < 44         # interleaved in one window
    z = PC.by_name("uright_bf0")
    assert z["bf"] == 0.0 and (z["uright"][[7, 21, 35, 49]] > 0).all()


def test_round_claims(oracle):
    ro = {k: PC.certify(oracle, PC.by_name(k))["ref"] for k in ("all_outliers", "readmitted", "late_outlier", "huber_rounds", "behind")}
    a, ca = ro["all_outliers"], PC.by_name("all_outliers")
    assert a["round_outlier"].all() and a["round_exit"][1:] == ["not_run"] * 3 and a["round_its"][1:].tolist() == [0, 0, 0] and a["info"][2] == 4
    assert np.abs(a["T"] - PC.quaternion_round_trip(ca["T0"])).max() <= 4e-16 and np.abs(a["T"] - ca["T0"]).max() <= 1e-14
    for name, early in (("readmitted", True), ("huber_rounds", True)):
        r = ro[name]
        assert (r["round_outlier"][:3].any(0) & ~r["outlier"]).any(), name               # flagged in an early round, clear at the end
    for name in ("late_outlier", "huber_rounds"):
        r = ro[name]
        assert (~r["round_outlier"][0] & r["outlier"] & PC.by_name(name)["has"]).any(), name
    c = PC.by_name("huber_rounds")
    assert PC.notices(oracle, c, "huber_off_early") and PC.notices(oracle, c, "huber_round4")
    b, cb = ro["behind"], PC.by_name("behind")
    i = cb["behind"]
    for T in (cb["T0"], PC.T_TRUE, b["T"]):
        assert (T[:3, :3] @ cb["Xw"][i] + T[:3, 3])[2] < -1.0
    assert b["round_outlier"][:, i].all() and b["outlier"].sum() == 1


def test_lm_exits_and_rejected_trials(oracle):
    seen = {e: [] for e in EXITS}
    for c in CASES:
        cert = PC.certify(oracle, c)
        for e in set(cert["ref"]["round_exit"]) - {"not_run"}:
            seen[e].append((c["name"], cert["count_stable"]))
    print({e: [n for n, st in v if st] for e, v in seen.items()})
    for e in EXITS:
        assert any(st for _, st in seen[e]), e                       # every exit in some count-stable case
    for c in PC.lm_cases():
        r = PC.certify(oracle, c)["ref"]
        assert c["exit"] in r["round_exit"], (c["name"], r["round_exit"])
    far = [PC.certify(oracle, c)["ref"] for c in PC.lm_cases() if c["name"].startswith("far")]
    assert all(r["info"][4] > r["info"][3] for r in far)             # rejected trials
    for c in PC.lm_cases():
        if c["name"].startswith("far"):
            d = c["T0"] @ np.linalg.inv(PC.T_TRUE)
            ang = np.degrees(np.arccos((np.trace(d[:3, :3]) - 1) / 2))
            assert 20.0 - 1e-9 <= ang <= 40.0 + 1e-9 and np.linalg.norm(d[:3, 3]) >= 0.1
        if c["name"].startswith("truth"):
            assert np.array_equal(c["T0"], PC.T_TRUE)


def test_count_stable_cases_exist_in_every_group(oracle):
    stable = {}
    for c in CASES:
        stable.setdefault(c["group"], []).append(c["name"]) if PC.certify(oracle, c)["count_stable"] else None
    print(stable)
    for g in ("gates", "lists", "rounds", "lm"):
        assert any(PC.certify(oracle, PC.by_name(n))["ref"]["info"][2] > 0 for n in stable.get(g, [])), g


def test_counterfactuals_are_noticed(oracle):
    """One deliberately wrong oracle per quirk: which cases would fail on a device that got it wrong.  `classify_at_est` is
    reported, not asserted (see the module docstring)."""
    from oracle import oracle as O
    hits = {cf: [c["name"] for c in CASES if PC.notices(oracle, c, cf)] for cf in O.COUNTERFACTUALS[1:]}
    for cf, names in hits.items():
        print(cf, len(names), names[:6])
    for cf in ("huber_off_early", "huber_round4", "no_restart", "stereo_delta", "gate_le10"):
        assert hits[cf], cf
    assert "gate_9" in hits["stereo_delta"]                          # one Huber round only: the pose itself carries the delta


def test_oracle_call_does_not_depend_on_the_previous_one(oracle):
    """_solver->x() used to be a static of the oracle: a failed first solve would have read the previous problem's step"""
    a, b = PC.by_name("far_qmax"), PC.by_name("noisy_nbad")
    ab = [PC.solve(oracle, c) for c in (a, b)]
    ba = [PC.solve(oracle, c) for c in (b, a)][::-1]
    for x, y in zip(ab, ba):
        assert np.array_equal(x["T"], y["T"]) and np.array_equal(x["round_outlier"], y["round_outlier"]) and PC.counts(x) == PC.counts(y)
        assert np.array_equal(x["chi2"], y["chi2"])
