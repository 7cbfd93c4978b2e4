"""CPU (no GPU): the restatement tests/cull_ref.py gives the hand answers of tests/cull_cases.py, and every case sits on its gate:
moving the gate's operand by one changes the stated output.  The same cases run on the device in tests/test_cull_gpu.py and
tests/test_erase_observations_gpu.py."""
import numpy as np
import pytest

import cull_cases as CC
import cull_ref as R

CASES = CC.cases()
ERASE = CC.erase_cases()


def run(c, **gates):
    return R.cull(c["q"], c["cand"], c["flags"], c["mono"], c["th"], **gates)


def stated(got, want):
    return {k: np.asarray(got[k]).tolist() for k in want}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_answers(name):
    c = CASES[name]
    assert c["want"], name
    got = run(c)
    want = {k: np.asarray(v).tolist() for k, v in c["want"].items()}
    assert stated(got, want) == want


# (case, the gate moved by one, the field that must change)
FLIPS = [
    ("observations_4", dict(th_obs=4), "verdict"),           # Observations() > 3 -> > 4: 4 is no longer enough
    ("observations_3", dict(th_obs=2), "verdict"),           # ... > 2, and two others are enough
    ("two_stereo_twin", dict(th_obs=4), "verdict"),          # three others are one too few
    ("own_entry_of_three", dict(th_obs=2), "verdict"),
    ("octave_plus_1", dict(oct_slack=0), "verdict"),
    ("octave_plus_2", dict(oct_slack=2), "verdict"),
    ("ratio_9_of_10", dict(ratio=0.9 - 1e-9), "verdict"),
    ("ratio_27_of_30", dict(ratio=0.9 - 1e-9), "verdict"),
    ("ratio_10_of_10", dict(ratio=1.0), "verdict"),
    ("ratio_19_of_20", dict(ratio=0.95), "verdict"),
    ("cascade_A_B", dict(bad_at=1), "verdict"),              # the shared points survive with nObs 2: B stays at 10 of 12
    ("list_empties", dict(bad_at=0), "point_bad"),
    ("points_1025", dict(bad_at=1), "point_bad"),
]


@pytest.mark.parametrize("name,gates,field", FLIPS)
def test_every_gate_sits_on_its_boundary(name, gates, field):
    c = CASES[name]
    assert field in c["want"]
    assert np.asarray(run(c, **gates)[field]).tolist() != np.asarray(c["want"][field]).tolist()


def test_depth_gate_twins():
    th = np.float32(CC.TH)
    assert np.float32(CC.ABOVE_TH) > th and np.nextafter(np.float32(CC.ABOVE_TH), np.float32(0)) == th
    at, above = CASES["depth_at_th"], CASES["depth_above_th"]
    assert run(at)["verdict"][0] == R.CULLED and run(above)["verdict"][0] == R.KEPT
    moved = dict(above, th=CC.ABOVE_TH)                                     # the threshold one float up: the point counts again
    assert run(moved)["verdict"][0] == R.CULLED
    assert run(CASES["depth_negative"])["counts2"].tolist() == [[0, 0]] and run(CASES["depth_negative_mono"])["counts2"].tolist() == [[1, 1]]


def test_order_of_the_candidates_decides():
    ab, ba = run(CASES["cascade_A_B"]), run(CASES["cascade_B_A"])
    assert ab["verdict"].tolist() == [R.CULLED, R.CULLED] and ba["verdict"].tolist() == [R.KEPT, R.CULLED]
    assert np.array_equal(CASES["cascade_A_B"]["q"]["kf"], CASES["cascade_B_A"]["q"]["kf"])          # the same data
    ne = run(CASES["not_erase"])
    assert not ne["obs_dead"].any() and not ne["point_bad"].any()


def test_flags_and_refusals():
    assert run(CASES["id0"])["verdict"][0] == R.SKIPPED_ID0 and run(dict(CASES["id0"], flags=np.array([0], np.uint8)))["verdict"][0] == R.CULLED
    for name, status in (("not_resident", R.NOT_RESIDENT), ("bad_index", R.BAD_INDEX)):
        got = run(CASES[name])
        assert got["info8"].tolist() == [status] + [0] * 7 and not got["obs_dead"].any() and not got["verdict"].any()
        assert run(CASES[name + "_bad_point"])["info8"][0] == R.OK


def test_random_maps_are_worth_running():
    for seed in range(3):
        c = CC.random_map(seed)
        got = run(c)
        assert got["info8"][0] == R.OK and got["info8"][1] >= 1 and (got["verdict"] == R.KEPT).any() and got["info8"][4] >= 1
        assert 3000 <= len(c["q"]["kf"]) <= 6000


@pytest.mark.parametrize("name", sorted(ERASE))
def test_erase_hand_answers(name):
    q, flags, want = ERASE[name]
    got = R.erase(q, flags)
    want = {k: np.asarray(v).tolist() for k, v in want.items()}
    assert want and stated(got, want) == want
    if name == "nothing":
        assert got["obs_off"].tolist() == q["off"].tolist() and got["ref_obs"].tolist() == q["ref_obs"].tolist()


def test_erase_gates_and_order():
    q, flags, _ = ERASE["leaves_2"]
    assert R.erase(q, flags, bad_at=1)["point_bad"].tolist() == [0, 0, 0]     # nObs <= 1: 2 survives
    q3, f3, _ = ERASE["leaves_3"]
    assert R.erase(q3, f3, bad_at=3)["point_bad"].tolist() == [0, 1, 0]
    # the order of the erasures does not matter: cull_ref walks the flags in entry order, here the list is reversed
    rng = np.random.default_rng(4)
    c = CC.random_map(7, n_kf=9, n_points=80, lo=2, hi=6)
    q = c["q"]
    flags = (rng.uniform(size=len(q["kf"])) < 0.3).astype(np.uint8)
    want = R.erase(q, flags)
    pts = [list(range(q["off"][p], q["off"][p + 1]))[::-1] for p in range(len(q["off"]) - 1)]
    perm = np.array([e for o in pts for e in o])
    qr = dict(q, kf=q["kf"][perm], octave=q["octave"][perm], stereo=q["stereo"][perm], depth=q["depth"][perm],
              ref_obs=np.diff(q["off"]) - 1 - q["ref_obs"])
    got = R.erase(qr, flags[perm])
    assert got["point_bad"].tolist() == want["point_bad"].tolist() and got["n_obs"].tolist() == want["n_obs"].tolist()
    assert got["obs_off"].tolist() == want["obs_off"].tolist() and want["info8"][2] >= 3
    # the mirror a caller keeps
    obs = [[(int(q["kf"][e]), e) for e in range(q["off"][p], q["off"][p + 1])] for p in range(len(q["off"]) - 1)]
    new, ro, pb = R.apply_erase(obs, q["ref_obs"], q["point_bad"], want)
    assert [len(o) for o in new] == np.diff(want["obs_off"]).tolist()
    assert [t[1] for o in new for t in o] == np.flatnonzero(want["obs_map"] >= 0).tolist()
