"""sd_track_global_ba (sdslam_amd/csrc/track_ba.hip) on the MI355X against the numpy restatement tests/gba_ref.py.

The blocked LDL^T alone through sd_debug_ldlt against ba_ref.ldlt_solve within gba_cases.SOLVER_BOUND, the zero pivots, two runs with
the same bytes.  The whole call through sd_debug_global_ba: every run of gba_cases.RUNS -- info16 and point_status equal, poses and
points within gba_cases.GPU_BOUND -- the refusals, determinism.  With a tracker on planted keyframes: the resident path equals the
debug entry byte for byte, write_back = 0 changes nothing, write_back = 1 leaves the getter's values, the getter fails after
sd_track_set_poses, and neither getter answers the other kind of run."""
import numpy as np
import pytest

import ba_ref
import gba_cases as G
import gba_ref
import test_local_ba_gpu as LB

pytestmark = pytest.mark.gpu
B = LB.B
_WANT = {}


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def want(name):
    if name not in _WANT:
        _, nit, robust = G.RUNS[name]
        _WANT[name] = gba_ref.run(G.problem(name), nit, robust)
    return _WANT[name]


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in ("T", "Xw", "point_status", "info16"))


# ------------------------------------------------------------------------------------------------ the solver alone
@pytest.mark.parametrize("n", G.SOLVER_SIZES)
def test_ldlt_against_the_unblocked_one(sd, n):
    from sdslam_amd import capi
    A, b = G.spd(n, n)
    ok_ref, x_ref = ba_ref.ldlt_solve(A, b)
    ok, x = capi.debug_ldlt(A, b)
    dev = np.abs(x - x_ref).max() / np.abs(x_ref).max()
    print(f"n = {n}: relative deviation {dev:.3e} (bound {G.SOLVER_BOUND:.1e})")
    assert ok_ref and ok
    assert dev <= G.SOLVER_BOUND
    if n in (198, 390):
        ok2, x2 = capi.debug_ldlt(A, b)
        assert ok2 and np.array_equal(x.view(np.uint8), x2.view(np.uint8))


@pytest.mark.parametrize("panel", [0, 1])
def test_ldlt_zero_pivot(sd, panel):
    from sdslam_amd import capi
    A, b, at = G.zero_pivot(panel)
    assert ba_ref.ldlt_solve(A, b) == (False, None) and at // gba_ref.PANEL == panel
    assert ba_ref.ldlt_solve(A[:at, :at], b[:at])[0]                       # ... and no pivot before it
    ok, x = capi.debug_ldlt(A, b)
    assert not ok and not x.any()


# ------------------------------------------------------------------------------------------------ the whole call
@pytest.mark.parametrize("name", list(G.RUNS))
def test_debug_entry_against_the_restatement(sd, name):
    from sdslam_amd import capi
    _, nit, robust = G.RUNS[name]
    p, w = G.problem(name), want(name)
    got = capi.debug_global_ba(p, nit, robust)
    dev = max(np.abs(got["T"] - w["T"]).max(), np.abs(got["Xw"] - w["Xw"]).max())
    print(f"{name}: info16 {got['info16'][:9].tolist()} deviation {dev:.3e} (bound {G.GPU_BOUND:.1e})")
    assert got["info16"].tolist() == w["info16"].tolist() and got["info16"][0] == 0
    assert np.array_equal(got["point_status"], w["point_status"])
    assert dev <= G.GPU_BOUND
    if name == "exact":                                                     # rho == 0 on the first trial: the inputs, exactly
        assert got["info16"][6:9].tolist() == [1, 1, ba_ref.EXIT_RHO_ZERO]
        assert np.array_equal(got["Xw"], p["Xw"]) and np.array_equal(got["T"], p["poses"])
    if name == "special_points":
        assert got["point_status"][:3].tolist() == [0, 0, 0] and got["point_status"][3] == 1
        assert np.array_equal(got["Xw"][:3], p["Xw"][:3]) and np.array_equal(got["T"][4], p["poses"][4])
    if name == "rejects36":
        assert got["info16"][7] == got["info16"][6] + 4                      # four rejected trials
    if name in ("k33", "k43", "band64", "rejects36"):
        assert got["info16"][1] > gba_ref.LDS_FREE_KF                        # the blocked solver ran
    if name in ("one_iteration", "twenty_iterations"):
        assert got["info16"][6] <= G.RUNS[name][1] and (name != "one_iteration" or got["info16"][6:9].tolist()[::2] == [1, ba_ref.EXIT_ITERATIONS])


@pytest.mark.parametrize("name", list(G.REFUSED))
def test_refusals_write_nothing(sd, name):
    from sdslam_amd import capi
    p, status = G.problem(name), G.REFUSED[name][1]
    w, got = gba_ref.run(p, 10, 1), capi.debug_global_ba(p, 10, 1)
    assert w["status"] == status and got["info16"].tolist() == [status] + [0] * 15 == w["info16"].tolist()
    assert np.array_equal(got["T"], p["poses"]) and np.array_equal(got["Xw"], p["Xw"])
    assert np.array_equal(got["point_status"], w["point_status"])


def test_two_runs_give_the_same_bytes(sd):
    from sdslam_amd import capi
    _, nit, robust = G.RUNS["band64"]
    assert same_bytes(capi.debug_global_ba(G.problem("band64"), nit, robust), capi.debug_global_ba(G.problem("band64"), nit, robust))


def test_argument_errors(sd):
    from sdslam_amd import capi
    p = G.problem("stereo_mix")
    for nit, robust in ((0, 1), (21, 1), (5, 2)):
        with pytest.raises(capi.SdError) as e:
            capi.debug_global_ba(p, nit, robust)
        assert e.value.code == 1                                            # SD_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ with a tracker
def resident_problem():
    """local BA's `noisy` on the rig of tests/test_local_ba_gpu.py, its observed cameras without a role made fixed vertices"""
    p = LB.resident_problem("noisy")
    p["roles"] = np.where(p["roles"] == 0, 2, p["roles"]).astype(np.uint8)
    return p


def resident_result(g):
    return dict(T=np.concatenate([g["T_ref"], g["T_cur"][None]]), Xw=g["Xw"], point_status=g["point_status"], info16=g["info16"])


def test_resident_path_equals_the_debug_entry_and_write_back(sd):
    from sdslam_amd import capi
    p = resident_problem()
    trk = LB.rig(sd)["trk"]
    LB.plant(sd, p)
    w = capi.debug_global_ba(p, 10, 0)
    assert w["info16"].tolist() == gba_ref.run(p, 10, 0)["info16"].tolist() and w["info16"][0] == 0
    with pytest.raises(capi.SdError):
        trk.get_global_ba()                                                 # nothing has run since the observations were set
    trk.global_ba(point_row=1, n_iterations=10, robust=False, write_back=False)
    assert same_bytes(resident_result(trk.get_global_ba()), w)
    Tr, Tc = trk.read_poses(B)
    assert np.array_equal(Tr, p["poses"][:B]) and np.array_equal(Tc, np.stack([p["poses"][B]] * B))
    assert np.array_equal(trk.get_local_points(1)["Xw"][:len(p["Xw"])], p["Xw"])
    with pytest.raises(capi.SdError) as e:                                  # a local-BA getter does not answer a global run
        trk._n_ba = (len(p["Xw"]), len(p["kf"]))
        trk.get_local_ba()
    assert "sd_track_local_ba has not run" in str(e.value)
    trk.local_ba(point_row=1, write_back=False)
    with pytest.raises(capi.SdError) as e:                                  # ... nor the global getter a local run
        trk.get_global_ba()
    assert "sd_track_global_ba has not run" in str(e.value)
    # write_back = 1: exactly the getter's values
    trk.global_ba(point_row=1, n_iterations=10, robust=False, write_back=True)
    assert same_bytes(resident_result(trk.get_global_ba()), w)
    Tr, Tc = trk.read_poses(B)
    assert np.array_equal(Tr, w["T"][:B]) and np.array_equal(Tc[0], w["T"][B]) and not np.array_equal(w["T"], p["poses"])
    n = len(p["Xw"])
    assert np.array_equal(trk.get_local_points(1)["Xw"][:n], w["Xw"]) and np.array_equal(trk.get_local_points(0)["Xw"][:n], p["Xw"])
    # the result is kept aside for poses that sd_track_set_poses replaces
    trk.set_poses(0, list(p["poses"][:B]), [p["poses"][B]] * B)
    with pytest.raises(capi.SdError):
        trk.get_global_ba()


def test_resident_argument_errors(sd):
    from sdslam_amd import capi
    trk = LB.rig(sd)["trk"]
    LB.plant(sd, resident_problem())
    for kw in (dict(n_iterations=0), dict(n_iterations=21), dict(robust=2), dict(write_back=2)):
        with pytest.raises(capi.SdError) as e:
            trk.global_ba(**kw)
        assert e.value.code == 1
