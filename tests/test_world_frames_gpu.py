"""GPU parity of the pose solvers and matchers in world frames far from the identity (tests/world_frames.py).  Every
other tracking test plants its data around T_ref = I and a T_cur half a degree away, so the kernels that take a world pose
have met the oracle only where R ~ I and |t| ~ 0.  Here each stage runs on the same images and keypoints with the world
moved by G (X' = G X, n' = R_G n, T' = T G^-1) and is compared with the oracle called on the same moved inputs: the three
`trace <= 0` branches of k_pose_opt's matrix -> quaternion conversion, its `t > 0` boundary and strict `>` ties, EPnP's
PCA of world points that do not lie in the camera's axes, and projections whose t cancels against R X.
tests/test_world_frames_cpu.py shows that the oracle alone meets the first-principles bounds used here."""
import numpy as np
import pytest

import stage_parity as SP
import sweep_rig as SR
import world_frames as WF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig(oracle):
    SR.device()
    r, close = SR.device_rig(WF.oracle_rig(oracle), pnp_max_iterations=512)
    yield r
    close()


@pytest.mark.parametrize("name", WF.NAMES)
def test_pose_optimization(oracle, rig, name):
    """The planted 30 %-outlier vector through set_matches, one and four waves per frame, mono and with planted uRight,
    from the perturbed start -- and, in the two exact frames, from the old-frame identity, whose rotation is the tie
    matrix.  Identical flags and counts, pose within 1e-5 of the oracle's, and the device's own result within the
    first-principles bounds."""
    G, B = WF.FRAMES[name], rig["B"]
    starts = [("perturbed", SR.starts(rig))] + ([("identity", [np.eye(4)] * B)] if name in WF.EXACT_TIES else [])
    res = SP.pose_optimization(oracle, rig, name, G, starts)
    for key, g in res["got"]:
        for i in range(B):
            WF.assert_converged(g["T"][i], rig["scenes"][i]["T_cur"], G, key + (i,))
    print(f"pose_opt {name}: largest device-oracle pose difference {res['worst']:.3e}")


@pytest.mark.parametrize("scenario", ["out30_c4", "out65_chunked"])       # one that refines at once; one re-entered in chunks
@pytest.mark.parametrize("name", WF.NAMES)
def test_pnp_ransac(oracle, rig, name, scenario):
    res = SP.pnp_ransac(oracle, rig, name, scenario, WF.FRAMES[name], refined=True)
    print(f"pnp {name} {scenario}: largest device-oracle pose difference {res['worst']:.3e}")


@pytest.mark.parametrize("name", WF.NAMES)
def test_epnp_alone(oracle, rig, name):
    """compute_pose through debug_epnp on the trials of test_epnp_device_vs_oracle; that test's absolute 1e-9 was set for
    |t| ~ 1 and scales with the size of t' here."""
    worst, _ = SP.epnp_alone(oracle, name, rig["cam"].K, WF.epnp_trials(WF.FRAMES[name]), tol=lambda Tp: 1e-9 * max(1.0, np.abs(Tp[:3, 3]).max()))
    print(f"epnp {name}: largest device-oracle difference {worst:.3e}")


def _depth(B):
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    depth = np.stack([(1.5 + 0.8 * np.sin(xx * 0.013 + i) * np.cos(yy * 0.017)).astype(np.float32) for i in range(B)])
    depth[:, 100:140, :] = 0.0            # holes: no depth -> mvuRight = -1
    return depth


@pytest.mark.parametrize("name", WF.NAMES)
def test_search_by_projection(oracle, rig, name):
    """SearchByProjection(Frame, Frame) as two kernels and as one, mono, and once on RGB-D frames (the forward / backward
    gate reads Tlc = Tcur Tlast^-1): match vector and count equal the oracle's."""
    runs = [(True, 8.0, 1), (True, 8.0, 0), (False, 8.0, 1)]        # (mono, th, track.match_split)
    SP.search_by_projection(oracle, rig, name, runs, {8.0: 100}, WF.FRAMES[name], depth=_depth(rig["B"]))


@pytest.mark.parametrize("name", WF.NAMES)
def test_local_map_search(oracle, rig, name):
    """isInFrustum (camera centre -R^T t, view cosine against the moved normals), PredictScale and the search: every
    output equals the oracle's."""
    SP.local_map_search(oracle, rig, name, 150, WF.FRAMES[name])


@pytest.mark.parametrize("name", WF.NAMES)
def test_image_align(oracle, rig, name):
    """ImageAlign from the perturbed start in modes 0 (frame), 2 (keyframe, fast) and 3 (keyframe against keyframe): what
    test_image_align_matches_oracle and test_image_align_modes compare, to their tolerances."""
    res = SP.image_align(oracle, rig, name, WF.FRAMES[name], modes=[(0, "last"), (2, "last"), (3, "last")], chi2=True)
    print(f"align {name}: largest device-oracle pose difference {res['worst']:.3e}")


@pytest.mark.parametrize("name", ["ry170", "far"])
def test_motion_model_then_local_map(oracle, rig, name):
    """TrackWithMotionModel and TrackLocalMap chained on the device, as test_track_with_motion_model_decisions and
    test_track_local_map_after_motion_model run them, in two frames."""
    G = WF.FRAMES[name]
    res = SP.motion_model_then_local_map(oracle, rig, name, ("n_local", 101), G)
    for i in range(rig["B"]):
        WF.assert_converged(res["T_mm"][i], rig["scenes"][i]["T_cur"], G, (name, "motion model", i))
