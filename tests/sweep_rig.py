"""The rig every tracking sweep runs on, and the cases planted on it (helper, no tests).

A sweep (tests/world_frames.py, tests/cameras.py, tests/geometries.py) is a table of values for one axis and the parameters of
its rig: a camera, a frame size, an extractor configuration, the tracker's max_points and the size of the local map.
oracle_rig builds the two scenes seen through that camera with the oracle's extraction, pyramids and tables and the last-frame
and local-map cases; device_rig puts the same scenes on two extractors and a tracker and asserts once that the device extracted
what the oracle did.  Every case builder below takes the rig and reads its camera, so one definition serves every sweep;
tests/stage_parity.py holds the device-versus-oracle comparison of each stage on such a rig.

A new sweep axis is a new table module whose oracle_rig calls the one here with its parameters (and, through `extend`, adds
what only it needs), plus a test file whose fixture calls device_rig and whose tests call the drivers of stage_parity."""
import numpy as np
import pytest

import cameras as CM
import pnp_cases as PC
from cameras import BF, MOTIONS, POSE_BOUND, SEEDS, START      # noqa: F401  (defined there, next to the builders that the rigs use)

_RIGS = {}


def oracle_rig(O, key, cam, w, h, cfg, max_points, n_extra=None, n_last=None, extend=None):
    """The two scenes of SEEDS / MOTIONS at w x h through `cam` with the oracle's extraction (cfg = the extractor's nfeatures,
    scale factor, levels, FAST threshold), undistorted keypoints, pyramids and tables, and the last-frame and local-map cases
    built from the undistorted keypoints.  ck_raw / rk_raw are mvKeys, ck / rk mvKeysUn (the same arrays without distortion).
    The last frame has the points of the first n_last reference keypoints valid (default: the extractor's nfeatures); the local
    map has n_extra points beside the keypoints' own (default: as many as fill max_points).  extend(O, rig) adds what one sweep
    needs on top.  Cached under `key`."""
    if key in _RIGS:
        return _RIGS[key]
    scenes = [CM.make_scene(s, cam, *m, w=w, h=h) for s, m in zip(SEEDS, MOTIONS)]
    fr = []
    for i, s in enumerate(scenes):
        oc, orf = O.OrbOracle(*cfg), O.OrbOracle(*cfg)
        ck, cd = oc.extract(s["cur"])
        rk, rd = orf.extract(s["ref"])
        cku, rku = CM.undistorted(O, ck, cam), CM.undistorted(O, rk, cam)
        last = CM.tracking_case(i, rku, rd, cam, max_points=cfg[0] if n_last is None else n_last)
        local = CM.local_map_case(100 + i, cku, cd, s["T_cur"], cam, n_extra=max_points - len(ck) if n_extra is None else n_extra,
                                  scale_factor=cfg[1], nlevels=cfg[2])
        fr.append(dict(ck_raw=ck, ck=cku, cd=cd, rk_raw=rk, rk=rku, rd=rd, tab=oc.tables(), last=last, local=local, oc=oc, orf=orf,
                       pc=[oc.level(l) for l in range(cfg[2])], pr=[orf.level(l) for l in range(cfg[2])]))
    rig = dict(cam=cam, w=w, h=h, cfg=cfg, max_points=max_points, scenes=scenes, fr=fr, B=len(scenes))
    if extend is not None:
        extend(O, rig)
    _RIGS[key] = rig
    return rig


# ---- the rig on the device ------------------------------------------------------------------------------------------------
def device():
    """sdslam_amd, if there is a device to run on."""
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sd


def device_rig(rig, pnp_max_iterations):
    """(rig, close): a copy of the oracle's rig with two extractors (with the camera's distortion) holding its scenes and a
    tracker, in the state `restore` leaves.  The oracle's keypoints, descriptors and undistorted keypoints equal the device's,
    asserted once."""
    sd = device()
    r = dict(rig)
    cam, B, scenes, fr = r["cam"], r["B"], r["scenes"], r["fr"]
    cur, ref = sd.ORBextractor(*r["cfg"], r["w"], r["h"], B), sd.ORBextractor(*r["cfg"], r["w"], r["h"], B)
    if cam.dist is not None:
        for e in (cur, ref):
            e.set_distortion(*cam.K, *cam.dist)
    ck, cd, cn = cur.extract_batch(np.stack([s["cur"] for s in scenes]))
    rk, rd, rn = ref.extract_batch(np.stack([s["ref"] for s in scenes]))
    cu, ru = cur.download_undistorted(0, B), ref.download_undistorted(0, B)
    for i in range(B):
        assert np.array_equal(fr[i]["ck_raw"], ck[i, :cn[i]]) and np.array_equal(fr[i]["cd"], cd[i, :cn[i]]), (cam.name, i)
        assert np.array_equal(fr[i]["rk_raw"], rk[i, :rn[i]]) and np.array_equal(fr[i]["rd"], rd[i, :rn[i]]), (cam.name, i)
        assert np.array_equal(fr[i]["ck"], cu[i, :cn[i]]) and np.array_equal(fr[i]["rk"], ru[i, :rn[i]]), (cam.name, i)
    trk = sd.Tracker(cur, ref, max_points=r["max_points"], max_batch=B, pnp_max_iterations=pnp_max_iterations)
    r.update(sd=sd, trk=trk, ext=(cur, ref), cap=ck.shape[1])
    restore(r)

    def close():
        trk.close()
        cur.close()
        ref.close()

    return r, close


def restore(rig):
    """Camera, last frames, local maps, right coordinates and poses as device_rig leaves them."""
    trk, cam = rig["trk"], rig["cam"]
    trk.set_camera(*cam.K, 0.0, cam.bounds)
    trk.stereo_from_depth(np.zeros((rig["B"], rig["h"], rig["w"]), np.float32))      # resets every mvuRight to -1
    trk.set_last(0, [f["last"] for f in rig["fr"]])
    trk.set_local(0, [f["local"] for f in rig["fr"]])
    trk.set_poses(0, refs(rig), currents(rig))


def refs(rig):
    return [s["T_ref"] for s in rig["scenes"]]


def currents(rig):
    return [s["T_cur"] for s in rig["scenes"]]


def starts(rig):
    """The perturbed start of every frame."""
    return [START @ s["T_cur"] for s in rig["scenes"]]


def log_sf(rig):
    return np.log(np.float32(rig["cfg"][1]))


# ---- the cases planted on a rig ---------------------------------------------------------------------------------------------
def planted_case(rig, i, seed=None):
    """The planted 30 %-outlier match vector of tests/test_pnp_ransac.py::test_pose_optimization_on_caller_matches on frame i's
    undistorted keypoints, through the rig's camera: (last, cm, truth)."""
    f = rig["fr"][i]
    return CM.planted_matches(11 + i if seed is None else seed, f["ck"], rig["scenes"][i]["T_cur"], rig["cam"], n_match=min(300, len(f["ck"])),
                              outlier_frac=0.3, noise_px=0.5)


def planted_uright(rig, i, last, cm, truth, bf=BF):
    """A right-image coordinate for every third matched keypoint: the planted inliers' from their true depth, the outliers' from
    a depth of 3 m (wrong like the rest of them)."""
    ck, T = rig["fr"][i]["ck"], rig["scenes"][i]["T_cur"]
    zc = (last["Xw"] @ T[:3, :3].T + T[:3, 3])[:, 2]
    zc = np.where(truth, zc, 3.0)
    return np.where((np.arange(len(ck)) % 3 == 0) & (cm >= 0), ck["x"] - bf / zc, -1.0).astype(np.float32)


def planted_cur_uright(rig, i, bf=BF):
    """mvuRight for every third current keypoint from the depth of the surface point it sees; -1 for the others."""
    f, T = rig["fr"][i], rig["scenes"][i]["T_cur"]
    Xw = CM.keyframe_case(f["ck"], f["cd"], T, rig["cam"])["Xw"]
    zc = (Xw @ T[:3, :3].T + T[:3, 3])[:, 2]
    return np.where(np.arange(len(zc)) % 3 == 0, f["ck"]["x"] - bf / zc, -1.0).astype(np.float32)


matched_points = PC.matched_points


def pnp_case(rig, i, scenario):
    """pnp_cases.SCENARIOS[scenario] planted through the rig's camera, the match count capped at the frame's keypoint count:
    (last, cm, truth, params, calls)."""
    kw, params, calls = PC.SCENARIOS[scenario]
    f = rig["fr"][i]
    last, cm, truth = CM.planted_matches(7 + i, f["ck"], rig["scenes"][i]["T_cur"], rig["cam"], **dict(kw, n_match=min(kw["n_match"], len(f["ck"]))))
    return last, cm, truth, params, calls

