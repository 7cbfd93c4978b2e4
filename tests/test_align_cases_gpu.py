"""The hand-built ImageAlign problems of tests/align_cases.py on the device: all cases of one mode and one frame size are the frames
of ONE sd_track_align launch (images through the extractors' pyramids, points through sd_track_set_last, poses through set_poses),
once per register budget of k_align (track.align_min_waves 3, 4, 5) and once more with the cases in reverse order, which must give
every case the same bytes.  Against the oracle, with the bars of tests/test_track_gpu.py: ok and per-level iterations equal, pose
within 1e-5, error to a relative 1e-7, chi2 to a relative 1e-9; where the oracle returns false, and in mode 3, the pose is the prior
byte for byte.  tests/test_align_cases_cpu.py certifies on the host that every case may be held to that."""
import numpy as np
import pytest

import align_cases as AC

pytestmark = pytest.mark.gpu
MP = 700                                                             # max_points: the 690-row arrays of the count cases


@pytest.fixture(scope="module")
def rig(oracle):
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    groups = {}
    for c in AC.all_cases(oracle):
        groups.setdefault((c["mode"], c["size"]), []).append(c)
    handles = {}
    for key, cs in groups.items():
        (w, h), B = key[1], len(cs)
        cur, ref = sd.ORBextractor(*AC.CFG, w, h, B), sd.ORBextractor(*AC.CFG, w, h, B)
        trk = sd.Tracker(cur, ref, MP, B)
        cam = AC.camera(key[1])
        trk.set_camera(*cam.K, 0.0, cam.bounds)
        handles[key] = (cur, ref, trk)
    yield dict(sd=sd, groups=groups, handles=handles, want={c["name"]: AC.certify(oracle, c)["ref"] for cs in groups.values() for c in cs})
    for cur, ref, trk in handles.values():
        for x in (trk, cur, ref):
            x.close()


def _set_last(trk, cases):
    """sd_track_set_last with each case's own n_last: rows at or above it keep the flags and points the case put there"""
    from sdslam_amd import capi
    n = len(cases)
    valid, Xw = np.zeros((n, MP), np.uint8), np.zeros((n, MP, 3))
    for i, c in enumerate(cases):
        valid[i, :len(c["valid"])], Xw[i, :len(c["Xw"])] = c["valid"], c["Xw"]
    n_last = np.array([c["n_last"] for c in cases], np.int32)
    desc, octave, angle, obs = np.zeros((n, MP, 32), np.uint8), np.zeros((n, MP), np.int32), np.zeros((n, MP), np.float32), np.ones((n, MP), np.int32)
    capi._check(trk.L.sd_track_set_last(trk.h, 0, n, *[capi._p(a) for a in (n_last, valid, Xw, desc, octave, angle, obs)]))


def _launch(rig, key, cases, min_waves):
    cur, ref, trk = rig["handles"][key]
    n = len(cases)
    assert cur.extract_batch(np.stack([c["cur"] for c in cases]))[2].shape == (n,)
    ref.extract_batch(np.stack([c["ref"] for c in cases]))
    _set_last(trk, cases)
    trk.set_poses(0, [c["T_ref"] for c in cases], [c["T0"] for c in cases])
    with rig["sd"].options({"track.align_min_waves": min_waves}):
        trk.align(n, key[0])
    return trk.get_align(0, n)


def _check(rig, c, g, i, what):
    r = rig["want"][c["name"]]
    d = np.abs(g["T"][i] - r["T"]).max()
    e = abs(g["error"][i] - r["error"]) / max(1.0, abs(r["error"]))
    q = abs(g["chi2"][i] - r["chi2"]) / max(1.0, abs(r["chi2"]))
    print(f"{c['name']} {what}: ok {bool(g['ok'][i])} / {r['ok']} iters {g['iters'][i][2:5].tolist()} / {r['iters'][2:5].tolist()} pose {d:.2e} "
          f"error {e:.1e} chi2 {q:.1e}")
    key = (c["name"], what)
    assert bool(g["ok"][i]) == r["ok"], key
    assert np.array_equal(g["iters"][i][:len(r["iters"])], r["iters"]) and not g["iters"][i][len(r["iters"]):].any(), (key, g["iters"][i], r["iters"])
    assert d <= AC.POSE_TOL, (key, d)
    assert e <= 1e-7, (key, g["error"][i], r["error"])
    assert q <= 1e-9, (key, g["chi2"][i], r["chi2"])
    if not r["ok"] or c["mode"] == 3:
        assert np.array_equal(g["T"][i], c["T0"]), key               # the prior, byte for byte
    if c["name"] == "same_image":
        assert g["chi2"][i] == 0.0 and g["error"][i] == 0.0, key
    return d


@pytest.mark.parametrize("min_waves", [3, 4, 5])
def test_align_cases(rig, min_waves):
    worst = 0.0
    for key, cases in rig["groups"].items():
        g = _launch(rig, key, cases, min_waves)
        for i, c in enumerate(cases):
            worst = max(worst, _check(rig, c, g, i, "min_waves %d" % min_waves))
    print(f"min_waves {min_waves}: largest device-oracle pose difference {worst:.2e} (host noise floor {AC.NOISE_FLOOR:.1e})")


def test_workgroups_are_independent(rig):
    """The same cases in reverse order: every case gets the same bytes whatever workgroup runs it and whatever its neighbours are"""
    for key, cases in rig["groups"].items():
        a, b = _launch(rig, key, cases, 5), _launch(rig, key, cases[::-1], 5)
        n = len(cases)
        for i, c in enumerate(cases):
            j = n - 1 - i
            _check(rig, c, b, j, "reversed")
            assert np.array_equal(a["T"][i], b["T"][j]) and a["ok"][i] == b["ok"][j] and np.array_equal(a["iters"][i], b["iters"][j]), c["name"]
            assert a["error"][i].tobytes() == b["error"][j].tobytes() and a["chi2"][i].tobytes() == b["chi2"][j].tobytes(), c["name"]
