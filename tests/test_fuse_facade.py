"""The C++ facade's ORBmatcher::Fuse on the GPU: tests/native/facade_fuse.cc builds a toy map (KeyFrame / MapPoint classes whose
Replace and AddObservation follow src/MapPoint.cc) over the dense extraction scene of tests/test_fuse_gpu.py, runs the vector
overload over the three target keyframes -- one device call with a shared point row, then the facade's in-order walk -- and,
in a second run, the Sim3 overload on one keyframe, and writes nFused, vpReplacePoint and the whole map's state.  Both must
equal the reference's sequential loops (fuse_ref.fuse_sequential / fuse_sim3) driven by the numpy restatement's searches.
(The link check without a GPU is in tests/test_fuse_cpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

import fuse_ref as FR
import test_fuse_gpu as G
import triangulation_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG = G.TG
SCALE = G.SCALES[0]


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


@pytest.fixture(scope="module")
def exe(sd, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("facade") / "sd_facade_fuse")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_fuse.cc"), "-o", out, "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    return out


def numbered(kfs, pts):
    """Ids for the program: list points first (None keeps its slot), then the foreign points the keyframes hold; target keyframes
    first, then every other keyframe an observation names."""
    all_pts = list(pts)
    seen = {id(p) for p in pts if p is not None}
    for kf in kfs:
        for p in kf.points:
            if p is not None and id(p) not in seen:
                seen.add(id(p))
                all_pts.append(p)
    all_kfs, kseen = list(kfs), {id(k) for k in kfs}
    for p in all_pts:
        for kf in (p.obs if p is not None else ()):
            if id(kf) not in kseen:
                kseen.add(id(kf))
                all_kfs.append(kf)
    return all_pts, all_kfs


def state(all_pts, all_kfs, n_targets, n_fused, replace):
    pid = {id(p): i for i, p in enumerate(all_pts) if p is not None}
    kid = {id(k): i for i, k in enumerate(all_kfs)}
    out = list(n_fused) + [-1 if r is None else pid[id(r)] for r in replace]
    for kf in all_kfs[:n_targets]:
        out += [len(kf.points)] + [-1 if p is None else pid[id(p)] for p in kf.points]
    for p in all_pts:
        if p is None:
            out += [0, -1, 0]
            continue
        obs = sorted((kid[id(kf)], idx) for kf, idx in p.obs.items())
        out += [int(p.bad), -1 if p.replaced is None else pid[id(p.replaced)], len(obs)] + [v for o in obs for v in o]
    return np.array(out, np.int32)


def run(exe, tmp_path, r, mode, all_pts, all_kfs, n_pts):
    sc = r["sc"]
    base = sc["rows"][0]
    pid = {id(p): i for i, p in enumerate(all_pts) if p is not None}
    kid = {id(k): i for i, k in enumerate(all_kfs)}
    obs = [(pid[id(p)], kid[id(kf)], idx, int(len(kf.points) > idx and kf.points[idx] is p))
           for p in all_pts if p is not None for kf, idx in p.obs.items()]
    S = TG.T_REF[0].copy()
    S[:3, :] *= SCALE
    inp, outp = str(tmp_path / ("fuse%d.in" % mode)), str(tmp_path / ("fuse%d.out" % mode))
    nf = r["cfg"]["cfg"][0]
    ur = np.full((G.B, nf), -1, np.float32)
    ur[:, :sc["cap"]] = sc["ur"][1][:, :nf]
    with open(inp, "wb") as f:
        f.write(np.array([G.W, G.H, G.B, n_pts, sc["M"], len(all_pts), len(all_kfs), len(obs), mode, nf], np.int32).tobytes())
        f.write(np.array([*TC.K, G.BF], np.float32).tobytes())
        f.write(np.array([3.0], np.float32).tobytes())
        f.write(np.ascontiguousarray(S, np.float64).tobytes())                          # row-major: read as Scw(r, c)
        f.write(np.ascontiguousarray(r["imgs"][1], np.uint8).tobytes())
        f.write(np.stack([np.ascontiguousarray(T.T, np.float64) for T in TG.T_REF]).tobytes())   # column-major, as GetPose().data()
        f.write(ur.tobytes())
        f.write(np.array([p is not None for p in all_pts[:n_pts]], np.uint8).tobytes())
        for key, dt in (("Xw", np.float64), ("normal", np.float64), ("min_dist", np.float32), ("max_dist", np.float32),
                        ("mf_max_dist", np.float32), ("desc", np.uint8)):
            f.write(np.ascontiguousarray(base[key], dt).tobytes())
        f.write(np.array([len(kf.points) for kf in all_kfs], np.int32).tobytes())
        f.write(np.array(obs, np.int32).reshape(-1, 4).tobytes())
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ran mode %d" % mode in out.stdout, (out.returncode, out.stdout, out.stderr)
    return np.frombuffer(open(outp, "rb").read(), np.int32)


def test_vector_overload_equals_the_sequential_loop(sd, exe, tmp_path):
    r = G.rig(sd, "dense")
    sc = r["sc"]
    kfs, pts = G.toy_map(sc)
    all_pts, all_kfs = numbered(kfs, pts)
    got = run(exe, tmp_path, r, 0, all_pts, all_kfs, len(pts))       # (the map is serialised before the reference loop changes it)
    want_n = FR.fuse_sequential(kfs, pts, G.toy_search(sc))
    want = state(all_pts, all_kfs, G.B, want_n, [None] * len(pts))
    assert got[:G.B].tolist() == want_n and sum(want_n) >= 20
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8] if len(got) == len(want) else (len(got), len(want))
    assert sum(p is not None and p.bad for p in all_pts) > 0         # something was replaced


def test_sim3_overload_fills_vpReplacePoint(sd, exe, tmp_path):
    r = G.rig(sd, "dense")
    sc = r["sc"]
    kfs, pts = G.toy_map(sc)
    all_pts, all_kfs = numbered(kfs, pts)
    got = run(exe, tmp_path, r, 1, all_pts, all_kfs, len(pts))
    base = sc["rows"][0]
    every = dict(sc, rows=[dict(base, cand=np.ones(len(base["cand"]), np.uint8))] * G.B)
    best = G.restate(every, (1, False, 0, 1), 0)[0]                  # slot 0 of that configuration: Scw = SCALES[0] * T_REF[0]
    replace = [None] * len(pts)
    n = FR.fuse_sim3(kfs[0], pts, lambda kf, i: int(best[i]), replace)
    want = state(all_pts, all_kfs, 1, [n], replace)
    assert got[0] == n and n >= 20 and 0 < sum(x is not None for x in replace) < n       # some replaced, some added
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8] if len(got) == len(want) else (len(got), len(want))
