"""CPU (no GPU): the numpy restatement tests/append_ref.py that tests/test_append_points_gpu.py holds k_append_points /
k_append_commit to, on the oracle's keypoints of the three-view scene of test_new_points_cpu.py with the stereo mix (broadcast:
cur frame 0 against the three ref frames): the `cand` rule equals IsInKeyFrame and `obs` equals nObs on the toy map after the
reference's sequential CreateNewMapPoints loop; overflow keeps the first points in order; the Fuse search over the appended row
finds appended points in every neighbour other than their own (the coverage the GPU chain test relies on); the lifetime table;
the new C entry points' presence and argument checks."""
import os
import subprocess

import numpy as np
import pytest

import append_ref as AR
import fuse_ref as FR
import new_points_cases as NC
import new_points_ref as NR
import triangulation_cases as TC
import triangulation_ref as TR

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = 40.0
B = 3
FIRST_ID = 1000
NEW_CALLS = ["sd_track_append_new_points", "sd_track_get_appended", "sd_track_get_local_points"]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
_SCENE = {}


def scene(oracle):
    """The broadcast CreateNewMapPoints of the three-view scene, by the reference's sequential loop (create_new_map_points) and by
    "search all, triangulate all, resolve" (what the device does): the points, and what the append reads besides.  Computed once."""
    if not _SCENE:
        import test_triangulation_gpu as TG
        sc = TG.scene(dict(cfg=(1000, 1.2, 8, 20)), oracle=oracle)
        mix = NC.batched_mix(sc["k1"], sc["k2"], TG.T_CUR, TG.T_REF, TC.K, BF)
        cam5 = np.array([*TC.K, BF], F32)
        n1 = int(sc["n1"][0])
        k1, d1 = sc["k1"][0, :n1], sc["d1"][0, :n1]
        neigh = []
        for b in range(B):
            n2 = int(sc["n2"][b])
            neigh.append(dict(ku=sc["k2"][b, :n2], k=sc["k2"][b, :n2], d=sc["d2"][b, :n2], has=np.zeros(n2, np.uint8), ur=mix["u2"][b, :n2],
                              z=mix["z2"][b, :n2], T=TG.T_REF[b], median=-1.0))
        seq = NR.create_new_map_points(k1, k1, d1, np.zeros(n1, np.uint8), mix["u1"][0, :n1], mix["z1"][0, :n1], neigh, TG.T_CUR[0], cam5,
                                       TC.SF, TC.SIGMA2, 1.2, False, FIRST_ID)
        verdicts, matches, Xws = [], [], []
        for nb in neigh:
            _, m12 = TR.search_for_triangulation(k1, d1, np.zeros(n1, np.uint8), mix["u1"][0, :n1], nb["ku"], nb["d"], nb["has"], nb["ur"],
                                                 TR.compute_f12(TG.T_CUR[0], nb["T"], TC.K), TR.epipole(TG.T_CUR[0], nb["T"], TC.K), TC.SF,
                                                 TC.SIGMA2)
            v, _, X = NR.triangulate(k1, k1, mix["u1"][0, :n1], mix["z1"][0, :n1], nb["ku"], nb["k"], nb["ur"], nb["z"], m12, TG.T_CUR[0],
                                     nb["T"], cam5, TC.SF, TC.SIGMA2, 1.2, False, -1.0)
            verdicts.append(v)
            matches.append(m12)
            Xws.append(X)
        pts, _ = NR.resolve(verdicts, matches, Xws, [TG.T_CUR[0]] * B, TG.T_REF, k1, d1, TC.SF, [FIRST_ID], True)
        _SCENE.update(sc=sc, mix=mix, seq=seq, pts=pts, neigh=neigh, n1=n1, T_REF=TG.T_REF, bounds=TG.BOUNDS)
    return _SCENE


def empty_rows(M, n_local=(0, 0, 0)):
    return AR.sentinel_rows(B, M, n_local)


def test_cand_is_is_in_keyframe_and_obs_is_nobs_on_the_toy_map(oracle):
    s = scene(oracle)
    pts, mix = s["pts"], s["mix"]
    assert NR.same_points(pts, s["seq"]) and len(pts) >= 150                  # the resolve is the sequential loop, here too
    kf1 = AR.StereoKeyFrame("kf1", mix["u1"][0])
    neigh = [AR.StereoKeyFrame("n%d" % b, mix["u2"][b]) for b in range(B)]
    extra = AR.StereoKeyFrame("target beyond the neighbours", mix["u2"][0])     # a Fuse target that triangulated nothing
    made = AR.toy_create(s["seq"], kf1, neigh)
    M = len(pts) + 7
    rows = empty_rows(M, (5, 0, 0))
    out, result, pos = AR.append(rows, pts, 0, B, mix["u1"], mix["u2"], 0, B)
    assert result.tolist() == [[5, len(pts), 0], [0, 0, 0], [0, 0, 0]] and out["n"].tolist() == [5 + len(pts), 0, 0]
    assert pos.tolist() == list(range(5, 5 + len(pts)))
    targets = neigh + [extra]
    out4, _, _ = AR.append(AR.sentinel_rows(B + 1, M, (5, 0, 0, 0)), pts, 0, B, mix["u1"], mix["u2"], 0, B + 1)
    for g, mp in enumerate(made):
        assert out["obs"][0, pos[g]] == mp.nObs, g
        for f, kf in enumerate(targets):
            assert out4["cand"][f, pos[g]] == (not mp.IsInKeyFrame(kf)), (g, f)
        assert (out["cand"][:, pos[g]] == out4["cand"][:B, pos[g]]).all()
    assert set(out["obs"][0, 5:5 + len(pts)].tolist()) == {2, 3, 4}            # mono-mono, one stereo side, both
    assert len({p["slot"] for p in pts}) == B
    # the fields, bit for bit, and nothing outside [base, base + appended) of any array or row
    for g, p in enumerate(pts):
        i = pos[g]
        assert out["Xw"][0, i].tobytes() == p["Xw"].tobytes() and out["normal"][0, i].tobytes() == p["normal"].tobytes()
        assert out["mf_max_dist"][0, i] == p["max_dist"] and out["max_dist"][0, i] == F32(F32(1.2) * p["max_dist"])
        assert out["min_dist"][0, i] == F32(F32(0.8) * p["min_dist"]) and (out["desc"][0, i] == p["desc"]).all()
    keep = np.ones(M, bool)
    keep[5:5 + len(pts)] = False
    for k, _, _ in AR.FIELDS:
        assert out[k][0, keep].tobytes() == rows[k][0, keep].tobytes(), k
        if k != "cand":
            assert out[k][1:].tobytes() == rows[k][1:].tobytes(), k
        else:
            assert out[k][1:, keep].tobytes() == rows[k][1:, keep].tobytes()


def test_overflow_keeps_the_first_points_in_order(oracle):
    s = scene(oracle)
    pts, mix = s["pts"], s["mix"]
    n = len(pts)
    M = n + 7
    full, _, _ = AR.append(empty_rows(M), pts, 0, B, mix["u1"], mix["u2"], 0, B)
    for base in (M - n // 2, M - 1, M):
        rows = empty_rows(M, (base, 3, 0))
        out, result, pos = AR.append(rows, pts, 0, B, mix["u1"], mix["u2"], 0, B)
        fit = M - base
        assert result[0].tolist() == [base, fit, n - fit] and out["n"].tolist() == [M if fit else base, 3, 0]
        assert pos.tolist() == list(range(base, M)) + [-1] * (n - fit)
        for k, _, _ in AR.FIELDS:
            if k == "cand":
                assert out[k][:, base:].tobytes() == full[k][:, :fit].tobytes()
                assert out[k][:, :base].tobytes() == rows[k][:, :base].tobytes()
            else:
                assert out[k][0, base:].tobytes() == full[k][0, :fit].tobytes(), k    # the first `fit` points, in order
                assert out[k][0, :base].tobytes() == rows[k][0, :base].tobytes() and out[k][1:].tobytes() == rows[k][1:].tobytes()
    # paired mode: every slot's points behind its own row's, each row overflowing on its own
    per_slot = np.bincount([p["slot"] for p in pts], minlength=B)
    paired = [dict(p) for p in pts]
    M2 = int(per_slot.max()) + 2
    bases = (0, M2 - 3, M2)
    u1 = np.stack([mix["u1"][0]] * B)                          # (the restatement of a paired result reads KF1's row per slot)
    out, result, pos = AR.append(empty_rows(M2, bases), paired, -1, B, u1, mix["u2"], -1, 0)
    for b in range(B):
        fit = min(int(per_slot[b]), M2 - bases[b])
        assert result[b].tolist() == [bases[b], fit, per_slot[b] - fit]
        mine = [g for g, p in enumerate(pts) if p["slot"] == b]
        assert pos[mine].tolist() == list(range(bases[b], bases[b] + fit)) + [-1] * (len(mine) - fit)
        assert (out["cand"][b, bases[b]:bases[b] + fit] == 1).all()


def fuse_coverage(s, rows, pts, pos, search):
    """Appended points the Fuse search of neighbour f finds (best_idx >= 0) although another neighbour triangulated them."""
    found = []
    for f in range(B):
        best_idx, _ = search(f, rows)
        found.append(sum(1 for g, p in enumerate(pts) if pos[g] >= 0 and p["slot"] != f and best_idx[pos[g]] >= 0))
    return found


def test_fuse_finds_appended_points_in_the_other_neighbours(oracle):
    s = scene(oracle)
    pts, mix, sc = s["pts"], s["mix"], s["sc"]
    M = len(pts) + 7
    rows = empty_rows(M, (5, 0, 0))
    rows["cand"][:, :5] = 0                                      # the sentinel points before the base are no candidates
    out, _, pos = AR.append(rows, pts, 0, B, mix["u1"], mix["u2"], 0, B)
    cam9 = np.array([*TC.K, BF, *s["bounds"]], F32)
    inv_sigma2 = (F32(1.0) / TC.SIGMA2).astype(F32)

    def search(f, rows):
        n2, n = int(sc["n2"][f]), int(rows["n"][0])
        p = dict(cand=rows["cand"][f, :n], Xw=rows["Xw"][0, :n], normal=rows["normal"][0, :n], min_dist=rows["min_dist"][0, :n],
                 max_dist=rows["max_dist"][0, :n], mf_max_dist=rows["mf_max_dist"][0, :n], desc=rows["desc"][0, :n])
        return FR.fuse_search(sc["k2"][f, :n2], sc["d2"][f, :n2], mix["u2"][f, :n2], p, s["T_REF"][f], cam9, TC.SF, inv_sigma2, 1.2, 3.0)
    found = fuse_coverage(s, out, pts, pos, search)
    print("appended points found in a neighbour other than their own:", found)
    assert all(n >= 1 for n in found), found
    # a point reads "not a candidate" in its own neighbour
    for f in range(B):
        best_idx, best_dist = search(f, out)
        own = [pos[g] for g, p in enumerate(pts) if p["slot"] == f]
        assert (best_idx[own] == -1).all() and (best_dist[own] == 256).all()


def test_mark_flags_is_add_map_point(oracle):
    s = scene(oracle)
    pts, mix = s["pts"], s["mix"]
    cap = s["sc"]["cap"]
    kf1 = AR.StereoKeyFrame("kf1", mix["u1"][0])
    neigh = [AR.StereoKeyFrame("n%d" % b, mix["u2"][b]) for b in range(B)]
    AR.toy_create(pts, kf1, neigh)
    pos = np.arange(len(pts))
    h1, h2 = AR.mark_flags(np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8), pts, pos, 0, B)
    for b in range(B):
        assert h1[b].tolist() == [p is not None for p in kf1.points]            # every slot's row stands for the one KF1
        assert h2[b].tolist() == [p is not None for p in neigh[b].points]
    pos[len(pts) // 2:] = -1                                                    # dropped points are not flagged
    h1, h2 = AR.mark_flags(np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8), pts, pos, 0, B)
    half = pts[:len(pts) // 2]                                                  # (two KF1 keypoints may share a KF2 keypoint)
    assert h1[0].sum() == len(half) and h2.sum() == len({(p["slot"], p["idx2"]) for p in half})
    # paired: KF1 of slot b is cur frame b, one row each
    h1, h2 = AR.mark_flags(np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8), pts, np.arange(len(pts)), -1, B)
    assert h1.sum() == len(pts) and all(h1[p["slot"], p["kp1"]] for p in pts)


def test_result_lifetimes(tmp_path):
    """tests/native/append_stamps_check.cpp: what ends the append's result, what an append ends, plain and under ASan + UBSan."""
    for flags in (["-O2"], SAN):
        exe = str(tmp_path / "append_stamps_check")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "sdslam_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", "append_stamps_check.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and "append_stamps_check OK" in out.stdout, out.stdout + out.stderr


def test_entry_points_exist_and_check_their_arguments():
    from sdslam_amd import build, capi
    import test_capi_signatures_cpu as SIG
    build.build()
    L = capi.lib()
    protos = SIG.prototypes()
    want = {
        "sd_track_append_new_points": ("int", [SIG.PTR, "int", "int", "int"]),
        "sd_track_get_appended": ("int", [SIG.PTR, "int", "int", SIG.PTR, SIG.PTR, SIG.PTR]),
        "sd_track_get_local_points": ("int", [SIG.PTR, "int"] + [SIG.PTR] * 9 + ["int"]),
    }
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in capi._SIGNATURES and protos[name] == want[name], name
    assert L.sd_track_append_new_points(None, 0, 0, 0) == 1 and b"NULL" in L.sd_last_error()
    assert L.sd_track_get_appended(None, 0, 1, None, None, None) == 1
    assert L.sd_track_get_local_points(None, 0, None, None, None, None, None, None, None, None, None, 0) == 1
    for m in ("append_new_points", "get_appended", "get_local_points"):
        assert callable(getattr(capi.Tracker, m))
