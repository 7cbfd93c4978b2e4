"""The C++ facade's Sim3Solver / LoopClosing::ComputeSim3Candidates: tests/native/facade_sim3.cc runs the iterate(5)
round-robin of src/LoopClosing.cc:270-290 on three loop candidates of which the second is the true loop, and must return
slot 1 with the iteration counts, inlier count, T12 and scale of the numpy restatement driven the same way (the batch iterates
all live slots per round, so the slot after the winner has run that round too)."""
import os
import subprocess

import numpy as np
import pytest

import sim3_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["n70_all_out", "n70_out30", "n70_all_out"]
PYR = "p8"


def _build(tmp_path, sd):
    exe = str(tmp_path / "sd_facade_sim3")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_sim3.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    return exe


def test_cpp_sim3_facade_compiles_and_links(tmp_path):
    import sdslam_amd as sd
    from sdslam_amd import build
    build.build()
    out = subprocess.run([_build(tmp_path, sd)], capture_output=True, text=True)
    assert out.returncode == 0 and "facade sim3 ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_compute_sim3_candidates(oracle, tmp_path):
    import sdslam_amd as sd
    from sdslam_amd import build
    build.build()
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    n = len(KINDS)
    cur, ref = SC.images()
    cur, ref = cur[:n], ref[:n]
    oct1, n1, oct2, n2 = SC.oracle_keypoints(oracle, PYR)
    rng = np.random.default_rng(21)
    slots = [SC.make_slot(rng, kind, oct1[b], n1[b], oct2[b], n2[b]) for b, kind in enumerate(KINDS)]
    rand = rng.integers(0, 2 ** 31, size=(n, SC.RAND_PER_SLOT), dtype=np.int64).astype(np.int32)
    # the restatement, driven like LoopClosing::ComputeSim3 with every candidate accepted
    solvers = [SC.solver(sl, rand[b], PYR, False) for b, sl in enumerate(slots)]
    gone, winner, want = [False] * n, -1, None
    while winner < 0 and not all(gone):
        results = [None if gone[b] else sv.iterate(5) for b, sv in enumerate(solvers)]
        for b, res in enumerate(results):
            if res is None:
                continue
            if res[1]:
                gone[b] = True
            if res[0][3, 3] != 0:
                winner, want = b, res
                break
    assert winner == 1 and want[3] == int(slots[1]["planted"].sum())
    cfg = SC.PYR[PYR]
    inp, outp = str(tmp_path / "sim3.in"), str(tmp_path / "sim3.out")
    with open(inp, "wb") as f:
        f.write(np.array([SC.W, SC.H, cfg[0], cfg[2], n, SC.RAND_PER_SLOT], np.int32).tobytes())
        f.write(np.array([cfg[1], *SC.K], np.float32).tobytes())
        f.write(np.ascontiguousarray(cur).tobytes())
        f.write(np.ascontiguousarray(ref).tobytes())
        f.write(np.stack([np.asarray(s["kf2"]["T"]).T.reshape(16) for s in slots]).tobytes())
        f.write(np.stack([np.asarray(s["kf1"]["T"]).T.reshape(16) for s in slots]).tobytes())
        f.write(np.stack([s["kf1"]["has_mp"] for s in slots]).astype(np.uint8).tobytes())
        f.write(np.stack([s["kf2"]["has_mp"] for s in slots]).astype(np.uint8).tobytes())
        f.write(np.stack([s["kf1"]["Xw"] for s in slots]).astype(np.float64).tobytes())
        f.write(np.stack([s["kf2"]["Xw"] for s in slots]).astype(np.float64).tobytes())
        f.write(np.stack([s["matches12"] for s in slots]).astype(np.int32).tobytes())
        f.write(rand.tobytes())
    out = subprocess.run([_build(tmp_path, sd), inp, outp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ran" in out.stdout, (out.returncode, out.stdout, out.stderr)
    raw = open(outp, "rb").read()
    assert len(raw) == 4 + 4 * n + 4 + 128 + 4
    got_winner = int(np.frombuffer(raw, np.int32, 1, 0)[0])
    its = np.frombuffer(raw, np.int32, n, 4)
    n_inl = int(np.frombuffer(raw, np.int32, 1, 4 + 4 * n)[0])
    T12 = np.frombuffer(raw, np.float64, 16, 8 + 4 * n).reshape(4, 4).T
    scale = float(np.frombuffer(raw, np.float32, 1, 8 + 4 * n + 128)[0])
    assert got_winner == 1
    assert its.tolist() == [sv.iterations for sv in solvers]
    assert n_inl == want[3]
    assert np.abs(T12 - want[0]).max() <= 1e-5 and abs(scale - float(solvers[1].best_s)) <= 1e-5 * scale
