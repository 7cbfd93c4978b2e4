"""The one reference translation unit that compiles without OpenCV/Eigen -- src/extra/utils.cc
(SD_SLAM::Random) -- pins the oracle's restatement of the RANSAC draw.  Its answers to a fixed sequence of calls
(glibc's default state, srand(1); `sizes` from default_rng(0)) are stored in tests/golden/ref_random_srand1.npz;
where the binary is built (oracle/Makefile `ref` -> oracle/_ref/libref_utils.so) it is called live as well."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_utils.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_random_srand1.npz")


def test_random_matches_reference_binary():
    from sdslam_amd.synth import glibc_rand_stream
    g = np.load(GOLDEN)
    mn, sizes, values = int(g["min"]), g["sizes"], g["values"]
    assert len(sizes) == len(values) == 4000
    np.testing.assert_array_equal(sizes, np.random.default_rng(0).integers(1, 2000, size=4000))
    rs = glibc_rand_stream(4000)               # the reference never seeds: default state == seed 1
    exp = [int((float(r) / (2147483647.0 + 1.0)) * d + mn) for r, d in zip(rs.tolist(), sizes.tolist())]   # oracle / device formula
    assert exp == values.tolist()
    if os.path.exists(REF):                    # the reference binary itself, where it is built
        ref = C.CDLL(REF)
        fn = ref._ZN7SD_SLAM6RandomEii          # int SD_SLAM::Random(int, int)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_int]
        libc = C.CDLL("libc.so.6")
        libc.srand(1)
        assert [fn(mn, mn + d - 1) for d in sizes.tolist()] == values.tolist()
