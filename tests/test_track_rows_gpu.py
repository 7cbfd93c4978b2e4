"""GPU: what sd_track_create leaves in the per-slot buffers, and the row copies between a caller's pitch `cap` and the
device's pitch (the keypoint capacity K) in every getter and setter that takes a `cap`.  No extraction: none of these calls
needs frames."""

import numpy as np
import pytest

from sdslam_amd import capi

pytestmark = pytest.mark.gpu
B, M = 3, 64
SENT_I, SENT_U8, SENT_F = 0x5A5A5A5, 0xA5, 777.0


@pytest.fixture
def rows():
    """A fresh tracker per test: each reads what creation left, or what it set itself."""
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    cur = sd.ORBextractor(100, 1.2, 8, 20, 64, 48, B)
    ref = sd.ORBextractor(100, 1.2, 8, 20, 64, 48, B)
    trk = sd.Tracker(cur, ref, max_points=M, max_batch=B, pnp_max_iterations=4)
    L = capi.lib()
    yield dict(trk=trk, L=L, K=trk.cap)
    trk.close()
    cur.close()
    ref.close()


def _ok(rows, rc):
    assert rc == 0, rows["L"].sd_last_error().decode()


def _wide(rows, dtype, sentinel):
    return np.full((B, rows["K"] + 7), sentinel, dtype)


def test_initial_fills_and_getter_pitch(rows):
    trk, L, K = rows["trk"], rows["L"], rows["K"]
    p, h, cap = capi._p, trk.h, K + 7

    def check(a, value, sentinel):
        assert (a[:, :K] == value).all(), a[:, :K]
        assert (a[:, K:] == sentinel).all(), a[:, K:]

    a = _wide(rows, np.int32, SENT_I)
    _ok(rows, L.sd_track_get_matches(h, 0, B, p(a), cap, None))
    check(a, -1, SENT_I)                                   # cur_match
    a = _wide(rows, np.int32, SENT_I)
    _ok(rows, L.sd_track_get_local(h, 0, B, p(a), cap, None, None, None, None, None))
    check(a, -1, SENT_I)                                   # lm_match
    a = _wide(rows, np.int32, SENT_I)
    _ok(rows, L.sd_track_get_local_map(h, 0, B, p(a), cap, None))
    check(a, -1, SENT_I)                                   # un_match
    a = _wide(rows, np.int32, SENT_I)
    _ok(rows, L.sd_track_get_point_matches(h, 0, B, p(a), cap, None))
    check(a, 0, SENT_I)                                    # sp_match
    a = _wide(rows, np.uint8, SENT_U8)
    _ok(rows, L.sd_track_get_pose_opt(h, 0, B, None, p(a), cap, None))
    check(a, 0, SENT_U8)                                   # po_outlier
    a = _wide(rows, np.uint8, SENT_U8)
    _ok(rows, L.sd_track_get_pnp(h, 0, B, None, p(a), cap, None))
    check(a, 0, SENT_U8)                                   # pnp_inliers
    u, d = _wide(rows, np.float32, SENT_F), _wide(rows, np.float32, SENT_F)
    _ok(rows, L.sd_track_get_stereo(h, 0, B, p(u), p(d), cap))
    check(u, -1.0, SENT_F)
    check(d, -1.0, SENT_F)
    assert (trk.get_last(0, B)["ids"] == -1).all()


def test_null_outputs_fill_only_the_one_asked_for(rows):
    """Every optional output NULL except one, in turn: SD_OK, and that one holds the buffer's content (zeros after creation,
    -1 in the local match rows)."""
    trk, L, K = rows["trk"], rows["L"], rows["K"]
    h = trk.h
    i32, f32, f64, u8 = np.int32, np.float32, np.float64, np.uint8
    cases = [
        (L.sd_track_get_align, lambda o: (h, 0, B, *o), [((B, 16), f64, 0), ((B,), f64, 0), ((B,), i32, 0), ((B, 16), i32, 0), ((B,), f64, 0)]),
        (L.sd_track_get_pose_opt, lambda o: (h, 0, B, o[0], o[1], K, o[2]), [((B, 16), f64, 0), ((B, K), u8, 0), ((B, 8), i32, 0)]),
        (L.sd_track_get_pnp, lambda o: (h, 0, B, o[0], o[1], K, o[2]), [((B, 16), f32, 0), ((B, K), u8, 0), ((B, 8), i32, 0)]),
        (L.sd_track_get_local, lambda o: (h, 0, B, o[0], K, *o[1:]),
         [((B, K), i32, -1), ((B,), i32, 0), ((B, M), u8, 0), ((B, M, 3), f32, 0), ((B, M), i32, 0), ((B, M), f32, 0)]),
    ]
    for fn, args, outs in cases:
        for k, (shape, dtype, value) in enumerate(outs):
            a = np.full(shape, 99, dtype)
            o = [None] * len(outs)
            o[k] = capi._p(a)
            _ok(rows, fn(*args(o)))
            assert (a == value).all(), (fn.__name__, k, a)


def test_narrow_setter_wide_getter_offset_slot(rows):
    trk, L, K = rows["trk"], rows["L"], rows["K"]
    p, h = capi._p, trk.h
    rng = np.random.default_rng(5)
    narrow = K - 5
    m_in = np.full((2, narrow), -1, np.int32)
    for f, count in enumerate((M, 40)):                   # distinct map point indices in [0, 64), -1 elsewhere
        m_in[f, rng.permutation(narrow)[:count]] = rng.permutation(M)[:count]
    _ok(rows, L.sd_track_set_matches(h, 1, 2, p(m_in), narrow))
    a, nm = _wide(rows, np.int32, SENT_I), np.full(B, SENT_I, np.int32)
    _ok(rows, L.sd_track_get_matches(h, 0, B, p(a), K + 7, p(nm)))
    assert (a[0, :K] == -1).all()
    assert np.array_equal(a[1:, :narrow], m_in)
    assert (a[1:, narrow:K] == -1).all()
    assert (a[:, K:] == SENT_I).all()
    assert list(nm) == [0, M, 40]

    u_in = rng.uniform(0.0, 60.0, (2, narrow)).astype(np.float32)
    _ok(rows, L.sd_track_set_uright(h, 1, 2, p(u_in), narrow))
    u, d = _wide(rows, np.float32, SENT_F), _wide(rows, np.float32, SENT_F)
    _ok(rows, L.sd_track_get_stereo(h, 0, B, p(u), p(d), K + 7))
    assert (u[0, :K] == -1.0).all()
    assert np.array_equal(u[1:, :narrow], u_in)
    assert (u[1:, narrow:K] == -1.0).all()
    assert (u[:, K:] == SENT_F).all()
    assert (d[:, :K] == -1.0).all() and (d[:, K:] == SENT_F).all()
