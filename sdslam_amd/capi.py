"""ctypes binding of libsdslam_hip.so (C ABI: include/sdslam_hip.h).

Host-side mirror of the reference interface for the hot path: the class/method names follow
the reference (`ORBextractor.__call__` == `ORBextractor::operator()`, reference
src/ORBextractor.h:38-70).  Nothing here computes: every method forwards to the HIP library
and raises SdError on a non-zero status.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

SD_OK = 0


class SdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sdslam_hip status {code}: {msg}")
        self.code = code


def lib_path() -> str:
    # SD_LIB: an instrumented build of the same library (profiling tools only; e.g. -DSD_PNP_PROF stage timers)
    return os.environ.get("SD_LIB") or os.path.join(_HERE, "libsdslam_hip.so")


# name -> (restype, [argtypes]), in the order of include/sdslam_hip.h: the one place a C signature is written down.  lib()
# applies every row at load; tests/test_capi_signatures_cpu.py holds the rows to the header.
_I, _F, _D, _Z, _P, _S = C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_void_p, C.c_char_p
_PP, _PI = C.POINTER(C.c_void_p), C.POINTER(C.c_int)        # a handle / an int the call returns through byref()

_SIGNATURES = {
    # status, version, process-wide options
    "sd_last_error": (_S, []),
    "sd_device_count": (_I, []),
    "sd_version": (_S, []),
    "sd_set_option": (_I, [_S, _I]),
    "sd_get_option": (_I, [_S, _PI]),
    "sd_option_count": (_I, []),
    "sd_option_name": (_S, [_I]),
    # ORB extractor
    "sd_orb_create": (_I, [_I, _F, _I, _I, _I, _I, _I, _I, _PP]),
    "sd_orb_destroy": (None, [_P]),
    "sd_orb_levels": (_I, [_P]),
    "sd_orb_scale_tables": (_I, [_P, _P, _P, _P, _P]),
    "sd_orb_features_per_level": (_I, [_P, _P]),
    "sd_orb_plan_info": (_I, [_I, _F, _I, _I, _I, _I, _P, _P, _I, _P, _P]),
    "sd_orb_plan_row_blocks": (_I, [_I, _F, _I, _I, _I, _I, _I, _P, _I, _P]),
    "sd_orb_extract": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "sd_orb_extract_batch": (_I, [_P, _P, _I, _I, _I, _I, _Z, _P, _P, _I, _P]),
    "sd_orb_extract_batch_device": (_I, [_P, _P, _I, _I, _I, _I, _Z]),
    "sd_orb_download": (_I, [_P, _I, _I, _P, _P, _I, _P]),
    "sd_orb_set_distortion": (_I, [_P, _F, _F, _F, _F, _F, _F, _F, _F, _F]),
    "sd_orb_download_undistorted": (_I, [_P, _I, _I, _P, _I]),
    "sd_orb_level_info": (_I, [_P, _I, _P, _P]),
    "sd_orb_level_copy": (_I, [_P, _I, _I, _I, _P, _I]),
    "sd_orb_debug_blurred": (_I, [_P, _I, _I, _P, _I]),
    "sd_orb_debug_cell_counts": (_I, [_P, _I, _I, _P, _I, _P]),
    "sd_orb_debug_level_keys": (_I, [_P, _I, _I, _P, _I, _P]),
    "sd_debug_orb_set_keypoints": (_I, [_P, _I, _I, _P, _P, _P, _I]),
    "sd_orb_set_stream": (_I, [_P, _P]),
    "sd_orb_stream_fence": (_I, [_P, _P, _I]),
    "sd_orb_sync": (_I, [_P]),
    "sd_orb_set_profiling": (_I, [_P, _I]),
    "sd_orb_num_stages": (_I, []),
    "sd_orb_stage_name": (_S, [_I]),
    "sd_orb_stage_ms": (_I, [_P, _P, _I]),
    "sd_orb_stage_bytes": (_I, [_P, _P, _I]),
    # device / pinned memory helpers
    "sd_dev_alloc": (_I, [_Z, _PP]),
    "sd_host_alloc": (_I, [_Z, _PP]),
    "sd_host_free": (_I, [_P]),
    "sd_dev_free": (_I, [_P]),
    "sd_dev_upload": (_I, [_P, _P, _Z]),
    "sd_dev_download": (_I, [_P, _P, _Z]),
    # batched tracking context
    "sd_track_create": (_I, [_P, _P, _I, _I, _I, _PP]),
    "sd_track_destroy": (None, [_P]),
    "sd_track_set_camera": (_I, [_P, _F, _F, _F, _F, _F, _F, _F, _F, _F]),
    "sd_track_set_last": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_set_poses": (_I, [_P, _I, _I, _P, _P]),
    "sd_track_set_rand": (_I, [_P, _I, _I, _P, _I]),
    "sd_track_set_uright": (_I, [_P, _I, _I, _P, _I]),
    "sd_track_stereo_from_depth": (_I, [_P, _I, _P, _I, _I, _I, _Z]),
    "sd_track_get_stereo": (_I, [_P, _I, _I, _P, _P, _I]),
    "sd_track_stereo_from_depth_device": (_I, [_P, _I, _P, _I, _I, _I, _I, _Z, _F]),
    "sd_track_set_local": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_match_local": (_I, [_P, _I, _F, _F, _F]),
    "sd_track_get_local": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "sd_track_pose_opt": (_I, [_P, _I, _I]),
    "sd_track_get_pose_opt": (_I, [_P, _I, _I, _P, _P, _I, _P]),
    "sd_track_set_current_broadcast": (_I, [_P, _I]),
    "sd_track_relocalize": (_I, [_P, _I, _I, _F, _I, _I, _I, _P, _P]),
    "sd_track_detect_loop": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P]),
    "sd_track_with_motion_model": (_I, [_P, _I, _I, _F, _I, _I, _I]),
    "sd_track_get_tracked": (_I, [_P, _I, _I, _P]),
    "sd_track_local_map": (_I, [_P, _I, _F, _F, _F, _I]),
    "sd_track_get_local_map": (_I, [_P, _I, _I, _P, _I, _P]),
    "sd_track_set_point_flags": (_I, [_P, _I, _I, _P, _P, _I]),
    "sd_track_search_by_points": (_I, [_P, _I, _F, _I]),
    "sd_track_get_point_matches": (_I, [_P, _I, _I, _P, _I, _P]),
    "sd_track_set_sim3_points": (_I, [_P, _I, _I, _P, _P, _I]),
    "sd_track_set_point_matches": (_I, [_P, _I, _I, _P, _I]),
    "sd_track_sim3": (_I, [_P, _I, _I, _D, _I, _I, _I]),
    "sd_track_sim3_iterate": (_I, [_P, _I, _I]),
    "sd_track_get_sim3": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "sd_track_set_uright_ref": (_I, [_P, _I, _I, _P, _I]),
    "sd_track_set_f12": (_I, [_P, _I, _I, _P]),
    "sd_track_search_for_triangulation": (_I, [_P, _I, _I, _I]),
    "sd_track_get_triangulation_matches": (_I, [_P, _I, _I, _P, _I, _P, _P, _P]),
    "sd_debug_search_for_triangulation": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "sd_track_set_tri_depth": (_I, [_P, _I, _I, _I, _P, _I]),
    "sd_track_set_tri_median_depth": (_I, [_P, _I, _I, _P]),
    "sd_track_triangulate": (_I, [_P, _I, _I]),
    "sd_track_get_triangulated": (_I, [_P, _I, _I, _P, _P, _P, _I, _P]),
    "sd_track_get_new_points": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "sd_debug_triangulate": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _F, _I, _F, _P, _P, _P]),
    "sd_track_append_new_points": (_I, [_P, _I, _I, _I]),
    "sd_track_get_appended": (_I, [_P, _I, _I, _P, _P, _P]),
    "sd_track_get_local_points": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "sd_track_set_fuse_scw": (_I, [_P, _I, _I, _P]),
    "sd_track_fuse": (_I, [_P, _I, _I, _I, _F, _I]),
    "sd_track_get_fuse": (_I, [_P, _I, _I, _P, _P, _I, _P]),
    "sd_debug_fuse": (_I, [_I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _F, _F, _I, _I, _P, _P, _P, _P]),
    "sd_track_set_observations": (_I, [_P, _I, _P, _P, _P, _P, _P, _P]),
    "sd_track_refresh_points": (_I, [_P, _I, _I]),
    "sd_track_get_refreshed": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "sd_debug_refresh_points": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_set_ba_keyframes": (_I, [_P, _I, _P, _I]),
    "sd_track_local_ba": (_I, [_P, _I, _I]),
    "sd_track_get_local_ba": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I]),
    "sd_debug_local_ba": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_global_ba": (_I, [_P, _I, _I, _I, _I]),
    "sd_track_get_global_ba": (_I, [_P, _P, _P, _P, _P, _P, _I]),
    "sd_debug_global_ba": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "sd_debug_ldlt": (_I, [_I, _P, _P, _P, _P]),
    "sd_track_cull_keyframes": (_I, [_P, _I, _P, _P, _I, _F]),
    "sd_track_get_culled": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I]),
    "sd_track_erase_observations": (_I, [_P, _I]),
    "sd_track_get_erased": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I]),
    "sd_debug_cull_keyframes": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P, _P]),
    "sd_debug_erase_observations": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_align": (_I, [_P, _I, _I]),
    "sd_track_match": (_I, [_P, _I, _F, _I, _I]),
    "sd_track_pnp": (_I, [_P, _I, _D, _I, _I, _I, _F, _F, _I]),
    "sd_track_pnp_iterate": (_I, [_P, _I, _I]),
    "sd_track_set_matches": (_I, [_P, _I, _I, _P, _I]),
    "sd_track_get_align": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "sd_track_get_matches": (_I, [_P, _I, _I, _P, _I, _P]),
    "sd_track_get_pnp": (_I, [_P, _I, _I, _P, _P, _I, _P]),
    "sd_debug_pnp_prof": (_I, [_P, _I]),          # the three *_prof: called by tools/prof_pnp.py and tools/prof_select.py
    "sd_debug_align_prof": (_I, [_P, _I]),
    "sd_debug_sel_prof": (_I, [_P, _I]),
    "sd_debug_epnp": (_I, [_I, _P, _P, _D, _D, _D, _D, _P, _P, _P]),
    "sd_track_debug_read": (_I, [_P, _I, _I, _P, _Z]),
    "sd_track_debug_features_in_area": (_I, [_P, _I, _F, _F, _F, _I, _I, _P, _I, _P, _P]),
    "sd_track_pack_records": (_I, [_P, _I, _I, _P]),
    # sequential tracking, motion and IMU models
    "sd_track_set_map_ids": (_I, [_P, _I, _I, _I, _P, _I]),
    "sd_track_advance": (_I, [_P, _I, _I]),
    "sd_track_set_prior": (_I, [_P, _I, _I, _P, _I]),
    "sd_track_get_last": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_get_extractors": (_I, [_P, _PP, _PP]),
    "sd_track_close_points": (_I, [_P, _I, _I, _F]),
    "sd_track_get_close_points": (_I, [_P, _I, _I, _P]),
    "sd_track_motion_predict": (_I, [_P, _I, _D]),
    "sd_track_motion_update": (_I, [_P, _I, _I]),
    "sd_track_motion_restart": (_I, [_P, _I, _I]),
    "sd_track_get_motion": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "sd_track_set_motion": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "sd_track_set_sensor_model": (_I, [_P, _I]),
    "sd_track_get_sensor_model": (_I, [_P, _PI]),
    "sd_track_set_measurements": (_I, [_P, _I, _I, _P]),
    "sd_track_get_imu": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "sd_track_set_imu": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "sd_track_stream_fence": (_I, [_P, _P, _I]),
    "sd_track_set_profiling": (_I, [_P, _I]),
    "sd_track_stage_ms": (_I, [_P, _P, _I]),
    # RGB-D map point creation and the keyframe decision
    "sd_track_set_next_map_id": (_I, [_P, _I, _I, _P]),
    "sd_track_stereo_init": (_I, [_P, _I, _I]),
    "sd_track_set_keyframe_state": (_I, [_P, _I, _I, _P]),
    "sd_track_need_keyframe": (_I, [_P, _I, _I, _I, _I, _I]),
    "sd_track_set_keyframe_flags": (_I, [_P, _I, _I, _P]),
    "sd_track_get_keyframe_flags": (_I, [_P, _I, _I, _P]),
    "sd_track_create_keyframe_points": (_I, [_P, _I, _I, _F, _I, _I]),
    "sd_track_get_created": (_I, [_P, _I, _I, _P, _P, _P, _P, _I]),
    "sd_hamming": (_I, [_P, _P]),
}

# Header prototypes left without a row, with the reason: nothing in Python calls them.
_UNBOUND = ("sd_track_set_local_view", "sd_track_match_local_view")      # the caller's own isInFrustum results: C++ facade only

_lib = None


def lib():
    """Load libsdslam_hip.so and declare every _SIGNATURES row on it.  Fails loudly if it is not built or lacks a row's name (no fallback)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise SdError(-1, f"{p} is missing: build it with `python -m sdslam_amd.build` "
                              "(hipcc, gfx950). There is no CPU fallback.")
        L = C.CDLL(p)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, name)           # AttributeError "undefined symbol" for a name the library lacks
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


def _check(rc):
    if rc != SD_OK:
        raise SdError(rc, lib().sd_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def set_option(name: str, value: int):
    """sd_set_option: process-wide tuning / test switch (include/sdslam_hip.h lists them; the library reads no environment)."""
    _check(lib().sd_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_int(0)
    _check(lib().sd_get_option(name.encode(), C.byref(v)))
    return v.value


def option_names():
    L = lib()
    return [L.sd_option_name(i).decode() for i in range(L.sd_option_count())]


class options:
    """with options({"extract.use_graph": 1}): ... -- set for the block, restore afterwards."""

    def __init__(self, values):
        self.values, self.saved = dict(values), {}

    def __enter__(self):
        for k, v in self.values.items():
            self.saved[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            set_option(k, v)
        return False


def device_count() -> int:
    return int(lib().sd_device_count())


def hamming(a: np.ndarray, b: np.ndarray) -> int:
    """ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:1459-1473)."""
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    assert a.size == 32 and b.size == 32
    return int(lib().sd_hamming(_p(a), _p(b)))


def plan_info(nfeatures, scale_factor, nlevels, th_fast, w, h):
    """Geometry the extractor uses for a w x h frame (host-only; no GPU needed)."""
    lv = np.zeros((nlevels, 8), np.int32)
    zones = np.zeros((65536, 6), np.int32)
    n = C.c_int32()
    nbytes = C.c_uint64()
    _check(lib().sd_orb_plan_info(nfeatures, scale_factor, nlevels, th_fast, w, h, _p(lv), _p(zones), len(zones),
                                  C.byref(n), C.byref(nbytes)))
    return dict(levels=lv, cells=zones[:n.value].copy(), bytes_per_frame=nbytes.value)


def plan_row_blocks(nfeatures, scale_factor, nlevels, th_fast, w, h, level):
    """Row blocks [n, 4] = {y0, rows, first source row, carries border rows} k_pyr_rows walks on that level (host-only);
    empty where k_pyr_split resizes the level."""
    out = np.zeros((4096, 4), np.int32)
    n = C.c_int32()
    _check(lib().sd_orb_plan_row_blocks(nfeatures, scale_factor, nlevels, th_fast, w, h, level, _p(out), len(out), C.byref(n)))
    return out[:n.value].copy()


def pinned_array(shape, dtype=np.uint8):
    """numpy array over page-locked host memory (sd_host_alloc); keep the returned owner alive."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    L = lib()
    p = C.c_void_p()
    _check(L.sd_host_alloc(n, C.byref(p)))
    buf = (C.c_uint8 * n).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype).reshape(shape)

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr

        def __del__(self):
            try:
                L.sd_host_free(self.ptr)
            except Exception:
                pass
    return arr, _Owner(p)


class DeviceBuffer:
    """Raw HBM allocation (for harnesses that stage inputs on the device themselves)."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        self.nbytes = nbytes
        _check(lib().sd_dev_alloc(nbytes, C.byref(self.ptr)))

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(lib().sd_dev_upload(self.ptr, _p(arr), arr.nbytes))

    def free(self):
        if self.ptr:
            lib().sd_dev_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ORBextractor:
    """Mirror of SD_SLAM::ORBextractor (reference src/ORBextractor.h:38-70) over sd_orb_*."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, thFAST=20, max_w=640, max_h=480, max_batch=1,
                 device=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.nfeatures, self.nlevels, self.max_batch = nfeatures, nlevels, max_batch
        _check(self.L.sd_orb_create(nfeatures, scaleFactor, nlevels, thFAST, max_w, max_h, max_batch, device,
                                    C.byref(self.h)))
        self.cap = nfeatures

    def close(self):
        if self.h:
            self.L.sd_orb_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- getters (GetLevels / GetScaleFactors / ...) ---
    def GetLevels(self):
        return self.nlevels

    def _tables(self):
        n = self.nlevels
        arrs = [np.zeros(n, np.float32) for _ in range(4)]
        _check(self.L.sd_orb_scale_tables(self.h, *[_p(a) for a in arrs]))
        return arrs

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        q = np.zeros(self.nlevels, np.int32)
        _check(self.L.sd_orb_features_per_level(self.h, _p(q)))
        return q

    # --- operator() ---
    def __call__(self, image: np.ndarray):
        """(keypoints[KP_DTYPE], descriptors[N,32]) of one grey frame; pyramid stays on device."""
        image = np.ascontiguousarray(image, np.uint8)
        if image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        k, d, n = self.extract_batch(image[None])
        return k[0, :n[0]].copy(), d[0, :n[0]].copy()

    def extract_batch(self, images: np.ndarray):
        images = np.ascontiguousarray(images, np.uint8)
        B, H, W = images.shape
        kps = np.zeros((B, self.cap), KP_DTYPE)
        desc = np.zeros((B, self.cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        _check(self.L.sd_orb_extract_batch(self.h, _p(images), B, W, H, images.strides[1], images.strides[0],
                                           _p(kps), _p(desc), self.cap, _p(n)))
        return kps, desc, n

    def extract_batch_device(self, d_ptr, B, W, H, stride=None, frame_stride=None):
        stride = stride or W
        frame_stride = frame_stride or stride * H
        _check(self.L.sd_orb_extract_batch_device(self.h, d_ptr, B, W, H, stride, frame_stride))

    def download(self, frame0=0, n_frames=1):
        kps = np.zeros((n_frames, self.cap), KP_DTYPE)
        desc = np.zeros((n_frames, self.cap, 32), np.uint8)
        n = np.zeros(n_frames, np.int32)
        _check(self.L.sd_orb_download(self.h, frame0, n_frames, _p(kps), _p(desc), self.cap, _p(n)))
        return kps, desc, n

    def set_distortion(self, fx, fy, cx, cy, k1, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        """Frame::UndistortKeyPoints parameters (mK as CV_32F, mDistCoef); k1 == 0 disables."""
        _check(self.L.sd_orb_set_distortion(self.h, fx, fy, cx, cy, k1, k2, p1, p2, k3))

    def download_undistorted(self, frame0=0, n_frames=1):
        kps = np.zeros((n_frames, self.cap), KP_DTYPE)
        _check(self.L.sd_orb_download_undistorted(self.h, frame0, n_frames, _p(kps), self.cap))
        return kps

    # --- pyramid / diagnostics ---
    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _check(self.L.sd_orb_level_info(self.h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def level(self, level, frame=0, padded=False):
        w, h = self.level_size(level)
        if padded:
            w, h = w + 38, h + 38
        out = np.zeros((h, w), np.uint8)
        _check(self.L.sd_orb_level_copy(self.h, frame, level, int(padded), _p(out), w))
        return out

    def blurred(self, level, frame=0):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _check(self.L.sd_orb_debug_blurred(self.h, frame, level, _p(out), w))
        return out

    def cell_counts(self, level, frame=0):
        out = np.zeros(4096, np.int32)
        n = C.c_int()
        _check(self.L.sd_orb_debug_cell_counts(self.h, frame, level, _p(out), 4096, C.byref(n)))
        return out[:n.value].copy()

    def level_keys(self, level, frame=0):
        out = np.zeros(max(self.cap, 1), np.uint32)
        n = C.c_int()
        _check(self.L.sd_orb_debug_level_keys(self.h, frame, level, _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def set_keypoints(self, frame0, kps_list, desc_list):
        """sd_debug_orb_set_keypoints: plant per-frame keypoints [n_f] (KP_DTYPE) and descriptors [n_f, 32] in the slots from
        frame0 on, as an extraction would have left them (needs one earlier extraction for the geometry; refuses a distortion)."""
        cap = max([len(k) for k in kps_list] + [1])
        kps, n = _padded(kps_list, (len(kps_list), cap), KP_DTYPE)
        desc, nd = _padded([np.asarray(d, np.uint8).reshape(-1, 32) for d in desc_list], (len(desc_list), cap, 32), np.uint8)
        assert np.array_equal(n, nd)
        _check(self.L.sd_debug_orb_set_keypoints(self.h, frame0, len(n), _p(n), _p(kps), _p(desc), cap))

    # --- stream / timing ---
    def set_stream(self, stream_ptr):
        _check(self.L.sd_orb_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def stream_fence(self, stream_ptr, direction):
        """sd_orb_stream_fence: 0 = the caller's stream waits for the extractions queued so far, 1 = later extractions wait for it."""
        _check(self.L.sd_orb_stream_fence(self.h, C.c_void_p(stream_ptr), direction))

    def sync(self):
        _check(self.L.sd_orb_sync(self.h))

    def set_profiling(self, on=True):
        _check(self.L.sd_orb_set_profiling(self.h, int(on)))

    def stage_names(self):
        return [self.L.sd_orb_stage_name(i).decode() for i in range(self.L.sd_orb_num_stages())]

    def stage_ms(self):
        n = self.L.sd_orb_num_stages()
        ms = np.zeros(n, np.float32)
        _check(self.L.sd_orb_stage_ms(self.h, _p(ms), n))
        return ms

    def stage_bytes(self):
        n = self.L.sd_orb_num_stages()
        b = np.zeros(n, np.float64)
        _check(self.L.sd_orb_stage_bytes(self.h, _p(b), n))
        return b


def _padded(items, shape, dtype, fill=0):
    """Per-frame arrays of differing length -> (one [n, M, ...] array of `shape`, row i = items[i] then `fill`; the lengths, int32)."""
    a, lens = np.full(shape, fill, dtype), np.zeros(shape[0], np.int32)
    for i, v in enumerate(items):
        v = np.asarray(v, dtype)
        a[i, :len(v)] = v
        lens[i] = len(v)
    return a, lens


def _cm(T):
    """4x4 (row-major math) -> 16 doubles column-major (Eigen::Matrix4d::data())."""
    return np.ascontiguousarray(np.asarray(T, np.float64).T).ravel()


def _from_cm(v):
    return np.asarray(v, np.float64).reshape(4, 4).T.copy()


class Tracker:
    """Batched TrackWithMotionModel context over two resident extractors (sd_track_*):
    ImageAlign.ComputePose -> ORBmatcher.SearchByProjection -> PnPsolver.iterate
    (reference src/Tracking.cc:654-718)."""

    MODE_FRAME, MODE_KF, MODE_KF_FAST, MODE_KFKF = 0, 1, 2, 3

    def __init__(self, cur: ORBextractor, ref: ORBextractor, max_points=1000, max_batch=1, pnp_max_iterations=300):
        self.L = lib()
        self.cur, self.ref = cur, ref
        self.M, self.B, self.cap = max_points, max_batch, cur.cap
        self.h = C.c_void_p()
        _check(self.L.sd_track_create(cur.h, ref.h, max_points, max_batch, pnp_max_iterations, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.sd_track_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_rows(self, fn, frame0, dtype, *rows, pitch=True):
        """A row setter fn(h, frame0, n, rows..., [cap']): `rows` are [n, cap'] arrays of one shape, cap' is passed with `pitch`."""
        a = [np.ascontiguousarray(r, dtype) for r in rows]
        assert a[0].ndim == 2 and all(r.shape == a[0].shape for r in a)
        _check(fn(self.h, frame0, a[0].shape[0], *[_p(r) for r in a], *([a[0].shape[1]] if pitch else [])))

    def set_camera(self, fx, fy, cx, cy, bf=0.0, bounds=(0.0, 640.0, 0.0, 480.0)):
        _check(self.L.sd_track_set_camera(self.h, fx, fy, cx, cy, bf, *[float(b) for b in bounds]))

    def set_last(self, frame0, cases):
        """cases: list of dict(valid, Xw, desc, octave, angle, obs) (one per frame)."""
        n, M = len(cases), self.M
        assert all(len(c["valid"]) <= M for c in cases)
        cols = [_padded([c[k] for c in cases], (n, M) + tail, dt) for k, tail, dt in (
            ("valid", (), np.uint8), ("Xw", (3,), np.float64), ("desc", (32,), np.uint8), ("octave", (), np.int32),
            ("angle", (), np.float32), ("obs", (), np.int32))]
        n_last = cols[0][1]
        assert all((k == n_last).all() for _, k in cols)          # a frame's arrays have one length
        _check(self.L.sd_track_set_last(self.h, frame0, n, _p(n_last), *[_p(a) for a, _ in cols]))

    def set_poses(self, frame0, T_ref_list, T_cur_list):
        n = len(T_ref_list)
        a = np.stack([_cm(T) for T in T_ref_list])
        b = np.stack([_cm(T) for T in T_cur_list])
        _check(self.L.sd_track_set_poses(self.h, frame0, n, _p(a), _p(b)))

    def set_rand(self, frame0, rand_values):
        self._set_rows(self.L.sd_track_set_rand, frame0, np.int32, rand_values)

    def set_uright(self, frame0, uright):
        self._set_rows(self.L.sd_track_set_uright, frame0, np.float32, uright)

    def stereo_from_depth(self, depth):
        """Frame::ComputeStereoFromRGBD for the current frames; depth: [n, H, W] float32."""
        d = np.ascontiguousarray(depth, np.float32)
        _check(self.L.sd_track_stereo_from_depth(self.h, d.shape[0], _p(d), d.shape[2], d.shape[1], d.shape[2], d.shape[1] * d.shape[2]))

    DEPTH_F32, DEPTH_U16 = 0, 1

    def stereo_from_depth_device(self, d_ptr, dtype, W, H, stride=None, frame_stride=None, depth_map_factor=1.0, n_frames=None):
        """Frame::ComputeStereoFromRGBD on depth maps already in device memory at d_ptr, queued on the tracking stream (no host
        wait, no copy); dtype DEPTH_F32 / DEPTH_U16; strides in elements; depth_map_factor = DepthMapFactor (converted as
        Tracking::GrabImageRGBD does); n_frames defaults to the tracker's max_batch."""
        stride = stride or W
        frame_stride = frame_stride or stride * H
        n = self.B if n_frames is None else n_frames
        _check(self.L.sd_track_stereo_from_depth_device(self.h, n, d_ptr, int(dtype), W, H, stride, frame_stride, float(depth_map_factor)))

    def get_stereo(self, frame0, n):
        u = np.zeros((n, self.cap), np.float32)
        d = np.zeros((n, self.cap), np.float32)
        _check(self.L.sd_track_get_stereo(self.h, frame0, n, _p(u), _p(d), self.cap))
        return u, d

    def set_local(self, frame0, pts_list, kp_claimed=None):
        """pts_list: per frame dict(cand, Xw, normal, min_dist, max_dist, mf_max_dist, desc, obs) (TrackLocalMap's points)."""
        n, M = len(pts_list), self.M
        cols = [_padded([p[k] for p in pts_list], (n, M) + tail, dt) for k, tail, dt in (
            ("cand", (), np.uint8), ("Xw", (3,), np.float64), ("normal", (3,), np.float64), ("min_dist", (), np.float32),
            ("max_dist", (), np.float32), ("mf_max_dist", (), np.float32), ("desc", (32,), np.uint8), ("obs", (), np.int32))]
        kc = None if kp_claimed is None else _padded(kp_claimed, (n, self.cap), np.uint8)[0]
        _check(self.L.sd_track_set_local(self.h, frame0, n, _p(cols[0][1]), *[_p(a) for a, _ in cols], _p(kc)))

    def match_local(self, n_frames, th=1.0, nnratio=0.8, cos_limit=0.5):
        _check(self.L.sd_track_match_local(self.h, n_frames, float(th), float(nnratio), float(cos_limit)))

    def get_local(self, frame0, n):
        M = self.M
        lm = np.zeros((n, self.cap), np.int32)
        nm = np.zeros(n, np.int32)
        iv = np.zeros((n, M), np.uint8)
        pr = np.zeros((n, M, 3), np.float32)
        lv = np.zeros((n, M), np.int32)
        cs = np.zeros((n, M), np.float32)
        _check(self.L.sd_track_get_local(self.h, frame0, n, _p(lm), self.cap, _p(nm), _p(iv), _p(pr), _p(lv), _p(cs)))
        return dict(match=lm, n=nm, in_view=iv.astype(bool), proj=pr, level=lv, cos=cs)

    def pose_opt(self, n_frames, source=0):
        _check(self.L.sd_track_pose_opt(self.h, n_frames, int(source)))

    def get_pose_opt(self, frame0, n):
        T = np.zeros((n, 16))
        out = np.zeros((n, self.cap), np.uint8)
        info = np.zeros((n, 8), np.int32)
        _check(self.L.sd_track_get_pose_opt(self.h, frame0, n, _p(T), _p(out), self.cap, _p(info)))
        return dict(T=[_from_cm(t) for t in T], outlier=out.astype(bool), n_initial=info[:, 0], n_bad=info[:, 1], rounds=info[:, 2],
                    iterations=info[:, 3], lm_trials=info[:, 4], n_inliers=info[:, 5])

    def track_with_motion_model(self, n_frames, th=15.0, mono=True, align_mode=0, min_matches=20, min_inliers=10):
        """Tracking::TrackWithMotionModel (src/Tracking.cc:654-718) for the batch; align_mode 1 = against the reference
        keyframe (TrackReferenceKeyFrame), -1 = align_image_ off."""
        _check(self.L.sd_track_with_motion_model(self.h, n_frames, int(align_mode), th, int(mono), min_matches, min_inliers))

    def get_tracked(self, frame0, n):
        info = np.zeros((n, 4), np.int32)
        _check(self.L.sd_track_get_tracked(self.h, frame0, n, _p(info)))
        return dict(status=info[:, 0], nmatches=info[:, 1], nmatches_map=info[:, 2], retried=info[:, 3])

    def track_local_map(self, n_frames, th=1.0, nnratio=0.8, cos_limit=0.5, min_inliers=30):
        """Tracking::TrackLocalMap (src/Tracking.cc:720-751) on top of the frame-to-frame matches and the current pose."""
        _check(self.L.sd_track_local_map(self.h, n_frames, th, nnratio, cos_limit, min_inliers))

    def get_local_map(self, frame0, n):
        mm = np.zeros((n, self.cap), np.int32)
        info = np.zeros((n, 4), np.int32)
        _check(self.L.sd_track_get_local_map(self.h, frame0, n, _p(mm), self.cap, _p(info)))
        return dict(match=mm, status=info[:, 0], n_points=info[:, 1], n_inliers=info[:, 2], n_local=info[:, 3])

    def set_current_broadcast(self, cur_frame):
        """One current frame against many keyframes (-1: slot f <-> current frame f)."""
        _check(self.L.sd_track_set_current_broadcast(self.h, int(cur_frame)))

    def relocalize(self, n_keyframes, cur_frame=0, th=15.0, mono=True, min_matches=20, min_good=10):
        """Tracking::Relocalization (src/Tracking.cc:1064-1097), one batch slot per keyframe attempt."""
        win = C.c_int32(-1)
        st = np.zeros((n_keyframes, 3), np.int32)
        _check(self.L.sd_track_relocalize(self.h, n_keyframes, cur_frame, th, int(mono), min_matches, min_good, C.byref(win), _p(st)))
        return int(win.value), st

    def detect_loop(self, n_keyframes, cur_frame=0, excluded=None):
        """Candidate search of LoopClosing::DetectLoop (src/LoopClosing.cc:115-149)."""
        ex = None if excluded is None else np.ascontiguousarray(excluded, np.uint8)
        cand = np.zeros(n_keyframes, np.int32)
        n = C.c_int32(0)
        best = C.c_double(0)
        err = np.zeros(n_keyframes)
        _check(self.L.sd_track_detect_loop(self.h, n_keyframes, cur_frame, None if ex is None else _p(ex), _p(cand), n_keyframes,
                                           C.byref(n), C.byref(best), _p(err)))
        return dict(candidates=cand[:n.value].copy(), best_error=best.value, errors=err)

    def align(self, n_frames, mode=0):
        _check(self.L.sd_track_align(self.h, n_frames, mode))

    def match(self, n_frames, th=8.0, mono=True, check_ori=True):
        _check(self.L.sd_track_match(self.h, n_frames, th, int(mono), int(check_ori)))

    def pnp(self, n_frames, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991,
            n_iterations=None):
        n_iterations = max_iterations if n_iterations is None else n_iterations
        _check(self.L.sd_track_pnp(self.h, n_frames, probability, min_inliers, max_iterations, min_set, epsilon, th2,
                                   n_iterations))

    def pnp_iterate(self, n_frames, n_iterations):
        """A further PnPsolver::iterate(n_iterations) on the solvers the last pnp() call constructed."""
        _check(self.L.sd_track_pnp_iterate(self.h, n_frames, int(n_iterations)))

    def set_matches(self, frame0, cur_match):
        """CurrentFrame.mvpMapPoints of the slots from the caller: [n, cap'] indices into the last-frame arrays, -1 = NULL."""
        self._set_rows(self.L.sd_track_set_matches, frame0, np.int32, cur_match)

    def get_align(self, frame0, n):
        T = np.zeros((n, 16))
        err = np.zeros(n)
        ok = np.zeros(n, np.int32)
        iters = np.zeros((n, 16), np.int32)
        chi2 = np.zeros(n)
        _check(self.L.sd_track_get_align(self.h, frame0, n, _p(T), _p(err), _p(ok), _p(iters), _p(chi2)))
        return dict(T=[_from_cm(t) for t in T], error=err, ok=ok.astype(bool), iters=iters, chi2=chi2)

    def get_matches(self, frame0, n):
        cm = np.zeros((n, self.cap), np.int32)
        nm = np.zeros(n, np.int32)
        _check(self.L.sd_track_get_matches(self.h, frame0, n, _p(cm), self.cap, _p(nm)))
        return cm, nm

    def get_pnp(self, frame0, n):
        T = np.zeros((n, 16), np.float32)
        inl = np.zeros((n, self.cap), np.uint8)
        info = np.zeros((n, 8), np.int32)
        _check(self.L.sd_track_get_pnp(self.h, frame0, n, _p(T), _p(inl), self.cap, _p(info)))
        return dict(T=T.reshape(n, 4, 4), inliers=inl.astype(bool), ok=info[:, 0].astype(bool), n_inliers=info[:, 1],
                    no_more=info[:, 2].astype(bool), iterations=info[:, 3], N=info[:, 4], min_inliers=info[:, 5],
                    max_its=info[:, 6], refined=info[:, 7].astype(bool))

    def set_point_flags(self, frame0, has_mp_cur, has_mp_ref):
        self._set_rows(self.L.sd_track_set_point_flags, frame0, np.uint8, has_mp_cur, has_mp_ref)

    def search_by_points(self, n_frames, nnratio=0.75, check_ori=True):
        """ORBmatcher::SearchByPoints(currentKF, pKF, matches): brute-force Hamming between two keyframes' map points."""
        _check(self.L.sd_track_search_by_points(self.h, n_frames, float(nnratio), int(check_ori)))

    def get_point_matches(self, frame0, n):
        m = np.zeros((n, self.cap), np.int32)
        nm = np.zeros(n, np.int32)
        _check(self.L.sd_track_get_point_matches(self.h, frame0, n, _p(m), self.cap, _p(nm)))
        return m, nm

    # --- ORBmatcher::SearchForTriangulation + LocalMapping::ComputeF12 on the SearchByPoints pairing (track_tri.hip) ---
    def set_uright_ref(self, frame0, uright):
        """mvuRight of the ref extractor's frames, [n, cap'] (-1: mono)."""
        self._set_rows(self.L.sd_track_set_uright_ref, frame0, np.float32, uright)

    def set_f12(self, frame0, F12):
        """The caller's own F12 per slot, [n, 3, 3], for search_for_triangulation(use_set_f12=True)."""
        F = np.ascontiguousarray(F12, np.float64).reshape(-1, 9)
        _check(self.L.sd_track_set_f12(self.h, frame0, F.shape[0], _p(F)))

    def search_for_triangulation(self, n_frames, use_set_f12=False, check_ori=False):
        """SearchForTriangulation(KF1 = cur slot, KF2 = ref slot, F12) with the flags of set_point_flags read as "holds a map
        point"; F12 = ComputeF12 of the slot's poses unless use_set_f12."""
        _check(self.L.sd_track_search_for_triangulation(self.h, n_frames, int(use_set_f12), int(check_ori)))

    def get_triangulation_matches(self, frame0, n):
        m = np.zeros((n, self.cap), np.int32)
        nm = np.zeros(n, np.int32)
        F, e = np.zeros((n, 9)), np.zeros((n, 2), np.float32)
        _check(self.L.sd_track_get_triangulation_matches(self.h, frame0, n, _p(m), self.cap, _p(nm), _p(F), _p(e)))
        return dict(matches12=m, n_matches=nm, F12=F.reshape(n, 3, 3), epipole=e)

    # --- LocalMapping::CreateNewMapPoints after the search (track_newpoints_tri.hip) ---
    def set_tri_depth(self, side, frame0, depth):
        """mvDepth rows [n, cap'] of the cur (side 0, indexed by cur frame) or ref (side 1) extractor's frames."""
        d = np.ascontiguousarray(depth, np.float32)
        assert d.ndim == 2
        _check(self.L.sd_track_set_tri_depth(self.h, int(side), frame0, d.shape[0], _p(d), d.shape[1]))

    def set_tri_median_depth(self, frame0, median_depth):
        """ComputeSceneMedianDepth(2) of every slot's KF2 (monocular baseline gate); negative: no gate."""
        a = np.ascontiguousarray(median_depth, np.float32)
        _check(self.L.sd_track_set_tri_median_depth(self.h, frame0, len(a), _p(a)))

    def triangulate(self, n_frames, monocular=True):
        """Triangulate and test every match of the live search_for_triangulation result, then number the new points."""
        _check(self.L.sd_track_triangulate(self.h, n_frames, int(monocular)))

    def get_triangulated(self, frame0, n):
        v, b = np.zeros((n, self.cap), np.uint8), np.zeros((n, self.cap), np.uint8)
        X, na = np.zeros((n, self.cap, 3)), np.zeros(n, np.int32)
        _check(self.L.sd_track_get_triangulated(self.h, frame0, n, _p(v), _p(b), _p(X), self.cap, _p(na)))
        return dict(verdict=v, branch=b, Xw=X, n_accepted=na)

    def get_new_points(self):
        """The points of the last triangulate() in (slot, idx1) order."""
        info = np.zeros(4, np.int32)
        _check(self.L.sd_track_get_new_points(self.h, _p(info), *[None] * 9, 0))
        n = int(info[0])
        i32 = [np.zeros(n, np.int32) for _ in range(4)]
        X, N = np.zeros((n, 3)), np.zeros((n, 3))
        mx, mn, d = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 32), np.uint8)
        if n:
            _check(self.L.sd_track_get_new_points(self.h, _p(info), *[_p(a) for a in i32], _p(X), _p(N), _p(mx), _p(mn), _p(d), n))
        return dict(info=info, kp1=i32[0], slot=i32[1], idx2=i32[2], id=i32[3], Xw=X, normal=N, max_dist=mx, min_dist=mn, desc=d)

    # --- the new points as local-map rows, on the device (track_append.hip) ---
    def append_new_points(self, point_row=0, n_cand_rows=0, mark_flags=False):
        """The points of the live triangulate() result behind the points of local row point_row (cand of rows < n_cand_rows:
        f != the point's slot), or with point_row = -1 behind those of each point's own slot's row.  Queued, no host wait."""
        _check(self.L.sd_track_append_new_points(self.h, int(point_row), int(n_cand_rows), int(mark_flags)))

    def get_appended(self, frame0, n):
        """dict(base, appended, dropped) per local row of the last append_new_points()."""
        out = [np.zeros(n, np.int32) for _ in range(3)]
        _check(self.L.sd_track_get_appended(self.h, frame0, n, *[_p(a) for a in out]))
        return dict(base=out[0], appended=out[1], dropped=out[2])

    def get_local_points(self, row):
        """Local row `row` as it is on the device: dict(n, cand, Xw, normal, min_dist, max_dist, mf_max_dist, desc, obs), M entries."""
        M = self.M
        n = np.zeros(1, np.int32)
        out = dict(cand=np.zeros(M, np.uint8), Xw=np.zeros((M, 3)), normal=np.zeros((M, 3)), min_dist=np.zeros(M, np.float32),
                   max_dist=np.zeros(M, np.float32), mf_max_dist=np.zeros(M, np.float32), desc=np.zeros((M, 32), np.uint8),
                   obs=np.zeros(M, np.int32))
        _check(self.L.sd_track_get_local_points(self.h, int(row), _p(n), *[_p(a) for a in out.values()], M))
        return dict(n=int(n[0]), **out)

    # --- ORBmatcher::Fuse, both overloads (src/ORBmatcher.cc:477-732); the points are set_local's rows ---
    def set_fuse_scw(self, frame0, Scw):
        """The Sim3 Scw per slot, [n, 4, 4], for fuse(sim3=True)."""
        S = np.ascontiguousarray(np.asarray(Scw, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
        _check(self.L.sd_track_set_fuse_scw(self.h, frame0, S.shape[0], _p(S)))

    def fuse(self, n_frames, kf_side=0, point_row=-1, th=3.0, sim3=False):
        """The Fuse search of every slot: kf_side 0 = the cur frame (or the broadcast frame) at Tcur, 1 = the ref frame at Tref;
        point_row r >= 0: every slot reads the points of row r and the cand flags of its own row."""
        _check(self.L.sd_track_fuse(self.h, n_frames, int(kf_side), int(point_row), float(th), int(sim3)))

    def get_fuse(self, frame0, n):
        bi, bd = np.zeros((n, self.M), np.int32), np.zeros((n, self.M), np.int32)
        nf = np.zeros(n, np.int32)
        _check(self.L.sd_track_get_fuse(self.h, frame0, n, _p(bi), _p(bd), self.M, _p(nf)))
        return dict(best_idx=bi, best_dist=bd, n_found=nf)

    def fuse_pose(self, frame):
        """What the last fuse() projected slot `frame` with: (Rcw [3, 3], tcw [3], Ow [3])."""
        p = np.zeros(15)
        _check(self.L.sd_track_debug_read(self.h, 2, frame, _p(p), p.nbytes))
        return p[:9].reshape(3, 3), p[9:12], p[12:]

    # --- MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (src/MapPoint.cc:225-343); points = a set_local row ---
    def set_observations(self, obs, ref_obs, point_bad=None):
        """obs: per point a list of (frame, kp) or (frame, kp, kf_bad) in the caller's iteration order; frame >= 0 a ref frame,
        -1 the current keyframe, -2 not resident.  ref_obs[i]: position of mpRefKF in point i's list."""
        off, fr, kp, kb = _refresh_csr(obs)
        ro = np.ascontiguousarray(ref_obs, np.int32)
        pb = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
        assert len(ro) == len(obs) and (pb is None or len(pb) == len(obs))
        _check(self.L.sd_track_set_observations(self.h, len(obs), _p(off), _p(fr), _p(kp), _p(kb), _p(ro), _p(pb)))
        self._n_refresh, self._n_refresh_obs = len(obs), len(fr)

    def refresh_points(self, point_row=0, write_local=True):
        """Both functions for the points of set_observations at Xw of local row `point_row`; write_local: into that row too."""
        _check(self.L.sd_track_refresh_points(self.h, int(point_row), int(write_local)))

    def get_refreshed(self, fill=None):
        """dict(status, best_obs, best_median, desc, normal, max_dist, min_dist) of the last refresh_points()."""
        out = _refresh_outputs(self._n_refresh, fill)
        _check(self.L.sd_track_get_refreshed(self.h, *[_p(out[k]) for k in _REFRESH_FIELDS], self._n_refresh))
        return out

    def read_local_row(self, frame):
        """The refreshable fields of local row `frame` as they are on the device: dict(desc, normal, min_dist, max_dist, mf_max_dist)."""
        M = self.M
        out = dict(desc=np.zeros((M, 32), np.uint8), normal=np.zeros((M, 3)), min_dist=np.zeros(M, np.float32),
                   max_dist=np.zeros(M, np.float32), mf_max_dist=np.zeros(M, np.float32))
        for which, key in enumerate(("desc", "normal", "min_dist", "max_dist", "mf_max_dist"), start=3):
            _check(self.L.sd_track_debug_read(self.h, which, frame, _p(out[key]), out[key].nbytes))
        return out

    # --- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:417-714) on the lists of set_observations ---
    def set_ba_keyframes(self, kf_role, cur_role=1):
        """kf_role[f] of the ref frames (1 local, 2 local and fixed, 0 otherwise) and the current keyframe's role (1 or 2)."""
        r = np.ascontiguousarray(kf_role, np.uint8)
        _check(self.L.sd_track_set_ba_keyframes(self.h, len(r), _p(r), int(cur_role)))
        self._n_ba_ref = len(r)

    def local_ba(self, point_row=0, write_back=True):
        """Both rounds on the points of set_observations at row `point_row`; write_back: poses and positions into Tref / Tcur / Xw."""
        _check(self.L.sd_track_local_ba(self.h, int(point_row), int(write_back)))
        self._n_ba = (self._n_refresh, self._n_refresh_obs)

    def global_ba(self, point_row=0, n_iterations=10, robust=False, write_back=False):
        """Optimizer::BundleAdjustment (src/Optimizer.cc:46-219): one optimize(n_iterations) on the points of set_observations at
        row `point_row`, every keyframe with role 1 free.  write_back: the nLoopKF == 0 branch."""
        _check(self.L.sd_track_global_ba(self.h, int(point_row), int(n_iterations), int(robust), int(write_back)))
        self._n_gba = self._n_refresh

    def _get_ba(self, getter, n, n_obs=None):
        """What both bundle adjustments' getters return; n_obs: the getter has obs_erase [n_obs] as well."""
        Tr, Tc = np.zeros((self._n_ba_ref, 16)), np.zeros(16)
        out = dict(Xw=np.zeros((n, 3)), point_status=np.zeros(n, np.uint8))
        if n_obs is not None:
            out["obs_erase"] = np.zeros(n_obs, np.uint8)
        out["info16"] = np.zeros(16, np.int32)
        _check(getter(self.h, _p(Tr), _p(Tc), *[_p(a) for a in out.values()], n, *([] if n_obs is None else [n_obs])))
        out.update(T_ref=np.stack([_from_cm(t) for t in Tr]) if len(Tr) else np.zeros((0, 4, 4)), T_cur=_from_cm(Tc))
        return out

    def get_global_ba(self):
        """dict(T_ref [n_ref, 4, 4], T_cur [4, 4], Xw, point_status, info16) of the last global_ba()."""
        return self._get_ba(self.L.sd_track_get_global_ba, getattr(self, "_n_gba", 0))

    def get_local_ba(self):
        """dict(T_ref [n_ref, 4, 4], T_cur [4, 4], Xw, point_status, obs_erase, info16) of the last local_ba()."""
        return self._get_ba(self.L.sd_track_get_local_ba, *self._n_ba)

    # --- LocalMapping::KeyFrameCulling (src/LocalMapping.cc:580-634) and the erasure of observations, on the same lists ---
    def cull_keyframes(self, cand_frame, cand_flags, monocular, th_depth):
        """The candidates (ref frames, in GetVectorCovisibleKeyFrames() order; flags bit 0 mnId == 0, bit 1 mbNotErase) against
        the lists of set_observations; the lists themselves stay."""
        cf, fl = np.ascontiguousarray(cand_frame, np.int32), np.ascontiguousarray(cand_flags, np.uint8)
        assert len(cf) == len(fl)
        _check(self.L.sd_track_cull_keyframes(self.h, len(cf), _p(cf), _p(fl), int(monocular), float(th_depth)))
        self._n_cull = (len(cf), self._n_refresh, self._n_refresh_obs)

    def get_culled(self):
        """dict(verdict, counts2, obs_dead, point_bad, ref_obs, n_obs, info8) of the last cull_keyframes()."""
        out = _cull_outputs(*self._n_cull)
        _check(self.L.sd_track_get_culled(self.h, *[_p(a) for a in out.values()], *self._n_cull))
        return out

    def erase_observations(self, source):
        """Kill the obs_erase of the last local_ba() (ERASE_LOCAL_BA) or the dead entries of the last cull (ERASE_CULL) with the
        reference's cascade and compact the resident lists.  The entry count the handle was packed for stays an upper bound."""
        _check(self.L.sd_track_erase_observations(self.h, int(source)))
        self._n_erased = (self._n_refresh, self._n_refresh_obs)

    def get_erased(self):
        """dict(obs_off, obs_map, point_bad, ref_obs, n_obs, info8) of the last erase_observations()."""
        out = _erase_outputs(*self._n_erased)
        _check(self.L.sd_track_get_erased(self.h, *[_p(a) for a in out.values()], *self._n_erased))
        return out

    def read_poses(self, n):
        """Tref and Tcur of slots 0 .. n - 1 as they are on the device: ([n, 4, 4], [n, 4, 4])."""
        out = np.zeros((2, n, 16))
        for side in range(2):
            for f in range(n):
                _check(self.L.sd_track_debug_read(self.h, 8 + side, f, _p(out[side, f]), 128))
        return np.stack([_from_cm(t) for t in out[0]]), np.stack([_from_cm(t) for t in out[1]])

    # --- Sim3Solver on the SearchByPoints pairing (src/Sim3Solver.cc; caller LoopClosing::ComputeSim3) ---
    def set_sim3_points(self, frame0, Xw_cur, Xw_ref):
        """GetWorldPos() of the two keyframes' map points, [n, cap', 3] each, by that keyframe's keypoint index."""
        a, b = np.ascontiguousarray(Xw_cur, np.float64), np.ascontiguousarray(Xw_ref, np.float64)
        assert a.ndim == 3 and a.shape == b.shape and a.shape[2] == 3
        _check(self.L.sd_track_set_sim3_points(self.h, frame0, a.shape[0], _p(a), _p(b), a.shape[1]))

    def set_point_matches(self, frame0, matches12):
        """vpMatched12 of the slots from the caller: [n, cap'] indices of pKF keypoints, -1 = NULL."""
        self._set_rows(self.L.sd_track_set_point_matches, frame0, np.int32, matches12)

    def sim3(self, n_frames, fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, n_iterations=None):
        """Sim3Solver ctor + SetRansacParameters + iterate(n_iterations) (None: find())."""
        n_iterations = max_iterations if n_iterations is None else n_iterations
        _check(self.L.sd_track_sim3(self.h, n_frames, int(fix_scale), probability, min_inliers, max_iterations, n_iterations))

    def sim3_iterate(self, n_frames, n_iterations):
        """A further Sim3Solver::iterate(n_iterations) on the solvers the last sim3() call constructed."""
        _check(self.L.sd_track_sim3_iterate(self.h, n_frames, int(n_iterations)))

    def get_sim3(self, frame0, n):
        T, R, t, s = np.zeros((n, 16)), np.zeros((n, 9)), np.zeros((n, 3)), np.zeros(n)
        inl = np.zeros((n, self.cap), np.uint8)
        info = np.zeros((n, 8), np.int32)
        _check(self.L.sd_track_get_sim3(self.h, frame0, n, _p(T), _p(R), _p(t), _p(s), _p(inl), self.cap, _p(info)))
        return dict(T12=np.stack([_from_cm(x) for x in T]), R=R.reshape(n, 3, 3).transpose(0, 2, 1), t=t, scale=s,
                    inliers=inl.astype(bool), info=info, returned=info[:, 0].astype(bool), n_inliers=info[:, 1],
                    no_more=info[:, 2].astype(bool), iterations=info[:, 3], N=info[:, 4], max_its=info[:, 5], best_inliers=info[:, 6])

    def features_in_area(self, frame, x, y, r, min_level=-1, max_level=-1, want_grid=False):
        """Frame::GetFeaturesInArea on the device grid of current frame `frame` (debug read-out)."""
        idx = np.zeros(self.cap, np.int32)
        n = C.c_int32(0)
        grid = np.zeros((64, 48), np.int32) if want_grid else None
        _check(self.L.sd_track_debug_features_in_area(self.h, frame, x, y, r, min_level, max_level, _p(idx), self.cap, C.byref(n),
                                                      _p(grid) if want_grid else None))
        return (idx[:n.value].copy(), grid) if want_grid else idx[:n.value].copy()

    def pack_records(self, n_frames, source, d_ptr):
        """Queue the packing of the batch's result records (n_frames x 20 f64) into device memory at `d_ptr`."""
        _check(self.L.sd_track_pack_records(self.h, n_frames, int(source), C.c_void_p(d_ptr)))

    def stream_fence(self, stream_ptr, direction):
        """direction 0: the caller's stream waits for the tracking stream; 1: the tracking stream waits for the caller's."""
        _check(self.L.sd_track_stream_fence(self.h, C.c_void_p(stream_ptr) if stream_ptr else None, int(direction)))

    # --- sequential tracking: the last-frame hand-off on the device (src/Tracking.cc:250-292) ---
    def set_map_ids(self, frame0, ids_list, which=0):
        """The caller's identity of each map point, one array per slot (-1 = none); which 0: last-frame points, 1: local map."""
        n, M = len(ids_list), self.M
        assert all(len(v) <= M for v in ids_list)
        ids, _ = _padded(ids_list, (n, M), np.int32, fill=-1)
        _check(self.L.sd_track_set_map_ids(self.h, frame0, n, int(which), _p(ids), M))

    def advance(self, n_frames, source=1):
        """mLastFrame = Frame(mCurrentFrame) for every slot on the device; source 0: after track_with_motion_model, 1: after
        track_local_map, 2: after stereo_init.  The extractors swap roles: extract the next frame into `self.cur`."""
        _check(self.L.sd_track_advance(self.h, n_frames, int(source)))
        self._follow_extractors()

    def _follow_extractors(self):
        cur, ref = C.c_void_p(), C.c_void_p()
        _check(self.L.sd_track_get_extractors(self.h, C.byref(cur), C.byref(ref)))
        if cur.value != self.cur.h.value:
            self.cur, self.ref = self.ref, self.cur
        assert cur.value == self.cur.h.value and ref.value == self.ref.h.value

    def set_prior(self, frame0, T_list, relative=False):
        """Tprior = Tcur = T (relative False) or T @ Tref computed on the device (ConstantVelocity::GetPose); Tref stays."""
        a = np.ascontiguousarray(np.stack([_cm(T) for T in T_list]))
        _check(self.L.sd_track_set_prior(self.h, frame0, len(T_list), _p(a), int(bool(relative))))

    # --- motion model on the device: EKF + ConstantVelocity per slot (src/sensors/EKF.cc, ConstantVelocity.cc) ---
    def motion_predict(self, n_frames, dt):
        """Queue EKF::Predict for slots < n_frames: Tprior = Tcur = Exp(X) @ Tref; dt is the time since the last update."""
        _check(self.L.sd_track_motion_predict(self.h, n_frames, float(dt)))

    def motion_update(self, n_frames, source=1):
        """Queue EKF::Update with the frames' final poses for the slots the call named by `source` tracked (0
        track_with_motion_model, 1 track_local_map, -1 every slot), EKF::Restart for the others.  Before advance()."""
        _check(self.L.sd_track_motion_update(self.h, n_frames, int(source)))

    def motion_restart(self, frame0, n_frames):
        _check(self.L.sd_track_motion_restart(self.h, frame0, n_frames))

    def get_motion(self, frame0, n):
        """dict(X [n][6], P [n][6] diagonal, started [n], it_time [n], E and last_pose as n 4x4 matrices); synchronises."""
        X, P, st, it = np.zeros((n, 6)), np.zeros((n, 6)), np.zeros(n, np.int32), np.zeros(n)
        E, Lp = np.zeros((n, 16)), np.zeros((n, 16))
        _check(self.L.sd_track_get_motion(self.h, frame0, n, _p(X), _p(P), _p(st), _p(it), _p(E), _p(Lp)))
        return dict(X=X, P=P, started=st, it_time=it, E=[_from_cm(e) for e in E], last_pose=[_from_cm(t) for t in Lp])

    def set_motion(self, frame0, X=None, P=None, started=None, it_time=None):
        """Restore a stream's filter: [n][6] X, [n][6] diagonal of P, [n] started, [n] it_time; None leaves a field alone."""
        a = [None if v is None else np.ascontiguousarray(v, dt) for v, dt in ((X, np.float64), (P, np.float64), (started, np.int32),
                                                                              (it_time, np.float64))]
        n = {len(v) for v in a if v is not None}
        assert len(n) == 1
        _check(self.L.sd_track_set_motion(self.h, frame0, n.pop(), *[None if v is None else _p(v) for v in a]))

    # --- IMU sensor model: the 16-state EKF of Monocular-IMU tracking (src/sensors/IMU.cc), chosen per tracker ---
    SENSOR_CONSTANT_VELOCITY, SENSOR_IMU = 0, 1

    def set_sensor_model(self, model):
        """The filter motion_predict / motion_update / motion_restart run; every slot's filter of that model restarts."""
        _check(self.L.sd_track_set_sensor_model(self.h, int(model)))

    def get_sensor_model(self):
        m = C.c_int(-1)
        _check(self.L.sd_track_get_sensor_model(self.h, C.byref(m)))
        return m.value

    def set_measurements(self, frame0, wa):
        """Tracking::SetMeasurements for slots frame0 ..: [n][6] (gyro xyz, accelerometer xyz); queued, persists until replaced."""
        a = np.ascontiguousarray(wa, np.float64).reshape(-1, 6)
        _check(self.L.sd_track_set_measurements(self.h, frame0, len(a), _p(a)))

    def get_imu(self, frame0, n):
        """dict(X [n][16], P [n][16][16], gravity [n][3], started [n], it_time [n], last_pose as n 4x4 matrices, measurements
        [n][6]); synchronises."""
        X, P, g, st, it = np.zeros((n, 16)), np.zeros((n, 16, 16)), np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n)
        Lp, me = np.zeros((n, 16)), np.zeros((n, 6))
        _check(self.L.sd_track_get_imu(self.h, frame0, n, _p(X), _p(P), _p(g), _p(st), _p(it), _p(Lp), _p(me)))
        return dict(X=X, P=P, gravity=g, started=st, it_time=it, last_pose=[_from_cm(t) for t in Lp], measurements=me)

    def set_imu(self, frame0, X=None, P=None, gravity=None, started=None, it_time=None):
        """Restore a stream's IMU filter: [n][16] X, [n][16][16] P, [n][3] gravity, [n] started, [n] it_time; None leaves a field."""
        a = [None if v is None else np.ascontiguousarray(v, dt) for v, dt in ((X, np.float64), (P, np.float64), (gravity, np.float64),
                                                                              (started, np.int32), (it_time, np.float64))]
        n = {len(v) for v in a if v is not None}
        assert len(n) == 1
        _check(self.L.sd_track_set_imu(self.h, frame0, n.pop(), *[None if v is None else _p(v) for v in a]))

    def get_last(self, frame0, n):
        """The last-frame arrays, [n][max_points] layout."""
        M = self.M
        out = dict(n_last=np.zeros(n, np.int32), valid=np.zeros((n, M), np.uint8), Xw=np.zeros((n, M, 3)), desc=np.zeros((n, M, 32), np.uint8),
                   octave=np.zeros((n, M), np.int32), angle=np.zeros((n, M), np.float32), obs=np.zeros((n, M), np.int32),
                   ids=np.zeros((n, M), np.int32))
        _check(self.L.sd_track_get_last(self.h, frame0, n, *[_p(out[k]) for k in ("n_last", "valid", "Xw", "desc", "octave", "angle", "obs",
                                                                                 "ids")]))
        return out

    def close_points(self, n_frames, source, th_depth):
        """Queue Tracking::NeedNewKeyFrame's RGB-D counts (src/Tracking.cc:776-789) for slots < n_frames: keypoints with
        0 < mvDepth < th_depth (mThDepth = mbf * ThDepth / fx) whose map point advance(source) would keep, and the others."""
        _check(self.L.sd_track_close_points(self.h, n_frames, int(source), float(th_depth)))

    def get_close_points(self, frame0, n):
        """dict(tracked=nTrackedClose, non_tracked=nNonTrackedClose), one entry per slot."""
        out = np.zeros((n, 2), np.int32)
        _check(self.L.sd_track_get_close_points(self.h, frame0, n, _p(out)))
        return dict(tracked=out[:, 0].copy(), non_tracked=out[:, 1].copy())

    # --- RGB-D map point creation and the keyframe decision on the device (src/Tracking.cc:302-349, :753-896) ---
    KF_KEEP = -2 ** 31      # SD_KF_KEEP: a state entry that leaves the device's value

    def set_next_map_id(self, frame0, next_ids):
        """MapPoint::nNextId of every slot's map: the id the next created point receives."""
        a = np.ascontiguousarray(next_ids, np.int32)
        _check(self.L.sd_track_set_next_map_id(self.h, frame0, len(a), _p(a)))

    def stereo_init(self, n_frames, min_keypoints=500):
        """Queue Tracking::StereoInitialization for slots < n_frames: identity pose, one map point per keypoint with depth."""
        _check(self.L.sd_track_stereo_init(self.h, n_frames, int(min_keypoints)))

    def set_keyframe_state(self, frame0, state8):
        """NeedNewKeyFrame's caller state, [n][8] int32: nKFs, nRefMatches, last_kf_id, last_reloc_id, flags, 3 reserved."""
        assert np.shape(state8)[1:] == (8,)
        self._set_rows(self.L.sd_track_set_keyframe_state, frame0, np.int32, state8, pitch=False)

    def need_keyframe(self, n_frames, rgbd, frame_id, min_frames, max_frames):
        """Queue Tracking::NeedNewKeyFrame for slots < n_frames; the result is the slots' keyframe flags."""
        _check(self.L.sd_track_need_keyframe(self.h, n_frames, int(bool(rgbd)), int(frame_id), int(min_frames), int(max_frames)))

    def set_keyframe_flags(self, frame0, flags):
        a = np.ascontiguousarray(flags, np.uint8)
        _check(self.L.sd_track_set_keyframe_flags(self.h, frame0, len(a), _p(a)))

    def get_keyframe_flags(self, frame0, n):
        out = np.zeros(n, np.uint8)
        _check(self.L.sd_track_get_keyframe_flags(self.h, frame0, n, _p(out)))
        return out

    def create_keyframe_points(self, n_frames, source, th_depth, use_flags=False, frame_id=0):
        """Queue the RGB-D part of Tracking::CreateNewKeyFrame for slots < n_frames (use_flags: only where flag bit 0 is set)."""
        _check(self.L.sd_track_create_keyframe_points(self.h, n_frames, int(source), float(th_depth), int(bool(use_flags)), int(frame_id)))

    def get_created(self, frame0, n, cap=None):
        """The points the last creation call made, per slot in creation order: dict(mode, created, P, candidates, kp_index, Xw, ids)
        with [n][cap] rows (cap defaults to the keypoint capacity), entries >= created are -1 / 0."""
        cap = self.cap if cap is None else cap
        info = np.zeros((n, 4), np.int32)
        idx, ids, Xw = np.full((n, cap), -1, np.int32), np.full((n, cap), -1, np.int32), np.zeros((n, cap, 3))
        _check(self.L.sd_track_get_created(self.h, frame0, n, _p(info), _p(idx), _p(Xw), _p(ids), cap))
        return dict(mode=info[:, 0].copy(), created=info[:, 1].copy(), P=info[:, 2].copy(), candidates=info[:, 3].copy(), kp_index=idx,
                    Xw=Xw, ids=ids)

    def set_profiling(self, on=True):
        _check(self.L.sd_track_set_profiling(self.h, int(on)))

    def stage_ms(self):
        ms = np.zeros(3, np.float32)
        _check(self.L.sd_track_stage_ms(self.h, _p(ms), 3))
        return ms


def debug_epnp(Xw, uv, K):
    """Device EPnP on explicit correspondences (diagnostics)."""
    L = lib()
    Xw = np.ascontiguousarray(Xw, np.float64)
    uv = np.ascontiguousarray(uv, np.float64)
    R, t, e = np.zeros(9), np.zeros(3), C.c_double()
    _check(L.sd_debug_epnp(len(Xw), _p(Xw), _p(uv), float(K[0]), float(K[1]), float(K[2]), float(K[3]), _p(R), _p(t),
                           C.byref(e)))
    return R.reshape(3, 3), t, e.value


def debug_search_for_triangulation(kps1, desc1, has_mp1, uright1, kps2, desc2, has_mp2, uright2, F12, epipole, scale_factors,
                                   level_sigma2, check_ori=False):
    """One keyframe pair from host arrays through k_search_triangulation (diagnostics): (nmatches, matches12[n1])."""
    L = lib()
    k1, k2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
    n1, n2 = len(k1), len(k2)
    d1, d2 = np.ascontiguousarray(desc1, np.uint8).reshape(n1, 32), np.ascontiguousarray(desc2, np.uint8).reshape(n2, 32)
    h1, h2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
    u1, u2 = np.ascontiguousarray(uright1, np.float32), np.ascontiguousarray(uright2, np.float32)
    assert len(h1) == len(u1) == n1 and len(h2) == len(u2) == n2
    F, e = np.ascontiguousarray(F12, np.float64).reshape(9), np.ascontiguousarray(epipole, np.float32).reshape(2)
    sf, s2 = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
    assert len(sf) == len(s2)
    m, n = np.full(max(n1, 1), -1, np.int32), np.zeros(1, np.int32)
    _check(L.sd_debug_search_for_triangulation(n1, n2, _p(k1), _p(d1), _p(h1), _p(u1), _p(k2), _p(d2), _p(h2), _p(u2), _p(F), _p(e),
                                               _p(sf), _p(s2), len(sf), int(check_ori), _p(m), _p(n)))
    return int(n[0]), m[:n1]


def debug_triangulate(kps1_un, kps1, uright1, depth1, kps2_un, kps2, uright2, depth2, matches12, Tcw1, Tcw2, cam5, scale_factors,
                      level_sigma2, scale_factor, monocular=True, median_depth=-1.0):
    """One keyframe pair and a matches12 row from host arrays through k_triangulate (diagnostics): (verdict, branch, Xw)."""
    L = lib()
    k1u, k1 = np.ascontiguousarray(kps1_un, KP_DTYPE), np.ascontiguousarray(kps1, KP_DTYPE)
    k2u, k2 = np.ascontiguousarray(kps2_un, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
    n1, n2 = len(k1u), len(k2u)
    u1, z1 = np.ascontiguousarray(uright1, np.float32), np.ascontiguousarray(depth1, np.float32)
    u2, z2 = np.ascontiguousarray(uright2, np.float32), np.ascontiguousarray(depth2, np.float32)
    m = np.ascontiguousarray(matches12, np.int32)
    assert len(k1) == len(u1) == len(z1) == len(m) == n1 and len(k2) == len(u2) == len(z2) == n2
    T1, T2 = _cm(Tcw1), _cm(Tcw2)
    cam = np.ascontiguousarray(cam5, np.float32)
    sf, s2 = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
    assert len(cam) == 5 and len(sf) == len(s2)
    v, b, X = np.zeros(max(n1, 1), np.uint8), np.zeros(max(n1, 1), np.uint8), np.zeros((max(n1, 1), 3))
    _check(L.sd_debug_triangulate(n1, n2, _p(k1u), _p(k1), _p(u1), _p(z1), _p(k2u), _p(k2), _p(u2), _p(z2), _p(m), _p(T1), _p(T2),
                                  _p(cam), _p(sf), _p(s2), len(sf), float(scale_factor), int(monocular), float(median_depth), _p(v),
                                  _p(b), _p(X)))
    return v[:n1], b[:n1], X[:n1]


def debug_fuse(kps, desc, uright, pts, T, cam9, scale_factors, inv_level_sigma2, scale_factor, th=3.0, sim3=False, kp_cap=None,
               max_points=None):
    """One keyframe and one point list from host arrays through k_fuse (diagnostics).  pts: dict(cand, Xw, normal, min_dist,
    max_dist, mf_max_dist, desc); T: Tcw or Scw [4, 4].  Returns dict(best_idx, best_dist [n_pts], n_found, pose = (Rcw, tcw, Ow))."""
    L = lib()
    k = np.ascontiguousarray(kps, KP_DTYPE)
    nk = len(k)
    d, u = np.ascontiguousarray(desc, np.uint8).reshape(nk, 32), np.ascontiguousarray(uright, np.float32)
    c = np.ascontiguousarray(pts["cand"], np.uint8)
    n = len(c)
    X, N = np.ascontiguousarray(pts["Xw"], np.float64).reshape(n, 3), np.ascontiguousarray(pts["normal"], np.float64).reshape(n, 3)
    mn, mx, mf = (np.ascontiguousarray(pts[key], np.float32) for key in ("min_dist", "max_dist", "mf_max_dist"))
    pd = np.ascontiguousarray(pts["desc"], np.uint8).reshape(n, 32)
    Tc = np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4).T)
    cam = np.ascontiguousarray(cam9, np.float32)
    sf, is2 = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(inv_level_sigma2, np.float32)
    K, M = int(kp_cap or max(nk, 1)), int(max_points or max(n, 1))
    bi, bd = np.zeros(M, np.int32), np.zeros(M, np.int32)
    nf, pose = np.zeros(1, np.int32), np.zeros(15)
    assert len(cam) == 9 and len(u) == nk and len(sf) == len(is2)
    _check(L.sd_debug_fuse(nk, _p(k), _p(d), _p(u), n, _p(c), _p(X), _p(N), _p(mn), _p(mx), _p(mf), _p(pd), _p(Tc), int(sim3), _p(cam),
                           _p(sf), _p(is2), len(sf), float(scale_factor), float(th), K, M, _p(bi), _p(bd), _p(nf), _p(pose)))
    return dict(best_idx=bi[:n], best_dist=bd[:n], n_found=int(nf[0]), pose=(pose[:9].reshape(3, 3), pose[9:12], pose[12:]),
                rest_idx=bi[n:], rest_dist=bd[n:])


REFRESH_MAX_OBS = 256
REFRESH_DESC, REFRESH_NORMAL, REFRESH_SKIPPED, REFRESH_NOT_RESIDENT, REFRESH_TOO_MANY, REFRESH_BAD_INDEX = 1, 2, 16, 32, 64, 128
_REFRESH_FIELDS = ("status", "best_obs", "best_median", "desc", "normal", "max_dist", "min_dist")


def _refresh_csr(obs):
    """Per-point observation lists of (frame, kp[, kf_bad]) -> (obs_off, obs_frame, obs_kp, obs_kf_bad)."""
    off = np.zeros(len(obs) + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    flat = [t for o in obs for t in o]
    fr = np.array([t[0] for t in flat], np.int32)
    kp = np.array([t[1] for t in flat], np.int32)
    kb = np.array([t[2] if len(t) > 2 else 0 for t in flat], np.uint8)
    return off, fr, kp, kb


def _refresh_outputs(n, fill=None):
    """The seven output arrays for n points; fill: a dict of arrays to start from (copied), else zeros."""
    shapes = dict(status=((n,), np.uint8), best_obs=((n,), np.int32), best_median=((n,), np.int32), desc=((n, 32), np.uint8),
                  normal=((n, 3), np.float64), max_dist=((n,), np.float32), min_dist=((n,), np.float32))
    return {k: (np.zeros(sh, dt) if fill is None else np.ascontiguousarray(fill[k], dt).reshape(sh).copy())
            for k, (sh, dt) in shapes.items()}


def debug_refresh_points(obs_off, obs_desc, obs_centre, obs_octave, ref_obs, Xw, scale_factors, obs_kf_bad=None, point_bad=None,
                         fill=None):
    """Observation lists from host arrays through k_refresh_points (diagnostics).  fill: what the outputs hold before the call
    (entries the kernel does not write come back unchanged).  Returns dict(status, best_obs, best_median, desc, normal,
    max_dist, min_dist)."""
    L = lib()
    off = np.ascontiguousarray(obs_off, np.int32)
    n, total = len(off) - 1, int(off[-1])
    d = np.ascontiguousarray(obs_desc, np.uint8).reshape(total, 32)
    c = np.ascontiguousarray(obs_centre, np.float64).reshape(total, 3)
    oc = np.ascontiguousarray(obs_octave, np.int32)
    ro, X = np.ascontiguousarray(ref_obs, np.int32), np.ascontiguousarray(Xw, np.float64).reshape(n, 3)
    kb = None if obs_kf_bad is None else np.ascontiguousarray(obs_kf_bad, np.uint8)
    pb = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
    sf = np.ascontiguousarray(scale_factors, np.float32)
    assert len(oc) == total and len(ro) == n and (kb is None or len(kb) == total) and (pb is None or len(pb) == n)
    out = _refresh_outputs(n, fill)
    _check(L.sd_debug_refresh_points(n, _p(off), _p(d), _p(c), _p(oc), _p(kb), _p(ro), _p(pb), _p(X), _p(sf), len(sf),
                                     *[_p(out[k]) for k in _REFRESH_FIELDS]))
    return out


ERASE_LOCAL_BA, ERASE_CULL = 0, 1
CULL_OK, CULL_NOT_RESIDENT, CULL_BAD_INDEX = 0, 1, 2
CULL_SKIPPED_ID0, CULL_KEPT, CULL_CULLED, CULL_TO_BE_ERASED = 0, 1, 2, 3


def _cull_outputs(n_cand, n, total):
    """The output arrays of both culling entries, in their order"""
    return dict(verdict=np.zeros(n_cand, np.uint8), counts2=np.zeros((n_cand, 2), np.int32), obs_dead=np.zeros(total, np.uint8),
                point_bad=np.zeros(n, np.uint8), ref_obs=np.zeros(n, np.int32), n_obs=np.zeros(n, np.int32),
                info8=np.zeros(8, np.int32))


def _erase_outputs(n, total):
    """The output arrays of both erasing entries, in their order"""
    return dict(obs_off=np.zeros(n + 1, np.int32), obs_map=np.zeros(total, np.int32), point_bad=np.zeros(n, np.uint8),
                ref_obs=np.zeros(n, np.int32), n_obs=np.zeros(n, np.int32), info8=np.zeros(8, np.int32))


def debug_cull_keyframes(q, cand_kf, cand_flags, monocular, th_depth):
    """A culling problem (the dict tests/cull_ref.py documents: off, kf, octave, stereo, depth, ref_obs, point_bad or None, n_kf)
    from host arrays through k_cull (diagnostics).  Returns dict(verdict, counts2, obs_dead, point_bad, ref_obs, n_obs, info8)."""
    off = np.ascontiguousarray(q["off"], np.int32)
    n, total = len(off) - 1, int(off[-1])
    kf, oc = np.ascontiguousarray(q["kf"], np.int32), np.ascontiguousarray(q["octave"], np.int32)
    st, dp = np.ascontiguousarray(q["stereo"], np.uint8), np.ascontiguousarray(q["depth"], np.float32)
    ro = np.ascontiguousarray(q["ref_obs"], np.int32)
    pb = None if q.get("point_bad") is None else np.ascontiguousarray(q["point_bad"], np.uint8)
    cf, fl = np.ascontiguousarray(cand_kf, np.int32), np.ascontiguousarray(cand_flags, np.uint8)
    assert len(kf) == len(oc) == len(st) == len(dp) == total and len(ro) == n and len(cf) == len(fl) and (pb is None or len(pb) == n)
    out = _cull_outputs(len(cf), n, total)
    _check(lib().sd_debug_cull_keyframes(n, _p(off), _p(kf), _p(oc), _p(st), _p(dp), _p(ro), _p(pb), int(q["n_kf"]), len(cf), _p(cf),
                                         _p(fl), int(monocular), float(th_depth), *[_p(a) for a in out.values()]))
    return out


def debug_erase_observations(off, stereo, erase, ref_obs, point_bad=None):
    """Observation lists and erase flags from host arrays through k_erase (diagnostics).  Returns dict(obs_off, obs_map,
    point_bad, ref_obs, n_obs, info8)."""
    off = np.ascontiguousarray(off, np.int32)
    n, total = len(off) - 1, int(off[-1])
    st, er, ro = np.ascontiguousarray(stereo, np.uint8), np.ascontiguousarray(erase, np.uint8), np.ascontiguousarray(ref_obs, np.int32)
    pb = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
    assert len(st) == len(er) == total and len(ro) == n and (pb is None or len(pb) == n)
    out = _erase_outputs(n, total)
    _check(lib().sd_debug_erase_observations(n, _p(off), _p(st), _p(er), _p(ro), _p(pb), *[_p(a) for a in out.values()]))
    return out


def _ba_marshal(q, cam9, erase):
    """A bundle-adjustment problem dict as (the arguments both debug entries begin with: n .. cam9, their output buffers in the
    entries' order: T, Xw, point_status, obs_erase if `erase`, info16)"""
    off = np.ascontiguousarray(q["off"], np.int32)
    n, total = len(off) - 1, int(off[-1])
    kf, uv = np.ascontiguousarray(q["kf"], np.int32), np.ascontiguousarray(q["uv"], np.float32).reshape(total, 2)
    ur, inv = np.ascontiguousarray(q["ur"], np.float32), np.ascontiguousarray(q["inv_sigma2"], np.float32)
    kb = None if q.get("kf_bad") is None else np.ascontiguousarray(q["kf_bad"], np.uint8)
    pb = None if q.get("point_bad") is None else np.ascontiguousarray(q["point_bad"], np.uint8)
    roles = np.ascontiguousarray(q["roles"], np.uint8)
    T = np.ascontiguousarray(np.stack([_cm(t) for t in np.asarray(q["poses"], np.float64)]))
    X = np.ascontiguousarray(q["Xw"], np.float64).reshape(n, 3)
    if cam9 is None:
        cam9 = list(q["cam"]) + [q["bf"], 0.0, 1.0, 0.0, 1.0]
    cam = np.ascontiguousarray(cam9, np.float32)
    assert len(kf) == len(ur) == len(inv) == total and len(T) == len(roles) and len(cam) == 9
    out = dict(T=np.zeros_like(T), Xw=np.zeros_like(X), point_status=np.zeros(n, np.uint8))
    if erase:
        out["obs_erase"] = np.zeros(total, np.uint8)
    out["info16"] = np.zeros(16, np.int32)
    return [n, off, kf, uv, ur, inv, kb, pb, len(roles), T, roles, X, cam], out


def _ba_call(entry, args, out):
    """The debug entry on the arguments (arrays as pointers) and the buffers, and the buffers as the result dict"""
    _check(entry(*[a if isinstance(a, int) else _p(a) for a in args + list(out.values())]))
    out["T"] = np.stack([_from_cm(t) for t in out["T"]])
    return out


def debug_local_ba(problem, cam9=None):
    """A LocalBundleAdjustment problem (the dict tests/ba_ref.py documents: off, kf, uv, ur, inv_sigma2, kf_bad, point_bad, poses
    [n_kf, 4, 4], roles, Xw, cam, bf) from host arrays through the kernels of sd_track_local_ba (diagnostics).  Returns dict(T
    [n_kf, 4, 4], Xw, point_status, obs_erase, info16)."""
    args, out = _ba_marshal(problem, cam9, True)
    return _ba_call(lib().sd_debug_local_ba, args, out)


def debug_global_ba(problem, n_iterations, robust, cam9=None):
    """A BundleAdjustment problem (the dict of debug_local_ba; roles 1 free, 2 fixed, 0 no vertex) through the kernels of
    sd_track_global_ba (diagnostics).  Returns dict(T [n_kf, 4, 4], Xw, point_status, info16)."""
    args, out = _ba_marshal(problem, cam9, False)
    return _ba_call(lib().sd_debug_global_ba, args + [int(n_iterations), int(robust)], out)


def debug_ldlt(A, b):
    """The blocked LDL^T of sd_track_global_ba alone on the symmetric matrix A [n, n] (its lower triangle is read): (ok, x)."""
    A, b = np.asarray(A, np.float64), np.ascontiguousarray(b, np.float64)
    n = len(b)
    packed = np.ascontiguousarray(A[np.tril_indices(n)])          # row order: (0, 0), (1, 0), (1, 1), ...
    x, ok = np.zeros(n), np.zeros(1, np.int32)
    _check(lib().sd_debug_ldlt(n, _p(packed), _p(b), _p(x), _p(ok)))
    return bool(ok[0]), x
