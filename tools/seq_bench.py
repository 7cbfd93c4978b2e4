#!/usr/bin/env python3
"""Sequential tracking: B camera streams x T frames, TrackWithMotionModel + TrackLocalMap every frame, in two modes.

  device   the hand-off on the device: sd_track_set_prior (relative) -> track -> sd_track_advance; no host round trip
  host     the hand-off a caller had to do before sd_track_advance: synchronise, download sd_track_get_local_map /
           sd_track_get_pose_opt / the last frame, rebuild the next last frame on the host (numpy gather), re-upload it with
           sd_track_set_last + sd_track_set_map_ids + sd_track_set_poses.  Two trackers with swapped extractor roles
           alternate, so the previous frame's pyramid is the reference without a second extraction.

RGB-D modes (device hand-off, bMono = false, TrackLocalMap at th 3, sd_track_close_points every frame):
  host_f32    per frame: sd_track_stereo_from_depth on CV_32F maps in (pageable) host memory -- the call allocates, copies
              the whole maps and synchronises
  device_u16  per frame: sd_track_stereo_from_depth_device on 16-bit maps resident in HBM, DepthMapFactor 5000 (TUM)
  mono        the monocular device loop above, as the baseline
  (the mode list "rgbd" = host_f32,device_u16,mono)

RGB-D keyframe modes (no static map: every stream starts from sd_track_stereo_init on frame 0 with an empty local map and lives
on the points it creates; u16 depth in HBM; keyframe state nKFs 5, nRefMatches 700, idle mapper, MinFrames 3, MaxFrames 30):
  kf_device   per frame: ... -> sd_track_close_points -> sd_track_need_keyframe -> sd_track_create_keyframe_points(use_flags)
              -> sd_track_advance; the 32-byte keyframe state of every slot is uploaded each step; no host wait in the loop
  kf_host     the host alternative: synchronise, download depth, matches, outlier flags, poses and the last frame, decide and
              create the points in numpy, re-upload through sd_track_set_last (two trackers alternate, as in `host`)
  (the mode list "rgbd_kf" = kf_device,kf_host,device_u16 -- the last one is the loop without creation, run in the same
  session; results in profiles/seq_bench_rgbd_kf.json)

Motion-model modes (monocular, the `device` loop with the prior from the filter instead of ground-truth velocities; dt 1/30):
  ekf_device  per frame: sd_track_motion_predict -> track -> sd_track_motion_update(1) -> sd_track_advance: the EKF +
              ConstantVelocity state lives on the device, no pose crosses the bus and the host decides nothing
  ekf_host    what a caller had to do before: synchronise, download the B final poses and statuses (sd_track_get_align /
              sd_track_get_local_map), run the filter for B streams on the host (vectorised numpy, the textbook SE(3) Exp / Log),
              upload B matrices through sd_track_set_prior
  (results in profiles/seq_bench_motion.json when one of them is in the mode list)

IMU sensor-model modes (the 16-state EKF of Monocular-IMU tracking; gyro readings from the ground-truth poses, a constant
accelerometer reading; dt 1/30):
  imu_device  the ekf_device loop under sd_track_set_sensor_model(SD_SENSOR_IMU) with one sd_track_set_measurements per step
              (48 bytes per slot through the pinned ring): no host wait in the loop
  imu_host    what a caller had to do before: synchronise, download the B final poses and statuses, run the dense filter for
              B streams on the host (batched numpy, numpy.linalg.inv for the 13 x 13 S), upload B priors through
              sd_track_set_prior(relative = 0)
  (results in profiles/seq_bench_imu.json when one of them is in the mode list)

python tools/seq_bench.py [T=8] [B list=1,1024] [modes=device,host]  -> one JSON line per (B, mode), all of them in
profiles/seq_bench.json (profiles/seq_bench_rgbd.json when RGB-D modes run).
Frames are resident in HBM (extraction from device memory); the timed region is frames 1..T-1 including extraction, ended
by a synchronisation.  NU distinct sequences are tiled over the B streams.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import sdslam_amd  # noqa: E402
from sdslam_amd import synth  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 8
BS = [int(b) for b in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 1024]
MODES = sys.argv[3].split(",") if len(sys.argv) > 3 else ["device", "host"]
if MODES == ["rgbd"]:
    MODES = ["host_f32", "device_u16", "mono"]
KF = MODES == ["rgbd_kf"] or any(m in ("kf_device", "kf_host") for m in MODES)
if MODES == ["rgbd_kf"]:
    MODES = ["kf_device", "kf_host", "device_u16"]
EKF = any(m in ("ekf_device", "ekf_host") for m in MODES)
IMU = any(m in ("imu_device", "imu_host") for m in MODES)
EKF_DT = 1.0 / 30.0
IMU_A = (0.05, -0.03, 0.02)
RGBD = any(m in ("host_f32", "device_u16", "kf_device", "kf_host") for m in MODES)
KF_STATE = (5, 700, 0, 0, 1, 0, 0, 0)
KF_MIN_FRAMES, KF_MAX_FRAMES = 3, 30
NU = 8
BF = 4.0             # baseline x fx of the synthetic RGB-D camera (tests/test_sequence_gpu.py)
TH_CLOSE = 2.0       # mThDepth handed to sd_track_close_points: about the median depth of the synthetic scenes
M = 1000
CFG = (1000, 1.2, 8, 20)
K = (synth.FX, synth.FY, synth.CX, synth.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
F = 640 * 480


def setup(B, seqs):
    views = np.stack([np.stack([seqs[b % NU]["views"][t] for b in range(B)]) for t in range(T)])   # [T][B][H][W]
    frames = sdslam_amd.DeviceBuffer(views.nbytes)
    frames.upload(views)
    ext = [sdslam_amd.ORBextractor(*CFG, 640, 480, B) for _ in range(2)]
    k, d, n = ext[1].extract_batch(views[0])
    maps = [synth.static_map(k[b, :n[b]], d[b, :n[b]], seqs[b % NU]["T"][0], seed=b % NU) for b in range(min(B, NU))]
    maps = [maps[b % NU] for b in range(B)]
    vel = [[seqs[b % NU]["T"][t] @ np.linalg.inv(seqs[b % NU]["T"][t - 1]) for b in range(B)] for t in range(1, T)]
    return frames, ext, maps, vel


def new_tracker(cur, ref, B, maps, seqs):
    trk = sdslam_amd.Tracker(cur, ref, max_points=M, max_batch=B, pnp_max_iterations=100)
    trk.set_camera(*K, 0.0, BOUNDS)
    trk.set_last(0, [m[1] for m in maps])
    trk.set_local(0, [m[0] for m in maps])
    trk.set_map_ids(0, [m[2] for m in maps], 0)
    trk.set_map_ids(0, [m[2] for m in maps], 1)
    T0 = [seqs[b % NU]["T"][0] for b in range(B)]
    trk.set_poses(0, T0, T0)
    return trk


def track(trk, frames, B, t, vel=None):
    trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
    if vel is not None:
        trk.set_prior(0, vel, relative=True)
    trk.track_with_motion_model(B, th=15.0)
    trk.track_local_map(B, th=1.0)


def run_device(B, seqs):
    frames, ext, maps, vel = setup(B, seqs)
    trk = new_tracker(ext[0], ext[1], B, maps, seqs)
    t0 = time.perf_counter()
    for t in range(1, T):
        track(trk, frames, B, t, vel[t - 1])
        trk.advance(B, 1)
    st = trk.get_local_map(0, B)["status"]        # synchronises
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    return dt, st


def run_ekf_device(B, seqs):
    frames, ext, maps, _ = setup(B, seqs)
    trk = new_tracker(ext[0], ext[1], B, maps, seqs)
    t0 = time.perf_counter()
    for t in range(1, T):
        trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
        trk.motion_predict(B, EKF_DT)
        trk.track_with_motion_model(B, th=15.0)
        trk.track_local_map(B, th=1.0)
        trk.motion_update(B, 1)
        trk.advance(B, 1)
    st = trk.get_local_map(0, B)["status"]        # synchronises
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    return dt, st


def _hat(w):
    O = np.zeros(w.shape[:-1] + (3, 3))
    O[..., 0, 1], O[..., 0, 2], O[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    O[..., 1, 2], O[..., 2, 0], O[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return O


def se3_exp(x):
    """[B][6] (v, w) -> [B][4][4], Rodrigues; series below 1e-6 rad."""
    w = x[:, 3:]
    th = np.linalg.norm(w, axis=1)[:, None, None]
    small = th < 1e-6
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th * th / 24, (1 - np.cos(ths)) / ths ** 2)
    c = np.where(small, 1.0 / 6 - th * th / 120, (ths - np.sin(ths)) / ths ** 3)
    O = _hat(w)
    O2 = O @ O
    E = np.tile(np.eye(4), (len(x), 1, 1))
    E[:, :3, :3] = np.eye(3) + a * O + b * O2
    E[:, :3, 3] = ((np.eye(3) + b * O + c * O2) @ x[:, :3, None])[..., 0]
    return E


def se3_log(T):
    """[B][4][4] -> [B][6] (v, w), rotations below pi."""
    Rm = T[:, :3, :3]
    cos = np.clip((np.trace(Rm, axis1=1, axis2=2) - 1) / 2, -1, 1)
    th = np.arccos(cos)
    small = th < 1e-6
    ths = np.where(small, 1.0, th)
    f = np.where(small, 0.5 + th * th / 12, ths / (2 * np.sin(ths)))
    w = f[:, None] * np.stack([Rm[:, 2, 1] - Rm[:, 1, 2], Rm[:, 0, 2] - Rm[:, 2, 0], Rm[:, 1, 0] - Rm[:, 0, 1]], 1)
    c = np.where(small, 1.0 / 12, (1 - ths / (2 * np.tan(ths / 2))) / ths ** 2)[:, None, None]
    O = _hat(w)
    v = ((np.eye(3) - 0.5 * O + c * (O @ O)) @ T[:, :3, 3:4])[..., 0]
    return np.concatenate([v, w], 1)


def run_ekf_host(B, seqs):
    frames, ext, maps, _ = setup(B, seqs)
    trk = new_tracker(ext[0], ext[1], B, maps, seqs)
    X = np.zeros((B, 6))
    P = np.tile(np.array([0.000625] * 6), (B, 1))
    sig2 = np.array([16.0] * 3 + [36.0] * 3)
    started = np.zeros(B, bool)
    T_last = np.stack([seqs[b % NU]["T"][0] for b in range(B)])
    t0 = time.perf_counter()
    for t in range(1, T):
        it = np.where(started, EKF_DT, 0.0)[:, None]
        Q = sig2 * it * it
        P = P + Q
        trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
        trk.set_prior(0, list(se3_exp(X)), relative=True)
        trk.track_with_motion_model(B, th=15.0)
        trk.track_local_map(B, th=1.0)
        # the host round trip of the motion model: poses and statuses down, the filter in numpy
        pose = np.stack(trk.get_align(0, B)["T"])
        ok = trk.get_local_map(0, B)["status"] == 2
        Z = se3_log(pose @ np.linalg.inv(T_last))
        S = P + Q
        Kg = P / S
        upd = (ok & started)[:, None]
        X = np.where(upd, X + Kg * (Z - X), np.where(ok[:, None], X * started[:, None], 0.0))
        P = np.where(upd, P - Kg * S * Kg, np.where(ok[:, None], P, 0.000625))
        started = ok
        trk.advance(B, 1)
        T_last = pose
    st = trk.get_local_map(0, B)["status"]
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    return dt, st


def _rot_quat(Rm):
    """[B][3][3] -> [B][4] (w, x, y, z), rotations with a positive trace (the sequences')."""
    t = np.sqrt(np.trace(Rm, axis1=1, axis2=2) + 1.0)
    q = np.stack([0.5 * t, (Rm[:, 2, 1] - Rm[:, 1, 2]) * 0.5 / t, (Rm[:, 0, 2] - Rm[:, 2, 0]) * 0.5 / t, (Rm[:, 1, 0] - Rm[:, 0, 1]) * 0.5 / t], 1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _quat_mul(a, b):
    return np.stack([a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2] - a[:, 3] * b[:, 3],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                     a[:, 0] * b[:, 2] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1] - a[:, 1] * b[:, 3],
                     a[:, 0] * b[:, 3] + a[:, 3] * b[:, 0] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]], 1)


def _quat_w(wt):
    ang = np.linalg.norm(wt, axis=1)
    safe = np.where(ang > 0, ang, 1.0)
    return np.concatenate([np.where(ang > 0, np.cos(ang / 2), 1.0)[:, None], (np.where(ang > 0, np.sin(ang / 2) / safe, 0.0))[:, None] * wt], 1)


def _quat_rot(q):
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def _dq_by_dw(q, w, t):
    """Sensor::dq_by_dw for [B] filters, both branches."""
    modw = np.linalg.norm(w, axis=1)
    zero = modw == 0
    m = np.where(zero, 1.0, modw)[:, None, None]
    sb, cb = np.sin(m * t / 2), np.cos(m * t / 2)
    mdw = np.zeros((len(w), 4, 3))
    mdw[:, 0, :] = (-t / 2 * sb[:, 0] * w / m[:, 0])
    mdw[:, 1:, :] = w[:, :, None] * w[:, None, :] / (m * m) * (t / 2 * cb - sb / m) + np.eye(3) * (sb / m)
    w_, x, y, z = q.T
    JR = np.stack([np.stack([w_, -x, -y, -z], 1), np.stack([x, w_, -z, y], 1), np.stack([y, z, w_, -x], 1), np.stack([z, -y, x, w_], 1)], 1)
    res = JR @ mdw
    res[zero] = np.vstack([np.zeros((1, 3)), np.eye(3) * t / 2])
    return res


def imu_measurements(B, seqs):
    """[T][B][6]: gyro w_t = 2 log(q_{t-1}^-1 q_t) / dt from the ground-truth poses, the constant accelerometer reading."""
    out = np.zeros((T, B, 6))
    out[:, :, 3:] = IMU_A
    for u in range(min(B, NU)):
        q = _rot_quat(np.stack([seqs[u]["T"][t][:3, :3] for t in range(T)]))
        d = _quat_mul(q[:-1] * np.array([1.0, -1.0, -1.0, -1.0]), q[1:])
        nv = np.linalg.norm(d[:, 1:], axis=1)
        w = np.where(nv[:, None] > 0, 2 * np.arctan2(nv, d[:, 0])[:, None] * d[:, 1:] / np.where(nv > 0, nv, 1.0)[:, None], 0.0) / EKF_DT
        out[1:, u::NU, :3] = w[:, None, :]
    return out


def run_imu_device(B, seqs):
    frames, ext, maps, _ = setup(B, seqs)
    trk = new_tracker(ext[0], ext[1], B, maps, seqs)
    trk.set_sensor_model(trk.SENSOR_IMU)
    meas = imu_measurements(B, seqs)
    t0 = time.perf_counter()
    for t in range(1, T):
        trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
        trk.set_measurements(0, meas[t])
        trk.motion_predict(B, EKF_DT)
        trk.track_with_motion_model(B, th=15.0)
        trk.track_local_map(B, th=1.0)
        trk.motion_update(B, 1)
        trk.advance(B, 1)
    st = trk.get_local_map(0, B)["status"]        # synchronises
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    return dt, st


IMU_SEL = np.array([0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15])
IMU_P0 = np.diag([0.0025] * 3 + [0.00001] * 4 + [0.000625] * 9)
IMU_R = np.array([0.05 ** 2] * 3 + [0.02 ** 2] * 4 + [2.60 ** 2] * 3 + [8.94 ** 2] * 3)
IMU_PN = np.array([16.0] * 3 + [36.0] * 3 + [8.94 ** 2] * 3)


def run_imu_host(B, seqs):
    frames, ext, maps, _ = setup(B, seqs)
    trk = new_tracker(ext[0], ext[1], B, maps, seqs)
    meas = imu_measurements(B, seqs)
    X = np.zeros((B, 16))
    X[:, 3] = 1.0
    P = np.tile(IMU_P0, (B, 1, 1))
    g = np.zeros((B, 3))
    started = np.zeros(B, bool)
    T_last = np.stack([seqs[b % NU]["T"][0] for b in range(B)])
    dt_, I3 = EKF_DT, np.eye(3)
    t0 = time.perf_counter()
    for t in range(1, T):
        # EKF::Predict for the started filters; the last pose for the others
        q, w = X[:, 3:7], X[:, 10:13]
        qwt, D = _quat_w(w * dt_), _dq_by_dw(q, w, dt_)
        jF = np.tile(np.eye(16), (B, 1, 1))
        jF[:, 0:3, 7:10] = I3 * dt_
        jF[:, 7:10, 13:16] = I3 * dt_
        a_, b_, c_, d_ = qwt.T
        jF[:, 3:7, 3:7] = np.stack([np.stack([a_, -b_, -c_, -d_], 1), np.stack([b_, a_, d_, -c_], 1), np.stack([c_, -d_, a_, b_], 1),
                                    np.stack([d_, c_, -b_, a_], 1)], 1)
        jF[:, 3:7, 10:13] = D
        G = np.zeros((B, 16, 9))
        G[:, 0:3, 0:3], G[:, 7:10, 0:3], G[:, 7:10, 6:9], G[:, 10:13, 3:6], G[:, 13:16, 6:9] = I3 * dt_, I3, I3 * dt_, I3, I3
        G[:, 3:7, 3:6] = D
        Xp = X.copy()
        Xp[:, 0:3] += X[:, 7:10] * dt_
        Xp[:, 3:7] = _quat_mul(q, qwt)
        Xp[:, 7:10] += X[:, 13:16] * dt_
        Pp = jF @ P @ jF.transpose(0, 2, 1) + (G * (IMU_PN * dt_ * dt_)) @ G.transpose(0, 2, 1)
        X = np.where(started[:, None], Xp, X)
        P = np.where(started[:, None, None], Pp, P)
        prior = np.tile(np.eye(4), (B, 1, 1))
        prior[:, :3, :3], prior[:, :3, 3] = _quat_rot(X[:, 3:7]), X[:, 0:3]
        prior = np.where(started[:, None, None], prior, T_last)
        trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
        trk.set_prior(0, list(prior), relative=False)
        trk.track_with_motion_model(B, th=15.0)
        trk.track_local_map(B, th=1.0)
        # the host round trip of the motion model: poses and statuses down, the filter in numpy
        pose = np.stack(trk.get_align(0, B)["T"])
        ok = trk.get_local_map(0, B)["status"] == 2
        it = np.where(started, dt_, 0.0)
        alpha = (0.27 / (0.27 + it))[:, None]
        g = alpha * g + (1 - alpha) * meas[t][:, 3:]
        Z = np.concatenate([pose[:, :3, 3], _rot_quat(pose[:, :3, :3]), meas[t][:, :3], meas[t][:, 3:] - g], 1)
        S = P[:, IMU_SEL][:, :, IMU_SEL] + np.eye(13) * (IMU_R * dt_ * dt_)
        Kg = P[:, :, IMU_SEL] @ np.linalg.inv(S)
        Xu = X + (Kg @ (Z - X[:, IMU_SEL])[..., None])[..., 0]
        Pu = P - Kg @ S @ Kg.transpose(0, 2, 1)
        Xi = np.zeros((B, 16))
        Xi[:, :7] = Z[:, :7]
        upd, init = (ok & started), (ok & ~started)
        X0 = np.zeros(16)
        X0[3] = 1.0
        X = np.where(upd[:, None], Xu, np.where(init[:, None], Xi, X0))
        P = np.where(upd[:, None, None], Pu, np.where(init[:, None, None], P, IMU_P0))
        g = np.where(upd[:, None], g, 0.0)
        started = ok
        trk.advance(B, 1)
        T_last = pose
    st = trk.get_local_map(0, B)["status"]
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    return dt, st


def run_rgbd(B, seqs, mode):
    frames, ext, maps, vel = setup(B, seqs)
    raw = np.stack([np.stack([np.round(seqs[b % NU]["depth"][t] * 5000.0).astype(np.uint16) for b in range(B)]) for t in range(T)])
    if mode == "device_u16":
        dmaps = sdslam_amd.DeviceBuffer(raw.nbytes)
        dmaps.upload(raw)
    else:
        conv = [raw[t].astype(np.float32) * (np.float32(1) / np.float32(5000)) for t in range(T)]
    del raw
    trk = new_tracker(ext[0], ext[1], B, maps, seqs)
    trk.set_camera(*K, BF, BOUNDS)
    t0 = time.perf_counter()
    for t in range(1, T):
        trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
        if mode == "device_u16":
            trk.stereo_from_depth_device(dmaps.ptr.value + t * B * F * 2, trk.DEPTH_U16, 640, 480, depth_map_factor=5000.0)
        else:
            trk.stereo_from_depth(conv[t])
        trk.set_prior(0, vel[t - 1], relative=True)
        trk.track_with_motion_model(B, th=15.0, mono=False)
        trk.track_local_map(B, th=3.0)
        trk.close_points(B, 1, TH_CLOSE)
        trk.advance(B, 1)
    st = trk.get_local_map(0, B)["status"]        # synchronises
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    if mode == "device_u16":
        dmaps.free()
    return dt, st


def kf_setup(B, seqs):
    frames, ext, _, vel = setup(B, seqs)
    raw = np.stack([np.stack([np.round(seqs[b % NU]["depth"][t] * 5000.0).astype(np.uint16) for b in range(B)]) for t in range(T)])
    dmaps = sdslam_amd.DeviceBuffer(raw.nbytes)
    dmaps.upload(raw)
    return frames, ext, vel, dmaps


def kf_tracker(cur, ref, B):
    trk = sdslam_amd.Tracker(cur, ref, max_points=M, max_batch=B, pnp_max_iterations=100)
    trk.set_camera(*K, BF, BOUNDS)
    return trk


def kf_frame(trk, frames, dmaps, B, t):
    trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, 640, 480)
    trk.stereo_from_depth_device(dmaps.ptr.value + t * B * F * 2, trk.DEPTH_U16, 640, 480, depth_map_factor=5000.0)


def run_kf_device(B, seqs):
    frames, ext, vel, dmaps = kf_setup(B, seqs)
    trk = kf_tracker(ext[0], ext[1], B)
    state = np.array([KF_STATE] * B, np.int32)
    trk.set_keyframe_state(0, state)
    state[:, 2] = trk.KF_KEEP
    kf_frame(trk, frames, dmaps, B, 0)
    trk.stereo_init(B, 500)
    trk.advance(B, 2)
    trk.get_last(0, 1)                            # synchronises
    t0 = time.perf_counter()
    for t in range(1, T):
        kf_frame(trk, frames, dmaps, B, t)
        trk.set_prior(0, vel[t - 1], relative=True)
        trk.set_keyframe_state(0, state)
        trk.track_with_motion_model(B, th=15.0, mono=False)
        trk.track_local_map(B, th=3.0)
        trk.close_points(B, 1, TH_CLOSE)
        trk.need_keyframe(B, True, t, KF_MIN_FRAMES, KF_MAX_FRAMES)
        trk.create_keyframe_points(B, 1, TH_CLOSE, use_flags=True, frame_id=t)
        trk.advance(B, 1)
    st = trk.get_local_map(0, B)["status"]        # synchronises
    dt = time.perf_counter() - t0
    trk.close()
    frames.free()
    dmaps.free()
    return dt, st


def unproject(u, v, z, Tcw):
    """Frame::UnprojectStereo for arrays, in the operation order of include/sdslam_hip.h."""
    f32 = np.float32
    x = (u - f32(K[2])) * z * (f32(1) / f32(K[0]))
    y = (v - f32(K[3])) * z * (f32(1) / f32(K[1]))
    c = np.stack([x, y, z], 1).astype(np.float64)
    Rwc, t = Tcw[:3, :3].T, Tcw[:3, 3]
    Ow = -((Rwc[:, 0] * t[0] + Rwc[:, 1] * t[1]) + Rwc[:, 2] * t[2])
    return ((c[:, 0:1] * Rwc[:, 0] + c[:, 1:2] * Rwc[:, 1]) + c[:, 2:3] * Rwc[:, 2]) + Ow


def run_kf_host(B, seqs):
    frames, ext, vel, dmaps = kf_setup(B, seqs)
    trks = [kf_tracker(ext[0], ext[1], B), kf_tracker(ext[1], ext[0], B)]
    th = np.float32(TH_CLOSE)
    # frame 0 on the device, mirrored to the host once (outside the timed region)
    kf_frame(trks[1], frames, dmaps, B, 0)
    trks[1].stereo_init(B, 500)
    c = trks[1].get_created(0, B)
    kps, desc, nk = trks[1].cur.download(0, B)
    cases, idl = [], []
    for b in range(B):
        n, k = nk[b], c["created"][b]
        v = np.zeros(n, np.uint8)
        X, ids = np.zeros((n, 3)), np.full(n, -1, np.int32)
        i = c["kp_index"][b, :k]
        v[i], X[i], ids[i] = 1, c["Xw"][b, :k], c["ids"][b, :k]
        cases.append(dict(valid=v, Xw=X, desc=desc[b, :n] * v[:, None], octave=kps["octave"][b, :n], angle=kps["angle"][b, :n], obs=v.astype(np.int32)))
        idl.append(ids)
    trks[0].set_last(0, cases)
    trks[0].set_map_ids(0, idl, 0)
    next_id = c["created"].astype(np.int64).copy()
    last_kf = np.zeros(B, np.int64)
    T_last = [np.eye(4)] * B
    bi = np.arange(B)[:, None]
    t0 = time.perf_counter()
    for t in range(1, T):
        trk, nxt = trks[(t - 1) % 2], trks[t % 2]
        trk.set_poses(0, T_last, [v @ Tl for v, Tl in zip(vel[t - 1], T_last)])
        kf_frame(trk, frames, dmaps, B, t)
        trk.track_with_motion_model(B, th=15.0, mono=False)
        trk.track_local_map(B, th=3.0)
        # the host round trip: decision, creation, hand-off
        lm, po, last = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_last(0, B)
        _, dd = trk.get_stereo(0, B)
        kps, desc, nk = trk.cur.download(0, B)
        m = lm["match"][:, :M]
        j = np.clip(m, 0, M - 1)
        has = (m >= 0) & (last["obs"][bi, j] >= 1) & (np.arange(m.shape[1])[None] < nk[:, None])
        keep = has & ~po["outlier"][:, :M]
        close = (dd > 0) & (dd < th) & (np.arange(dd.shape[1])[None] < nk[:, None])
        n_tr, n_non = (close & keep).sum(1), (close & ~keep).sum(1)
        inl = lm["n_inliers"]
        need_close = (n_tr < 100) & (n_non > 70)
        c1 = (t >= last_kf + KF_MAX_FRAMES) | (t >= last_kf + KF_MIN_FRAMES) | (inl.astype(np.float64) < KF_STATE[1] * 0.25) | need_close
        c2 = ((inl.astype(np.float32) < np.float32(KF_STATE[1]) * np.float32(0.75)) | need_close) & (inl > 15)
        insert = c1 & c2 & (lm["status"] == 2)
        Xw = last["Xw"][bi, j] * keep[..., None]
        dsc = last["desc"][bi, j] * keep[..., None]
        ids = np.where(keep, last["ids"][bi, j], -1)
        obs = last["obs"][bi, j] * keep
        valid = keep.copy()
        for b in np.nonzero(insert)[0]:
            n = nk[b]
            d = dd[b, :n]
            order = np.argsort(np.where(d > 0, d, np.inf), kind="stable")[:int((d > 0).sum())]
            far = np.nonzero((d[order] > th) & (np.arange(len(order)) >= 100))[0]
            pre = order[:far[0] + 1] if len(far) else order
            new = pre[~has[b, pre]]
            valid[b, new], obs[b, new], dsc[b, new] = True, 1, desc[b, new]
            Xw[b, new] = unproject(kps["x"][b, new], kps["y"][b, new], d[new], po["T"][b])
            ids[b, new] = next_id[b] + np.arange(len(new))
            next_id[b] += len(new)
            last_kf[b] = t
        cases = [dict(valid=valid[b, :nk[b]].astype(np.uint8), Xw=Xw[b, :nk[b]], desc=dsc[b, :nk[b]], octave=kps["octave"][b, :nk[b]],
                      angle=kps["angle"][b, :nk[b]], obs=obs[b, :nk[b]]) for b in range(B)]
        nxt.set_last(0, cases)
        nxt.set_map_ids(0, [ids[b, :nk[b]] for b in range(B)], 0)
        T_last = po["T"]
    st = trks[(T - 2) % 2].get_local_map(0, B)["status"]
    dt = time.perf_counter() - t0
    for trk in trks:
        trk.close()
    frames.free()
    dmaps.free()
    return dt, st


def run_host(B, seqs):
    frames, ext, maps, vel = setup(B, seqs)
    trks = [new_tracker(ext[0], ext[1], B, maps, seqs), new_tracker(ext[1], ext[0], B, maps, seqs)]
    local_ids = np.stack([np.pad(m[2], (0, M - len(m[2])), constant_values=-1) for m in maps])
    lXw = np.zeros((B, M, 3))
    ldesc = np.zeros((B, M, 32), np.uint8)
    lobs = np.zeros((B, M), np.int32)
    for b, m in enumerate(maps):
        n = len(m[2])
        lXw[b, :n], ldesc[b, :n], lobs[b, :n] = m[0]["Xw"], m[0]["desc"], m[0]["obs"]
    T_last = [seqs[b % NU]["T"][0] for b in range(B)]
    t0 = time.perf_counter()
    for t in range(1, T):
        trk = trks[(t - 1) % 2]
        nxt = trks[t % 2]
        prior = [v @ Tl for v, Tl in zip(vel[t - 1], T_last)]
        trk.set_poses(0, T_last, prior)
        track(trk, frames, B, t)
        # the host hand-off
        lm, po, last = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_last(0, B)
        kps, _, nk = trk.cur.download(0, B)
        m = lm["match"][:, :M]
        keep = (m >= 0) & ~po["outlier"][:, :M]
        loc = m >= M
        j = np.clip(np.where(loc, m - M, m), 0, M - 1)
        bi = np.arange(B)[:, None]
        obs = np.where(loc, lobs[bi, j], last["obs"][bi, j])
        keep &= obs >= 1
        Xw = np.where(loc[..., None], lXw[bi, j], last["Xw"][bi, j]) * keep[..., None]
        desc = np.where(loc[..., None], ldesc[bi, j], last["desc"][bi, j]) * keep[..., None]
        ids = np.where(keep, np.where(loc, local_ids[bi, j], last["ids"][bi, j]), -1)
        cases = [dict(valid=keep[b, :nk[b]].astype(np.uint8), Xw=Xw[b, :nk[b]], desc=desc[b, :nk[b]], octave=kps["octave"][b, :nk[b]],
                      angle=kps["angle"][b, :nk[b]], obs=(obs * keep)[b, :nk[b]]) for b in range(B)]
        nxt.set_last(0, cases)
        nxt.set_map_ids(0, [ids[b, :nk[b]] for b in range(B)], 0)
        T_last = po["T"]
    st = trks[(T - 2) % 2].get_local_map(0, B)["status"]
    dt = time.perf_counter() - t0
    for trk in trks:
        trk.close()
    frames.free()
    return dt, st


def main():
    seqs = [synth.make_sequence(100 + i, T, with_depth=RGBD) for i in range(NU)]
    fns = dict(device=run_device, mono=run_device, host=run_host, host_f32=lambda B, s: run_rgbd(B, s, "host_f32"),
               device_u16=lambda B, s: run_rgbd(B, s, "device_u16"), kf_device=run_kf_device, kf_host=run_kf_host,
               ekf_device=run_ekf_device, ekf_host=run_ekf_host, imu_device=run_imu_device, imu_host=run_imu_host)
    out = []
    for B in BS:
        for mode in MODES:
            dt, st = fns[mode](B, seqs)
            r = dict(metric="seq_track", mode=mode, B=B, T=T, seconds=round(dt, 4), frames_per_s=round(B * (T - 1) / dt, 1),
                     ms_per_step=round(1e3 * dt / (T - 1), 3), tracked_last_frame=float(np.mean(st == 2)))
            if mode in ("host_f32", "device_u16"):
                r["depth_bytes_copied_per_step"] = B * F * 4 if mode == "host_f32" else 0
            print(json.dumps(r), flush=True)
            out.append(r)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "seq_bench_imu.json" if IMU else "seq_bench_motion.json" if EKF else "seq_bench_rgbd_kf.json" if KF else "seq_bench_rgbd.json" if RGBD else "seq_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
