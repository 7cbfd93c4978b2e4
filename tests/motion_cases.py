"""Inputs shared by the motion-model tests (helper, no tests): the per-frame twists (v, w) that exercise every branch of
ConstantVelocity::Exp / Log and of the matrix -> quaternion conversion, and the step schedule of the filter test."""
import numpy as np

_AX = np.array([1.0, 0.3, 0.2]) / np.linalg.norm([1.0, 0.3, 0.2])

# name -> twist; the branch each one is there for is asserted in tests/test_motion_cpu.py
TWISTS = {
    "zero": np.zeros(6),
    "translation": np.array([0.01, -0.02, 0.005, 0.0, 0.0, 0.0]),              # exactly zero rotation
    "rot_1e-11": np.array([0.01, 0.0, -0.01, 6e-12, -8e-12, 0.0]),             # below SMALL_EPS
    "rot_1e-6": np.array([-0.01, 0.02, 0.0, 0.0, 6e-7, 8e-7]),
    "sequence": np.array([0.01, -0.002, 0.003, 0.004, -0.004, 0.002]),         # the sequence generator's ~ (1 cm, 6 mrad)
    "rot_0.5": np.array([0.02, 0.01, -0.01, 0.3, -0.3, 0.264575131106459]),
    "rot_x": np.array([0.01, 0.0, 0.005, 2.5, 0.05, -0.04]),                   # beyond 120 degrees: trace < 0, largest diagonal x
    "rot_y": np.array([0.0, 0.01, 0.005, 0.05, 2.5, -0.04]),                   # ... y
    "rot_z": np.array([0.005, 0.01, 0.0, -0.04, 0.05, 2.5]),                   # ... z
    "w_negative": np.concatenate([[0.01, -0.01, 0.02], -2.4 * _AX]),           # the converted quaternion has w < 0
}
NAMES = list(TWISTS)

# dt per step: 1/30 and 0.1 on alternate steps, one step with dt = 0
DTS = [1.0 / 30.0, 0.1, 1.0 / 30.0, 0.1, 0.0, 1.0 / 30.0, 0.1, 1.0 / 30.0]


def slot_twist(i):
    return TWISTS[NAMES[i % len(NAMES)]]
