"""The yardstick of the sensor / command front end's tests (tests/test_frontend_host.py on the CPU, tests/test_gpu_sensor_frontend.py on the GPU): a numpy restatement,
written from the reference's source and Eigen's, of what the C ABI's a1mpc_sensor_frontend_batch and a1mpc_command_batch are documented to equal, and the inputs both
suites feed.  float64 scalar arithmetic of numpy is IEEE add / subtract / multiply / divide / sqrt, one rounding each and never contracted: what the kernels are built
to reproduce bit for bit.  The angles and the filters come from the reference's own compiled code (oracle/_ref: ref_quat_to_euler, ref_filter_run), not from here."""
import math

import numpy as np

SIZES = (1, 63, 64, 65, 257)   # one lane, either side of a wavefront edge, past one 256-thread workgroup
ROOT_HALF = np.sqrt(0.5)


# ---------------------------------------------------------------------------------------------------------------- the two rotation matrices
def quat_to_rotation(q):
    """Eigen::QuaternionBase::toRotationMatrix (Eigen/src/Geometry/Quaternion.h) as gt_pose_callback calls it, S/GazeboA1ROS.cpp:258: q = (w, x, y, z), NOT normalised;
    (n, 4) -> (n, 9) row-major.  Operation order as there: tx = 2x, ty = 2y, tz = 2z, twx = tx * w, ..., R00 = 1 - (tyy + tzz)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(invalid="ignore"):
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        return np.stack([1.0 - (tyy + tzz), txy - twz, txz + twy,
                         txy + twz, 1.0 - (txx + tzz), tyz - twx,
                         txz - twy, tyz + twx, 1.0 - (txx + tyy)], axis=1)


_libm = lambda f: np.vectorize(f, otypes=[np.float64])   # the C library's sin / cos, what the reference's compiled code calls (numpy's array loops are its own)


def yaw_rotation(yaw, sin=_libm(math.sin), cos=_libm(math.cos)):
    """Eigen::AngleAxisd(yaw, Vector3d::UnitZ()).toRotationMatrix() (Eigen/src/Geometry/AngleAxis.h), S/GazeboA1ROS.cpp:262, with the axis (0, 0, 1) written out:
    sin_axis = sin(angle) * axis, c = cos(angle), cos1_axis = (1 - c) * axis; tmp = cos1_axis.x * axis.y: (0,1) = tmp - sin_axis.z, (1,0) = tmp + sin_axis.z;
    tmp = cos1_axis.x * axis.z: (0,2) = tmp + sin_axis.y, (2,0) = tmp - sin_axis.y; tmp = cos1_axis.y * axis.z: (1,2) = tmp - sin_axis.x, (2,1) = tmp + sin_axis.x;
    diagonal = cos1_axis .* axis + c -- so (2,2) is (1 - c) + c.  (n,) -> (n, 9) row-major."""
    yaw = np.asarray(yaw, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        s, c = sin(yaw), cos(yaw)
        ax, ay, az = 0.0, 0.0, 1.0
        sx, sy, sz = s * ax, s * ay, s * az
        cx, cy, cz = (1.0 - c) * ax, (1.0 - c) * ay, (1.0 - c) * az
        t01 = cx * ay; t02 = cx * az; t12 = cy * az
        return np.stack([cx * ax + c, t01 - sz, t02 + sy,
                         t01 + sz, cy * ay + c, t12 - sx,
                         t02 - sy, t12 + sx, cz * az + c], axis=1)


def assert_yaw_rotation(Rz, yaw, tol):
    """R_z against yaw_rotation(yaw) within `tol` absolute, and what holds exactly whatever library evaluates sin and cos: the four elements that are products with the
    axis' zeros are zero, (0,1) = -(1,0), (0,0) = (1,1); a NaN yaw fills its row and no other.
    tol on the host is 1e-15: the compiler may call sincos() where this file calls sin() and cos(), and glibc documents each within one ulp of the true value, so two
    evaluations of an element of magnitude <= 1 lie within 2 ulp(1) = 4.5e-16 of each other, and (1 - c) + c adds two roundings of at most 1.2e-16 each.  On the GPU
    it is the 1e-12 the reference pin uses for quat_to_euler (tests/test_ref_pin.py)."""
    want = yaw_rotation(yaw)
    nan = np.isnan(np.asarray(yaw))
    assert np.array_equal(np.isnan(Rz).all(1), nan) and np.array_equal(np.isnan(Rz).any(1), nan)
    got, want = Rz[~nan], want[~nan]
    worst = float(np.abs(got - want).max()) if len(got) else 0.0
    assert worst <= tol, worst
    assert not got[:, [2, 5, 6, 7]].any() and np.array_equal(got[:, 1], -got[:, 3]) and np.array_equal(got[:, 0], got[:, 4])
    return worst


def rotate(R, v):
    """root_ang_vel = root_rot_mat * imu_ang_vel, S/GazeboA1ROS.cpp:299: every row a three-term sum, left to right; (n, 9), (n, 3) -> (n, 3)"""
    R = np.asarray(R).reshape(-1, 3, 3); v = np.asarray(v).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.stack([(R[:, i, 0] * v[:, 0] + R[:, i, 1] * v[:, 1]) + R[:, i, 2] * v[:, 2] for i in range(3)], axis=1)


def reference_euler(REF, q):
    """Utils::quat_to_euler of the reference's own compiled code, row by row; (n, 4) as w, x, y, z -> (n, 3)"""
    return np.array([REF.quat_to_euler(*row) for row in np.asarray(q, dtype=np.float64).reshape(-1, 4)])


def t2_of(q):
    """the argument of asin before its clamp, S/utils/Utils.cpp:24"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    return 2.0 * (q[:, 0] * q[:, 2] - q[:, 3] * q[:, 1])


def quaternion_rows(rng, n):
    """(n, 4) as w, x, y, z: seeded random unit quaternions, and over them (as far as n reaches; row n // 2 for the NaN) the special rows of the tests: identity, w < 0,
    a non-unit one (scale 1.001), both gimbal-lock poles w = y = +-sqrt(1/2) scaled so that t2 leaves [-1, 1] and the clamp acts, a NaN row"""
    q = rng.normal(0, 1, (n, 4)); q /= np.linalg.norm(q, axis=1)[:, None]
    up = np.nextafter(ROOT_HALF, 1.0)
    special = [(1.0, 0.0, 0.0, 0.0), None, None, (up, 0.0, up, 0.0), (up, 0.0, -up, 0.0), (-up, 0.0, up, 0.0)]
    for k, row in enumerate(special[:n]):
        if row is not None:
            q[k] = row
    if n > 1:
        q[1] = -np.abs(q[1])          # w < 0 (and the rest with it: still a unit quaternion)
    if n > 2:
        q[2] = q[2] * 1.001           # not normalised
    if n >= 16:
        q[n // 2, 2] = np.nan
    return np.ascontiguousarray(q)


def assert_special_rows_are_special(q):
    n = len(q)
    if n > 5:
        t2 = t2_of(q)
        assert t2[3] > 1.0 and t2[4] < -1.0 and t2[5] < -1.0, t2[:6]      # the clamp acts, on both sides
        assert q[1, 0] < 0 and abs(np.linalg.norm(q[2]) - 1.001) < 1e-12
    if n >= 16:
        assert np.isnan(q[n // 2]).any() and np.isnan(q).any(1).sum() == 1


# ---------------------------------------------------------------------------------------------------------------- the IMU samples
def imu_sequence(rng, calls, n):
    """(calls, n, 6) raw samples (acc x, y, z, gyro x, y, z) that take BOTH branches of the Neumaier update in every channel: magnitudes from 1e-8 to 1e8 drawn log-uniformly
    with alternating signs, so that the running sum is now larger, now smaller than the value added (S/utils/filter.hpp:55-60)"""
    mag = 10.0 ** rng.uniform(-8, 8, (calls, n, 6))
    sign = np.where((np.arange(calls)[:, None, None] + np.arange(6)[None, None, :] + np.arange(n)[None, :, None]) % 2 == 0, 1.0, -1.0)
    return np.ascontiguousarray(mag * sign)


def neumaier_branches(window, x):
    """how often a channel's samples took the `sum is larger` / `value is larger` branch (subtractions of the oldest sample included)"""
    s = 0.0; big = small = 0; q = []
    for v in x:
        for val in ([-q.pop(0)] if len(q) >= window else []) + [v]:
            if abs(s) >= abs(val): big += 1
            else: small += 1
            s = s + val
        q.append(v)
    return big, small


def assert_samples_take_both_branches(seq, windows):
    """the input-side assertion: every channel of the first robot takes both Neumaier branches at every window, the magnitudes span 1e-6 .. 1e6 at the least and
    the sign alternates from call to call"""
    for w in windows:
        for k in range(6):
            big, small = neumaier_branches(w, seq[:, 0, k])
            assert big > 0 and small > 0, (w, k)
    assert (seq[1:] * seq[:-1] < 0).all()
    if seq.shape[1] >= 16:
        assert np.abs(seq).min() < 1e-6 and np.abs(seq).max() > 1e6


def reference_filters(REF, window, seq):
    """ref_filter_run (MovingWindowFilter::CalculateAverage of the reference's compiled code) per robot and channel over the calls; (calls, n, 6) -> the same shape"""
    out = np.empty_like(seq)
    for b in range(seq.shape[1]):
        for k in range(6):
            out[:, b, k] = REF.filter_run(window, np.ascontiguousarray(seq[:, b, k]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the command stage
COMMAND_DEFAULTS = dict(body_height_max=0.32, body_height_min=0.1, kp_linear_lock_x=120.0, kp_linear_lock_y=120.0, lock_speed=0.05, mpc_init_ticks=10)
STATE_KEYS = ("body_height", "ctrl_state", "root_euler_d", "root_pos_d", "kp_linear_xy", "mpc_init_counter")
OUT_KEYS = ("root_lin_vel_d", "root_ang_vel_d", "movement_mode", "mpc_active", "root_pos_d_z")


def initial_state(n):
    """the reference's initial values: joy_cmd_body_height 0.3 (S/GazeboA1ROS.h:130), joy_cmd_ctrl_state 0, root_pos_d / root_euler_d zero (S/A1CtrlStates.h:35-36),
    kp_linear (a1_kp_linear_x, a1_kp_linear_y) = 120 (S/A1CtrlStates.h:273-274, 301), mpc_init_counter 0 (S/A1RobotControl.cpp:25)"""
    return dict(body_height=np.full(n, 0.3), ctrl_state=np.zeros(n, np.uint8), root_euler_d=np.zeros((n, 3)), root_pos_d=np.zeros((n, 3)),
                kp_linear_xy=np.full((n, 2), 120.0), mpc_init_counter=np.zeros(n, np.int32))


def command_step(state, cmd, toggle, root_pos, dt, cfg=COMMAND_DEFAULTS):
    """main_update's first half, S/GazeboA1ROS.cpp:124-188, and the gate of compute_joint_torques, S/A1RobotControl.cpp:292-294, one robot after the other in the
    reference's statement order; `state` (initial_state) is updated in place, the outputs of the tick are returned"""
    n = len(cmd)
    out = dict(root_lin_vel_d=np.zeros((n, 3)), root_ang_vel_d=np.zeros((n, 3)), movement_mode=np.zeros(n, np.uint8), mpc_active=np.zeros(n, np.uint8), root_pos_d_z=np.zeros(n))
    dt = np.float64(dt)
    for b in range(n):
        velx, vely, velz, roll_rate, pitch_rate, yaw_rate = (np.float64(v) for v in cmd[b])
        h = state["body_height"][b] + velz * dt                                  # :124
        if h >= cfg["body_height_max"]: h = np.float64(cfg["body_height_max"])    # :125-127
        if h <= cfg["body_height_min"]: h = np.float64(cfg["body_height_min"])    # :128-130
        state["body_height"][b] = h
        prev = int(state["ctrl_state"][b])                                       # :140
        cs = prev
        if toggle[b]: cs = (cs + 1) % 2                                          # :142-147
        state["ctrl_state"][b] = cs
        out["root_lin_vel_d"][b] = (velx, vely, velz)                            # :150-152
        out["root_ang_vel_d"][b] = (roll_rate, pitch_rate, yaw_rate)             # :155-157
        state["root_euler_d"][b, 0] += roll_rate * dt                            # :158-160
        state["root_euler_d"][b, 1] += pitch_rate * dt
        state["root_euler_d"][b, 2] += yaw_rate * dt
        state["root_pos_d"][b, 2] = h                                            # :161
        if cs == 1:                                                              # :164-176
            mode = 1
        elif cs == 0 and prev == 1:
            mode = 0
            state["root_pos_d"][b, :2] = root_pos[b, :2]
            state["kp_linear_xy"][b] = (cfg["kp_linear_lock_x"], cfg["kp_linear_lock_y"])
        else:
            mode = 0
        if mode == 1:                                                            # :179-188
            if np.sqrt(velx * velx + vely * vely) > cfg["lock_speed"]:
                state["root_pos_d"][b, :2] = root_pos[b, :2]
                state["kp_linear_xy"][b] = (0.0, 0.0)
            else:
                state["kp_linear_xy"][b] = (cfg["kp_linear_lock_x"], cfg["kp_linear_lock_y"])
        state["mpc_init_counter"][b] += 1                                        # S/A1RobotControl.cpp:292
        out["movement_mode"][b] = mode
        out["mpc_active"][b] = 0 if state["mpc_init_counter"][b] < cfg["mpc_init_ticks"] else 1   # :294
        out["root_pos_d_z"][b] = h
    return out


TICKS = 16
_NEXT = lambda v: np.nextafter(v, np.inf)
_PREV = lambda v: np.nextafter(v, -np.inf)
# (vx, vy) on and one ulp either side of lock_speed = 0.05: (0.05, 0) has norm 0.05 exactly (not above: lock); (0.03, 0.04) is 0.05 in exact arithmetic -- float64 decides
SPEEDS = [(0.05, 0.0), (_NEXT(0.05), 0.0), (_PREV(0.05), 0.0), (0.03, 0.04), (_NEXT(0.03), 0.04), (_PREV(0.03), 0.04), (0.03, _NEXT(0.04)), (0.03, _PREV(0.04)),
          (0.0, 0.0), (0.4, -0.2), (-0.05, 0.0), (0.0, -_NEXT(0.05))]


def command_script(rng, n, dt=0.0025):
    """(cmd (TICKS, n, 6), toggle (TICKS, n) uint8, root_pos (TICKS, n, 3)) -- a 16-tick script per robot, eight scripts dealt out lane by lane (lane % 8) so that the
    lanes of one wavefront diverge at every branch:
      toggle on at tick 2 + script % 3, walk above lock_speed, walk below it, toggle off around tick 9 (the one-tick lock), stand; script 7 never walks, script 6 toggles
      twice in a row; the speeds of SPEEDS on the walking ticks; velz drives the body height into the upper clamp (scripts 0-2), into the lower (3-4: a large velz), and
      onto 0.32 exactly (script 5: 0.3 + 8 * 0.0025 lands on the clamp's value by rounding or passes it -- either way >= acts)"""
    cmd = np.zeros((TICKS, n, 6)); toggle = np.zeros((TICKS, n), np.uint8)
    root_pos = np.cumsum(rng.normal(0, 0.01, (TICKS, n, 3)), axis=0) + np.array([0.0, 0.0, 0.3])
    for b in range(n):
        s = b % 8
        on, off = 2 + s % 3, 9 + s % 2
        if s != 7:
            toggle[on, b] = 1; toggle[off, b] = 1
        if s == 6:
            toggle[on + 1, b] = 1; toggle[on + 2, b] = 1     # off after one walking tick, on again
        for t in range(TICKS):
            vx, vy = SPEEDS[(t + 3 * s + b // 8) % len(SPEEDS)]
            velz = (0.5, 0.5, 2.0, -30.0, -3.0, 1.0, 0.0, 0.04)[s] * (1.0 if t < 10 else -0.3)
            if s in (2, 3) and t in (7, 8):
                velz = 0.0                                   # the height sits ON its clamp (0.32 / 0.1) and stays: h + 0 * dt == the bound, >= / <= act on equality
            cmd[t, b] = (vx, vy, velz, rng.normal(0, 0.2), rng.normal(0, 0.2), rng.uniform(-0.5, 0.5))
    return cmd, toggle, root_pos
