"""ctypes binding of liba1mpc.so -- the host-side mirror of the reference interface for the hot path.

The reference is C++ (ConvexMpc + A1RobotControl::compute_grf); the C++ adapter with the reference's own
class interface is include/a1mpc_convex_mpc.hpp.  This module is the Python plumbing the tests and
bench.py use: numpy arrays in the C-ABI layouts in, GRFs out.  There is no fallback: if the HIP library is
missing, or there is no GPU, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

NS, NU, NC = 13, 12, 20
STATUS_NAMES = {1: "solved", 2: "solved_inaccurate", -2: "max_iter_reached", -7: "non_cvx", -10: "unsolved"}
SUPPORTED_HORIZONS = (1, 4, 6, 8, 10, 12, 14, 16, 20)   # (1, 10, 16, 20: tuned; the others: the kernel families as they instantiate)


class Config(C.Structure):  # a1mpc_config, include/a1mpc.h
    _fields_ = [("horizon", C.c_int32), ("dt", C.c_double), ("mu", C.c_double), ("fz_min", C.c_double),
                ("fz_max", C.c_double), ("q", C.c_double * NS), ("r", C.c_double * NU), ("mass", C.c_double),
                ("inertia_body", C.c_double * 9), ("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double),
                ("eps_abs", C.c_double), ("eps_rel", C.c_double), ("adaptive_rho_tolerance", C.c_double),
                ("max_iter", C.c_int32), ("check_termination", C.c_int32), ("adaptive_rho", C.c_int32),
                ("adaptive_rho_interval", C.c_int32), ("scaling", C.c_int32), ("warm_start", C.c_int32)]


class BalanceConfig(C.Structure):  # a1mpc_balance_config
    _fields_ = [("Q", C.c_double * 6), ("R", C.c_double), ("mu", C.c_double), ("F_min", C.c_double), ("F_max", C.c_double)]


class GaitConfig(C.Structure):  # a1mpc_gait_config
    _fields_ = [("counter_per_gait", C.c_double), ("counter_per_swing", C.c_double), ("control_dt", C.c_double),
                ("foot_delta_x_limit", C.c_double), ("foot_delta_y_limit", C.c_double), ("default_foot_pos", C.c_double * 12),
                ("gait_counter_reset", C.c_double * 4)]


class ContactConfig(C.Structure):  # a1mpc_contact_config
    _fields_ = [("counter_per_swing", C.c_double), ("foot_force_low", C.c_double), ("use_terrain_adapt", C.c_int32)]


class TickParams(C.Structure):  # a1mpc_tick_params
    _fields_ = [("gait", GaitConfig), ("contact", ContactConfig), ("control_dt", C.c_double), ("assume_flat_ground", C.c_int32),
                ("kp_foot", C.c_double * 3), ("kd_foot", C.c_double * 3), ("km_foot", C.c_double * 3), ("rho_fix", C.c_double * 20), ("rho_opt", C.c_double * 12)]


class PreviewConfig(C.Structure):  # a1mpc_preview_config: the gait-aware horizon (contact schedule / foot preview)
    _fields_ = [("contact_schedule", C.c_int32), ("foot_preview", C.c_int32), ("ticks_per_step", C.c_int32)]


class BalanceGains(C.Structure):  # a1mpc_balance_gains: the PD gains of the balance controller's wrench (S/A1CtrlStates.h:117-120)
    _fields_ = [("kp_linear", C.c_double * 3), ("kd_linear", C.c_double * 3), ("kp_angular", C.c_double * 3), ("kd_angular", C.c_double * 3)]


class BalanceTick(C.Structure):  # a1mpc_balance_tick: what a1mpc_control_tick_balance_device takes beside TickParams / TickBuffers (device pointers)
    _fields_ = [("gains", BalanceGains), ("qp", BalanceConfig), ("root_pos_d", C.c_void_p), ("root_acc", C.c_void_p), ("f_world", C.c_void_p)]


class SensorConfig(C.Structure):  # a1mpc_sensor_config: the window of the six IMU filters (S/GazeboA1ROS.cpp:99-104)
    _fields_ = [("imu_window", C.c_int32)]


class CommandConfig(C.Structure):  # a1mpc_command_config: the constants of main_update's first half (S/GazeboA1ROS.cpp:124-188) and the mpc_init_counter gate
    _fields_ = [("body_height_max", C.c_double), ("body_height_min", C.c_double), ("kp_linear_lock_x", C.c_double), ("kp_linear_lock_y", C.c_double),
                ("lock_speed", C.c_double), ("mpc_init_ticks", C.c_int32)]


class PlantConfig(C.Structure):  # a1mpc_plant_config: one call of the single-rigid-body plant advances by dt in `substeps` sub-steps
    _fields_ = [("dt", C.c_double), ("substeps", C.c_int32), ("gravity_z", C.c_double)]


class WalkConfig(C.Structure):  # a1mpc_walk_config: the plant's configuration, how far a swing foot moves towards its target per call, the flat ground
    _fields_ = [("plant", PlantConfig), ("swing_track", C.c_double), ("flat_ground", C.c_int32), ("ground_z", C.c_double)]


class Heightfield(C.Structure):  # a1mpc_heightfield: a gridded field of heights under the walking plant; `height` is a device pointer in the _device entries
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("x0", C.c_double), ("y0", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("interp", C.c_int32),
                ("height", C.c_void_p)]


class NoiseConfig(C.Structure):  # a1mpc_noise_config: the generator's seed and the levels of the eight noise channels (0 = that channel is off)
    _fields_ = [("seed", C.c_uint64), ("gyro_sigma", C.c_double), ("acc_sigma", C.c_double), ("gyro_bias_walk", C.c_double), ("acc_bias_walk", C.c_double),
                ("att_sigma", C.c_double), ("joint_pos_sigma", C.c_double), ("joint_vel_sigma", C.c_double), ("foot_force_sigma", C.c_double)]


class EpisodeConfig(C.Structure):  # a1mpc_episode_config: when an episode ends -- R22 below min_up (tilt), the body less than min_height above its ground
    _fields_ = [("min_up", C.c_double), ("min_height", C.c_double)]


class RespawnConfig(C.Structure):  # a1mpc_respawn_config: which ended episodes start again, the time limit, the hold while the estimator is primed, the blocks cleared
    _fields_ = [("codes", C.c_uint32), ("max_ticks", C.c_uint64), ("hold_ticks", C.c_int32), ("what", C.c_uint32)]


class RespawnRows(C.Structure):  # a1mpc_respawn_rows: one entry of the table of a1mpc_respawn_rows_device
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("row_bytes", C.c_int32), ("src_rows", C.c_int32), ("when", C.c_uint32)]


RESPAWN_EKF, RESPAWN_CONTACT, RESPAWN_SENSOR, RESPAWN_WARM, RESPAWN_ROWS_MAX = 1, 2, 4, 8, 16   # A1MPC_RESPAWN_*
EPISODE_WORDS = 16   # doubles per robot of an episode record; all zero is the start of an episode
EPISODE_FIELDS = ("ticks", "end_tick_p1", "end_code", "vel_err_sum", "height_err_sum", "tilt_max", "est_pos_err_sum", "est_vel_err_sum", "est_vel_err_max", "effort_sum",
                  "fz_max", "solver_bad", "reach_bad", "x0", "y0", "dist2")
SUMMARY_FIELDS = ("n", "alive", "ended_nonfinite", "ended_tilt", "ended_height", "first_end_tick", "ticks", "vel_err_sum", "height_err_sum", "tilt_max", "tilt_max_row",
                  "est_pos_err_sum", "est_vel_err_sum", "est_vel_err_max", "effort_sum", "fz_max", "solver_bad", "reach_bad", "dist2_sum", "dist2_max")
# the optional inputs of a1mpc_episode_update_batch behind state and R_world, in its order: (name, columns (0: one value per robot), dtype)
EPISODE_INPUTS = (("root_pos", 3, np.float64), ("root_lin_vel", 3, np.float64), ("root_lin_vel_d", 3, np.float64), ("root_pos_d_z", 0, np.float64), ("ground", 3, np.float64),
                  ("grf_body", 12, np.float64), ("contacts", 4, np.uint8), ("status", 0, np.int32), ("reach", 4, np.uint8))
NOISE_SENSORS = ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")   # the arrays a1mpc_sensor_noise_batch works on in place, in its order
NOISE_WIDTHS = dict(quat=4, imu_acc_raw=3, imu_gyro_raw=3, joint_pos=12, joint_vel=12, foot_force=4, imu_bias=6, z=44)
TICK_SENSOR_POINTERS = ("quat", "imu_acc_raw", "imu_gyro_raw", "cmd", "mode_toggle", "body_height", "ctrl_state", "root_pos_d", "kp_linear_xy", "mpc_init_counter")
COMMAND_STATE_FIELDS = ("body_height", "ctrl_state", "root_euler_d", "root_pos_d", "kp_linear_xy", "mpc_init_counter")   # carried by the caller, in the C ABI's order


class TickSensors(C.Structure):  # a1mpc_tick_sensors: what a1mpc_control_tick_sensors_device takes beside TickParams / TickBuffers (device pointers)
    _fields_ = [("sensor", SensorConfig), ("command", CommandConfig)] + [(k, C.c_void_p) for k in TICK_SENSOR_POINTERS]


TICK_BUFFER_FIELDS = ("joint_pos", "joint_vel", "R_world", "R_z", "root_euler", "root_ang_vel", "imu_acc", "imu_ang_vel", "foot_force", "movement_mode", "mpc_active",
                      "root_lin_vel_d", "root_ang_vel_d", "root_pos_d_z", "gait_counter_speed", "torques_gravity", "gait_counter", "foot_pos_start", "foot_pos_rel_last_time",
                      "foot_pos_target_last_time", "root_euler_d", "joint_torques", "root_pos", "root_lin_vel", "estimated_contacts", "plan_contacts", "contacts", "foot_pos_rel",
                      "j_foot_blocks", "foot_vel_rel", "foot_pos_abs", "foot_vel_abs", "foot_pos_world", "foot_vel_world", "foot_pos_target_rel", "foot_pos_target_abs",
                      "foot_pos_target_world", "foot_pos_cur", "foot_forces_kin", "foot_pos_recent_contact", "terrain_angle", "grf", "iters", "status")


class TickBuffers(C.Structure):  # a1mpc_tick_buffers: device pointers, in the header's order
    _fields_ = [(k, C.c_void_p) for k in TICK_BUFFER_FIELDS]


EXPORTS = ["a1mpc_default_heightfield", "a1mpc_heightfield_step_batch", "a1mpc_heightfield_step_batch_device", "a1mpc_heightfield_sample_batch",
           "a1mpc_heightfield_sample_batch_device", "a1mpc_default_respawn_config", "a1mpc_respawn_reset_batch", "a1mpc_respawn_reset_batch_device", "a1mpc_respawn_batch", "a1mpc_respawn_batch_device",
           "a1mpc_respawn_rows_device", "a1mpc_default_episode_config", "a1mpc_episode_update_batch", "a1mpc_episode_update_batch_device", "a1mpc_episode_summary_batch",
           "a1mpc_episode_summary_batch_device", "a1mpc_default_noise_config", "a1mpc_sensor_noise_batch", "a1mpc_sensor_noise_batch_device",
           "a1mpc_ground_step_batch", "a1mpc_ground_step_batch_device", "a1mpc_touch_sensors_batch", "a1mpc_touch_sensors_batch_device",
           "a1mpc_default_walk_config", "a1mpc_walk_step_batch", "a1mpc_walk_step_batch_device", "a1mpc_walk_sensors_batch", "a1mpc_walk_sensors_batch_device",
           "a1mpc_sensor_synthesis_batch", "a1mpc_sensor_synthesis_batch_device", "a1mpc_default_plant_config", "a1mpc_plant_step_batch", "a1mpc_plant_step_batch_device",
           "a1mpc_default_sensor_config", "a1mpc_default_command_config", "a1mpc_reset_sensor_state", "a1mpc_sensor_frontend_batch", "a1mpc_sensor_frontend_batch_device",
           "a1mpc_command_batch", "a1mpc_command_batch_device", "a1mpc_control_tick_sensors_device", "a1mpc_balance_wrench_kp_batch", "a1mpc_balance_wrench_kp_batch_device",
           "a1mpc_default_balance_gains", "a1mpc_balance_wrench_batch", "a1mpc_balance_wrench_batch_device", "a1mpc_balance_solve_batch_device", "a1mpc_contacts_batch",
           "a1mpc_contacts_batch_device", "a1mpc_control_tick_balance_device",
           "a1mpc_horizon_states_batch", "a1mpc_horizon_states_batch_device", "a1mpc_horizon_states_ticks_batch", "a1mpc_horizon_states_ticks_batch_device",
           "a1mpc_horizon_preview_footholds_batch", "a1mpc_horizon_preview_footholds_batch_device", "a1mpc_control_tick_preview_footholds_device",
           "a1mpc_pipeline_submit_ticks_strided_device", "a1mpc_default_preview_config", "a1mpc_horizon_preview_batch", "a1mpc_horizon_preview_batch_device", "a1mpc_solve_batch_ticks_strided", "a1mpc_solve_batch_ticks_strided_device",
           "a1mpc_control_tick_preview_device", "a1mpc_set_timing", "a1mpc_default_tick_params", "a1mpc_control_tick_device", "a1mpc_last_control_tick_ms", "a1mpc_last_stage_ms", "a1mpc_sharded_create", "a1mpc_sharded_solve_batch", "a1mpc_sharded_solve_batch_ticks", "a1mpc_sharded_solve_batch_device", "a1mpc_sharded_solve_batch_ticks_device", "a1mpc_sharded_handle",
           "a1mpc_sharded_last_transfer", "a1mpc_sharded_info", "a1mpc_sharded_destroy", "a1mpc_terrain_batch", "a1mpc_form_qp_batch", "a1mpc_solve_batch_strided", "a1mpc_solve_batch_strided_device", "a1mpc_update_config", "a1mpc_warm_start", "a1mpc_get_warm_start", "a1mpc_get_workspace_z", "a1mpc_get_workspace_scaling", "a1mpc_last_warm_start_mode", "a1mpc_set_profiling", "a1mpc_last_stage_cycles", "a1mpc_last_tick_stage_cycles", "a1mpc_update_plan_batch_device", "a1mpc_swing_legs_batch_device", "a1mpc_contact_terrain_batch_device", "a1mpc_leg_state_batch_device",
           "a1mpc_ekf_update_batch_device", "a1mpc_joint_torques_batch_device", "a1mpc_ekf_update_batch", "a1mpc_reset_ekf_state", "a1mpc_leg_state_batch", "a1mpc_swing_legs_batch", "a1mpc_default_contact_config", "a1mpc_contact_terrain_batch", "a1mpc_reset_contact_state", "a1mpc_default_gait_config", "a1mpc_update_plan_batch", "a1mpc_joint_torques_batch", "a1mpc_set_schedule", "a1mpc_default_config", "a1mpc_default_balance_config", "a1mpc_create", "a1mpc_destroy", "a1mpc_solve_batch",
           "a1mpc_solve_batch_device", "a1mpc_solve_batch_ticks", "a1mpc_solve_batch_ticks_device", "a1mpc_balance_solve_batch", "a1mpc_reset_warm_start", "a1mpc_last_kernel_ms",
           "a1mpc_kernel_info", "a1mpc_last_nfact", "a1mpc_status_string", "a1mpc_last_error", "a1mpc_build_info", "a1mpc_pipeline_create", "a1mpc_pipeline_submit_device", "a1mpc_pipeline_submit",
           "a1mpc_pipeline_submit_strided_device", "a1mpc_pipeline_submit_strided", "a1mpc_pipeline_submit_ticks_device", "a1mpc_pipeline_wait", "a1mpc_pipeline_join", "a1mpc_pipeline_handle", "a1mpc_pipeline_depth", "a1mpc_pipeline_destroy"]

_lib = None


class A1MpcError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen liba1mpc.so (no compute).  Raises if the library has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or _build.LIB_PATH
    if not os.path.exists(path):
        raise A1MpcError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback for the solver)")
    lib = C.CDLL(path)
    vp, i32, dp, u8p, i32p = C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    lib.a1mpc_default_config.argtypes = [C.POINTER(Config)]; lib.a1mpc_default_config.restype = None
    lib.a1mpc_default_balance_config.argtypes = [C.POINTER(BalanceConfig)]; lib.a1mpc_default_balance_config.restype = None
    lib.a1mpc_create.argtypes = [C.POINTER(Config), i32, i32, C.POINTER(vp)]; lib.a1mpc_create.restype = C.c_int
    lib.a1mpc_destroy.argtypes = [vp]; lib.a1mpc_destroy.restype = None
    lib.a1mpc_solve_batch.argtypes = [vp, i32, dp, dp, dp, dp, u8p, dp, dp, i32p, i32p]; lib.a1mpc_solve_batch.restype = C.c_int
    lib.a1mpc_solve_batch_device.argtypes = [vp, i32] + [vp] * 9 + [vp]; lib.a1mpc_solve_batch_device.restype = C.c_int
    lib.a1mpc_solve_batch_ticks.argtypes = [vp, i32, dp, dp, dp, u8p, dp, dp, i32p, i32p]; lib.a1mpc_solve_batch_ticks.restype = C.c_int
    lib.a1mpc_solve_batch_ticks_device.argtypes = [vp, i32] + [vp] * 8 + [vp]; lib.a1mpc_solve_batch_ticks_device.restype = C.c_int
    lib.a1mpc_balance_solve_batch.argtypes = [vp, C.POINTER(BalanceConfig), i32, dp, dp, dp, dp, u8p, dp, dp, i32p, i32p]
    lib.a1mpc_balance_solve_batch.restype = C.c_int
    lib.a1mpc_default_gait_config.argtypes = [C.POINTER(GaitConfig)]; lib.a1mpc_default_gait_config.restype = None
    lib.a1mpc_update_plan_batch.argtypes = [vp, C.POINTER(GaitConfig), i32, u8p, dp, dp, dp, dp, dp, dp, dp, u8p, dp, dp, dp]
    lib.a1mpc_update_plan_batch.restype = C.c_int
    lib.a1mpc_joint_torques_batch.argtypes = [vp, i32, u8p, u8p, dp, dp, dp, dp, dp, dp]; lib.a1mpc_joint_torques_batch.restype = C.c_int
    lib.a1mpc_default_contact_config.argtypes = [C.POINTER(ContactConfig)]; lib.a1mpc_default_contact_config.restype = None
    lib.a1mpc_contact_terrain_batch.argtypes = [vp, C.POINTER(ContactConfig), i32, dp, u8p, dp, dp, dp, dp, u8p, dp, dp]
    lib.a1mpc_contact_terrain_batch.restype = C.c_int
    lib.a1mpc_reset_contact_state.argtypes = [vp]; lib.a1mpc_reset_contact_state.restype = C.c_int
    lib.a1mpc_swing_legs_batch.argtypes = [vp, i32, C.c_double, C.c_double, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp]
    lib.a1mpc_swing_legs_batch.restype = C.c_int
    lib.a1mpc_leg_state_batch.argtypes = [vp, i32] + [dp] * 14; lib.a1mpc_leg_state_batch.restype = C.c_int
    lib.a1mpc_ekf_update_batch.argtypes = [vp, i32, C.c_double, i32, u8p, dp, dp, dp, dp, dp, dp, dp, dp, u8p]; lib.a1mpc_ekf_update_batch.restype = C.c_int
    lib.a1mpc_reset_ekf_state.argtypes = [vp]; lib.a1mpc_reset_ekf_state.restype = C.c_int
    vpp = C.c_void_p
    lib.a1mpc_update_plan_batch_device.argtypes = [vp, C.POINTER(GaitConfig), i32] + [vpp] * 12 + [vpp]; lib.a1mpc_update_plan_batch_device.restype = C.c_int
    lib.a1mpc_swing_legs_batch_device.argtypes = [vp, i32, C.c_double, C.c_double] + [vpp] * 4 + [dp, dp] + [vpp] * 5 + [vpp]; lib.a1mpc_swing_legs_batch_device.restype = C.c_int
    lib.a1mpc_contact_terrain_batch_device.argtypes = [vp, C.POINTER(ContactConfig), i32] + [vpp] * 9 + [vpp]; lib.a1mpc_contact_terrain_batch_device.restype = C.c_int
    lib.a1mpc_leg_state_batch_device.argtypes = [vp, i32] + [vpp] * 5 + [dp, dp] + [vpp] * 7 + [vpp]; lib.a1mpc_leg_state_batch_device.restype = C.c_int
    lib.a1mpc_ekf_update_batch_device.argtypes = [vp, i32, C.c_double, i32] + [vpp] * 10 + [vpp]; lib.a1mpc_ekf_update_batch_device.restype = C.c_int
    lib.a1mpc_joint_torques_batch_device.argtypes = [vp, i32] + [vpp] * 5 + [dp] + [vpp] * 2 + [vpp]; lib.a1mpc_joint_torques_batch_device.restype = C.c_int
    lib.a1mpc_solve_batch_strided.argtypes = [vp, i32, dp, dp, dp, dp, i32, u8p, i32, dp, dp, dp, i32p, i32p]; lib.a1mpc_solve_batch_strided.restype = C.c_int
    lib.a1mpc_solve_batch_strided_device.argtypes = [vp, i32] + [vp] * 4 + [i32, vp, i32] + [vp] * 5 + [vp]; lib.a1mpc_solve_batch_strided_device.restype = C.c_int
    lib.a1mpc_sharded_create.argtypes = [C.POINTER(Config), i32, i32p, i32, i32, C.POINTER(vp)]; lib.a1mpc_sharded_create.restype = C.c_int
    lib.a1mpc_sharded_solve_batch.argtypes = [vp, i32, dp, dp, dp, dp, u8p, dp, i32p, i32p]; lib.a1mpc_sharded_solve_batch.restype = C.c_int
    lib.a1mpc_sharded_info.argtypes = [vp, i32p, i32p, i32p]; lib.a1mpc_sharded_info.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_sharded_solve_batch_ticks"):   # (round 6)
        lib.a1mpc_sharded_solve_batch_ticks.argtypes = [vp, i32, dp, dp, dp, u8p, dp, i32p, i32p]; lib.a1mpc_sharded_solve_batch_ticks.restype = C.c_int
        lib.a1mpc_sharded_solve_batch_device.argtypes = [vp, i32] + [vp] * 9; lib.a1mpc_sharded_solve_batch_device.restype = C.c_int
        lib.a1mpc_sharded_solve_batch_ticks_device.argtypes = [vp, i32] + [vp] * 8; lib.a1mpc_sharded_solve_batch_ticks_device.restype = C.c_int
        lib.a1mpc_sharded_handle.argtypes = [vp, i32, C.POINTER(vp)]; lib.a1mpc_sharded_handle.restype = C.c_int
        lib.a1mpc_sharded_last_transfer.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.a1mpc_sharded_last_transfer.restype = C.c_int
    lib.a1mpc_sharded_destroy.argtypes = [vp]; lib.a1mpc_sharded_destroy.restype = None
    lib.a1mpc_pipeline_create.argtypes = [C.POINTER(Config), i32, i32, i32, C.POINTER(vp)]; lib.a1mpc_pipeline_create.restype = C.c_int
    lib.a1mpc_pipeline_submit_device.argtypes = [vp, i32, i32, i32] + [vp] * 9 + [vp, i32p]; lib.a1mpc_pipeline_submit_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_pipeline_submit"):  # (an older build bound by hand for an A/B, tools/ab_probe.py, may lack the round-3 entries)
        lib.a1mpc_pipeline_submit.argtypes = [vp, i32, i32, i32, dp, dp, dp, dp, u8p, dp, dp, i32p, i32p, i32p]; lib.a1mpc_pipeline_submit.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_pipeline_submit_strided_device"):   # (round 6)
        lib.a1mpc_pipeline_submit_strided_device.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32p]; lib.a1mpc_pipeline_submit_strided_device.restype = C.c_int
        lib.a1mpc_pipeline_submit_strided.argtypes = [vp, i32, i32, i32, dp, dp, dp, dp, i32, u8p, i32, dp, dp, dp, i32p, i32p, i32p]; lib.a1mpc_pipeline_submit_strided.restype = C.c_int
        lib.a1mpc_pipeline_submit_ticks_device.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32p]; lib.a1mpc_pipeline_submit_ticks_device.restype = C.c_int
    lib.a1mpc_pipeline_wait.argtypes = [vp, i32]; lib.a1mpc_pipeline_wait.restype = C.c_int
    lib.a1mpc_pipeline_join.argtypes = [vp, i32, vp]; lib.a1mpc_pipeline_join.restype = C.c_int
    lib.a1mpc_pipeline_handle.argtypes = [vp, i32, C.POINTER(vp)]; lib.a1mpc_pipeline_handle.restype = C.c_int
    lib.a1mpc_pipeline_depth.argtypes = [vp, i32p]; lib.a1mpc_pipeline_depth.restype = C.c_int
    lib.a1mpc_pipeline_destroy.argtypes = [vp]; lib.a1mpc_pipeline_destroy.restype = None
    lib.a1mpc_terrain_batch.argtypes = [vp, i32, i32, dp, dp, dp, dp]; lib.a1mpc_terrain_batch.restype = C.c_int
    lib.a1mpc_form_qp_batch.argtypes = [vp, i32, dp, dp, dp, dp, i32, u8p, i32, dp, dp, dp, dp, dp]; lib.a1mpc_form_qp_batch.restype = C.c_int
    lib.a1mpc_update_config.argtypes = [vp, C.POINTER(Config)]; lib.a1mpc_update_config.restype = C.c_int
    lib.a1mpc_warm_start.argtypes = [vp, i32, dp, dp, dp]; lib.a1mpc_warm_start.restype = C.c_int
    lib.a1mpc_get_warm_start.argtypes = [vp, i32, dp, dp, dp]; lib.a1mpc_get_warm_start.restype = C.c_int
    lib.a1mpc_get_workspace_z.argtypes = [vp, i32, dp]; lib.a1mpc_get_workspace_z.restype = C.c_int
    lib.a1mpc_get_workspace_scaling.argtypes = [vp, i32, dp, dp, dp]; lib.a1mpc_get_workspace_scaling.restype = C.c_int
    lib.a1mpc_set_profiling.argtypes = [vp, i32]; lib.a1mpc_set_profiling.restype = C.c_int
    lib.a1mpc_last_stage_cycles.argtypes = [vp, dp, C.POINTER(C.c_int32)]; lib.a1mpc_last_stage_cycles.restype = C.c_int
    lib.a1mpc_last_warm_start_mode.argtypes = [vp, C.POINTER(C.c_int32)]; lib.a1mpc_last_warm_start_mode.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_set_timing"):   # (round 5)
        lib.a1mpc_set_timing.argtypes = [vp, i32]; lib.a1mpc_set_timing.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_control_tick_device"):   # (round 5)
        lib.a1mpc_default_tick_params.argtypes = [C.POINTER(TickParams)]; lib.a1mpc_default_tick_params.restype = None
        lib.a1mpc_control_tick_device.argtypes = [vp, C.POINTER(TickParams), C.POINTER(TickBuffers), i32, vp]; lib.a1mpc_control_tick_device.restype = C.c_int
        lib.a1mpc_last_control_tick_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]; lib.a1mpc_last_control_tick_ms.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_control_tick_preview_device"):   # (the gait-aware horizon; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_default_preview_config.argtypes = [C.POINTER(PreviewConfig)]; lib.a1mpc_default_preview_config.restype = None
        lib.a1mpc_horizon_preview_batch.argtypes = [vp, C.POINTER(PreviewConfig), C.POINTER(GaitConfig), i32, u8p, dp, dp, u8p, dp, dp, dp, u8p, dp]
        lib.a1mpc_horizon_preview_batch.restype = C.c_int
        lib.a1mpc_horizon_preview_batch_device.argtypes = [vp, C.POINTER(PreviewConfig), C.POINTER(GaitConfig), i32] + [vpp] * 9 + [vpp]
        lib.a1mpc_horizon_preview_batch_device.restype = C.c_int
        lib.a1mpc_solve_batch_ticks_strided.argtypes = [vp, i32, dp, dp, dp, i32, u8p, i32, dp, dp, dp, i32p, i32p]; lib.a1mpc_solve_batch_ticks_strided.restype = C.c_int
        lib.a1mpc_solve_batch_ticks_strided_device.argtypes = [vp, i32] + [vpp] * 3 + [i32, vpp, i32] + [vpp] * 5 + [vpp]; lib.a1mpc_solve_batch_ticks_strided_device.restype = C.c_int
        lib.a1mpc_control_tick_preview_device.argtypes = [vp, C.POINTER(TickParams), C.POINTER(PreviewConfig), C.POINTER(TickBuffers), i32, vp]
        lib.a1mpc_control_tick_preview_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_control_tick_preview_footholds_device"):   # (the foothold preview; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_horizon_preview_footholds_batch.argtypes = [vp, C.POINTER(PreviewConfig), C.POINTER(GaitConfig), i32, u8p, dp, dp, u8p, dp, dp, dp, dp, u8p, dp]
        lib.a1mpc_horizon_preview_footholds_batch.restype = C.c_int
        lib.a1mpc_horizon_preview_footholds_batch_device.argtypes = [vp, C.POINTER(PreviewConfig), C.POINTER(GaitConfig), i32] + [vpp] * 10 + [vpp]
        lib.a1mpc_horizon_preview_footholds_batch_device.restype = C.c_int
        lib.a1mpc_control_tick_preview_footholds_device.argtypes = [vp, C.POINTER(TickParams), C.POINTER(PreviewConfig), C.POINTER(TickBuffers), i32, vp]
        lib.a1mpc_control_tick_preview_footholds_device.restype = C.c_int
        lib.a1mpc_pipeline_submit_ticks_strided_device.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32p]
        lib.a1mpc_pipeline_submit_ticks_strided_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_horizon_states_batch"):   # (predicted horizon states and cost; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_horizon_states_batch.argtypes = [vp, i32, dp, dp, dp, dp, i32, dp, dp, dp, dp]; lib.a1mpc_horizon_states_batch.restype = C.c_int
        lib.a1mpc_horizon_states_batch_device.argtypes = [vp, i32] + [vpp] * 4 + [i32] + [vpp] * 4 + [vpp]; lib.a1mpc_horizon_states_batch_device.restype = C.c_int
        lib.a1mpc_horizon_states_ticks_batch.argtypes = [vp, i32, dp, dp, dp, i32, dp, dp, dp, dp]; lib.a1mpc_horizon_states_ticks_batch.restype = C.c_int
        lib.a1mpc_horizon_states_ticks_batch_device.argtypes = [vp, i32] + [vpp] * 3 + [i32] + [vpp] * 4 + [vpp]; lib.a1mpc_horizon_states_ticks_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_plant_step_batch"):   # (the single-rigid-body plant step; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_default_plant_config.argtypes = [C.POINTER(PlantConfig)]; lib.a1mpc_default_plant_config.restype = None
        lib.a1mpc_plant_step_batch.argtypes = [vp, C.POINTER(PlantConfig), i32, dp, i32, dp, dp, dp, u8p, dp, dp, dp, dp]; lib.a1mpc_plant_step_batch.restype = C.c_int
        lib.a1mpc_plant_step_batch_device.argtypes = [vp, C.POINTER(PlantConfig), i32, vpp, i32] + [vpp] * 8 + [vpp]; lib.a1mpc_plant_step_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_sensor_synthesis_batch"):   # (sensor synthesis from the plant; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_sensor_synthesis_batch.argtypes = [vp, i32, dp, i32, dp, dp, dp, u8p, dp, dp, dp] + [dp] * 6 + [u8p, dp, dp]; lib.a1mpc_sensor_synthesis_batch.restype = C.c_int
        lib.a1mpc_sensor_synthesis_batch_device.argtypes = [vp, i32, vpp, i32] + [vpp] * 5 + [dp, dp] + [vpp] * 9 + [vpp]; lib.a1mpc_sensor_synthesis_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_walk_step_batch"):   # (the walking plant and its sensors; an older build bound by hand for an A/B lacks them)
        lib.a1mpc_default_walk_config.argtypes = [C.POINTER(WalkConfig)]; lib.a1mpc_default_walk_config.restype = None
        lib.a1mpc_walk_step_batch.argtypes = [vp, C.POINTER(WalkConfig), i32, dp, i32, dp, dp, dp, u8p, dp, dp, dp, dp, dp, dp, dp]; lib.a1mpc_walk_step_batch.restype = C.c_int
        lib.a1mpc_walk_step_batch_device.argtypes = [vp, C.POINTER(WalkConfig), i32, vpp, i32] + [vpp] * 11 + [vpp]; lib.a1mpc_walk_step_batch_device.restype = C.c_int
        lib.a1mpc_walk_sensors_batch.argtypes = [vp, i32, dp, i32, dp, dp, dp, u8p, dp, dp, dp, dp] + [dp] * 6 + [u8p, dp, dp]; lib.a1mpc_walk_sensors_batch.restype = C.c_int
        lib.a1mpc_walk_sensors_batch_device.argtypes = [vp, i32, vpp, i32] + [vpp] * 6 + [dp, dp] + [vpp] * 9 + [vpp]; lib.a1mpc_walk_sensors_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_ground_step_batch"):   # (sloped ground and sensed touchdowns; an older build bound by hand for an A/B lacks them)
        lib.a1mpc_ground_step_batch.argtypes = [vp, C.POINTER(WalkConfig), i32, dp, i32, dp, dp, dp, u8p, dp, dp, dp, dp, dp, dp, dp, dp, u8p]
        lib.a1mpc_ground_step_batch.restype = C.c_int
        lib.a1mpc_ground_step_batch_device.argtypes = [vp, C.POINTER(WalkConfig), i32, vpp, i32] + [vpp] * 13 + [vpp]; lib.a1mpc_ground_step_batch_device.restype = C.c_int
        lib.a1mpc_touch_sensors_batch.argtypes = [vp, i32, dp, i32, dp, dp, dp, u8p, dp, dp, u8p, C.c_double, dp, dp] + [dp] * 6 + [u8p, dp, dp]
        lib.a1mpc_touch_sensors_batch.restype = C.c_int
        lib.a1mpc_touch_sensors_batch_device.argtypes = [vp, i32, vpp, i32] + [vpp] * 7 + [C.c_double, dp, dp] + [vpp] * 9 + [vpp]
        lib.a1mpc_touch_sensors_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_heightfield_step_batch"):   # (height-field terrain; an older build bound by hand for an A/B lacks it)
        hfp = C.POINTER(Heightfield)
        lib.a1mpc_default_heightfield.argtypes = [hfp]; lib.a1mpc_default_heightfield.restype = None
        lib.a1mpc_heightfield_step_batch.argtypes = [vp, C.POINTER(WalkConfig), i32, dp, i32, dp, dp, dp, u8p, dp, dp, dp, hfp, dp, dp, dp, dp, dp, u8p, dp]
        lib.a1mpc_heightfield_step_batch.restype = C.c_int
        lib.a1mpc_heightfield_step_batch_device.argtypes = [vp, C.POINTER(WalkConfig), i32, vpp, i32] + [vpp] * 7 + [hfp] + [vpp] * 7 + [vpp]
        lib.a1mpc_heightfield_step_batch_device.restype = C.c_int
        lib.a1mpc_heightfield_sample_batch.argtypes = [vp, hfp, i32, dp, dp, dp]; lib.a1mpc_heightfield_sample_batch.restype = C.c_int
        lib.a1mpc_heightfield_sample_batch_device.argtypes = [vp, hfp, i32, vpp, vpp, vpp, vpp]; lib.a1mpc_heightfield_sample_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_sensor_noise_batch"):   # (sensor noise and IMU bias; an older build bound by hand for an A/B lacks them)
        u64 = C.c_uint64
        lib.a1mpc_default_noise_config.argtypes = [C.POINTER(NoiseConfig)]; lib.a1mpc_default_noise_config.restype = None
        lib.a1mpc_sensor_noise_batch.argtypes = [vp, C.POINTER(NoiseConfig), i32, u64, u64] + [dp] * 8; lib.a1mpc_sensor_noise_batch.restype = C.c_int
        lib.a1mpc_sensor_noise_batch_device.argtypes = [vp, C.POINTER(NoiseConfig), i32, u64, u64] + [vpp] * 8 + [vpp]; lib.a1mpc_sensor_noise_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_episode_update_batch"):   # (episode record and batch summary; an older build bound by hand for an A/B lacks them)
        u64 = C.c_uint64; u8p = C.POINTER(C.c_uint8); i32p = C.POINTER(C.c_int32)
        lib.a1mpc_default_episode_config.argtypes = [C.POINTER(EpisodeConfig)]; lib.a1mpc_default_episode_config.restype = None
        lib.a1mpc_episode_update_batch.argtypes = [vp, C.POINTER(EpisodeConfig), i32, u64, dp, i32] + [dp] * 7 + [u8p, i32p, u8p, dp]
        lib.a1mpc_episode_update_batch.restype = C.c_int
        lib.a1mpc_episode_update_batch_device.argtypes = [vp, C.POINTER(EpisodeConfig), i32, u64, vpp, i32] + [vpp] * 11 + [vpp]
        lib.a1mpc_episode_update_batch_device.restype = C.c_int
        lib.a1mpc_episode_summary_batch.argtypes = [vp, i32, dp, dp]; lib.a1mpc_episode_summary_batch.restype = C.c_int
        lib.a1mpc_episode_summary_batch_device.argtypes = [vp, i32, vpp, vpp, vpp]; lib.a1mpc_episode_summary_batch_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_respawn_batch"):   # (respawn; an older build bound by hand for an A/B lacks it)
        u32 = C.c_uint32; u8p = C.POINTER(C.c_uint8); i32p = C.POINTER(C.c_int32)
        lib.a1mpc_default_respawn_config.argtypes = [C.POINTER(RespawnConfig)]; lib.a1mpc_default_respawn_config.restype = None
        lib.a1mpc_respawn_reset_batch.argtypes = [vp, i32, u8p, u32]; lib.a1mpc_respawn_reset_batch.restype = C.c_int
        lib.a1mpc_respawn_reset_batch_device.argtypes = [vp, i32, vpp, u32, vpp]; lib.a1mpc_respawn_reset_batch_device.restype = C.c_int
        lib.a1mpc_respawn_batch.argtypes = [vp, C.POINTER(RespawnConfig), i32, dp, i32p, dp, u8p]; lib.a1mpc_respawn_batch.restype = C.c_int
        lib.a1mpc_respawn_batch_device.argtypes = [vp, C.POINTER(RespawnConfig), i32, vpp, vpp, vpp, vpp, vpp]; lib.a1mpc_respawn_batch_device.restype = C.c_int
        lib.a1mpc_respawn_rows_device.argtypes = [vp, i32, vpp, C.POINTER(RespawnRows), i32, vpp]; lib.a1mpc_respawn_rows_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_control_tick_balance_device"):   # (the balance-QP controller on the device; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_default_balance_gains.argtypes = [C.POINTER(BalanceGains)]; lib.a1mpc_default_balance_gains.restype = None
        lib.a1mpc_balance_wrench_batch.argtypes = [vp, C.POINTER(BalanceGains), i32] + [dp] * 10; lib.a1mpc_balance_wrench_batch.restype = C.c_int
        lib.a1mpc_balance_wrench_batch_device.argtypes = [vp, C.POINTER(BalanceGains), i32] + [vpp] * 10 + [vpp]; lib.a1mpc_balance_wrench_batch_device.restype = C.c_int
        lib.a1mpc_balance_solve_batch_device.argtypes = [vp, C.POINTER(BalanceConfig), i32] + [vpp] * 9 + [vpp]; lib.a1mpc_balance_solve_batch_device.restype = C.c_int
        lib.a1mpc_contacts_batch.argtypes = [vp, C.POINTER(ContactConfig), i32, dp, u8p, dp, dp, u8p, dp]; lib.a1mpc_contacts_batch.restype = C.c_int
        lib.a1mpc_contacts_batch_device.argtypes = [vp, C.POINTER(ContactConfig), i32] + [vpp] * 6 + [vpp]; lib.a1mpc_contacts_batch_device.restype = C.c_int
        lib.a1mpc_control_tick_balance_device.argtypes = [vp, C.POINTER(TickParams), C.POINTER(BalanceTick), C.POINTER(TickBuffers), i32, vp]
        lib.a1mpc_control_tick_balance_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_control_tick_sensors_device"):   # (the sensor / command front end; an older build bound by hand for an A/B lacks it)
        lib.a1mpc_balance_wrench_kp_batch.argtypes = [vp, C.POINTER(BalanceGains), i32] + [dp] * 11; lib.a1mpc_balance_wrench_kp_batch.restype = C.c_int
        lib.a1mpc_balance_wrench_kp_batch_device.argtypes = [vp, C.POINTER(BalanceGains), i32] + [vpp] * 11 + [vpp]; lib.a1mpc_balance_wrench_kp_batch_device.restype = C.c_int
        lib.a1mpc_default_sensor_config.argtypes = [C.POINTER(SensorConfig)]; lib.a1mpc_default_sensor_config.restype = None
        lib.a1mpc_default_command_config.argtypes = [C.POINTER(CommandConfig)]; lib.a1mpc_default_command_config.restype = None
        lib.a1mpc_reset_sensor_state.argtypes = [vp]; lib.a1mpc_reset_sensor_state.restype = C.c_int
        lib.a1mpc_sensor_frontend_batch.argtypes = [vp, C.POINTER(SensorConfig), i32] + [dp] * 9; lib.a1mpc_sensor_frontend_batch.restype = C.c_int
        lib.a1mpc_sensor_frontend_batch_device.argtypes = [vp, C.POINTER(SensorConfig), i32] + [vpp] * 9 + [vpp]; lib.a1mpc_sensor_frontend_batch_device.restype = C.c_int
        lib.a1mpc_command_batch.argtypes = [vp, C.POINTER(CommandConfig), i32, dp, u8p, dp, C.c_double, dp, u8p, dp, dp, dp, i32p, dp, dp, u8p, u8p, dp]
        lib.a1mpc_command_batch.restype = C.c_int
        lib.a1mpc_command_batch_device.argtypes = [vp, C.POINTER(CommandConfig), i32, vpp, vpp, vpp, C.c_double] + [vpp] * 11 + [vpp]; lib.a1mpc_command_batch_device.restype = C.c_int
        lib.a1mpc_control_tick_sensors_device.argtypes = [vp, C.POINTER(TickParams), C.POINTER(TickSensors), C.POINTER(TickBuffers), i32, vpp]
        lib.a1mpc_control_tick_sensors_device.restype = C.c_int
    if path == _build.LIB_PATH or hasattr(lib, "a1mpc_last_tick_stage_cycles"):  # (round 5; an older build bound by hand for an A/B may lack it)
        lib.a1mpc_last_tick_stage_cycles.argtypes = [vp, dp, C.POINTER(C.c_int32)]; lib.a1mpc_last_tick_stage_cycles.restype = C.c_int
    lib.a1mpc_set_schedule.argtypes = [vp, i32]; lib.a1mpc_set_schedule.restype = C.c_int
    lib.a1mpc_reset_warm_start.argtypes = [vp]; lib.a1mpc_reset_warm_start.restype = C.c_int
    lib.a1mpc_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]; lib.a1mpc_last_kernel_ms.restype = C.c_int
    lib.a1mpc_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]; lib.a1mpc_last_stage_ms.restype = C.c_int
    lib.a1mpc_last_nfact.argtypes = [vp, i32, i32p]; lib.a1mpc_last_nfact.restype = C.c_int
    lib.a1mpc_kernel_info.argtypes = [vp, i32p, i32p, i32p]; lib.a1mpc_kernel_info.restype = C.c_int
    lib.a1mpc_status_string.argtypes = [C.c_int]; lib.a1mpc_status_string.restype = C.c_char_p
    lib.a1mpc_last_error.argtypes = []; lib.a1mpc_last_error.restype = C.c_char_p
    if path == _build.LIB_PATH:
        _lib = lib
    return lib


def _check(lib, rc, what):
    if rc != 0:
        raise A1MpcError(f"{what}: {lib.a1mpc_status_string(rc).decode()} ({lib.a1mpc_last_error().decode()})")


def make_config(params, horizon, **osqp):
    """params: dict with dt, mu, fz_min, fz_max, q(13), r(12), mass, inertia(9) -- e.g. scenarios.*()['params'].
    osqp: overrides of the OSQP settings fields (rho, eps_abs, eps_rel, max_iter, warm_start, ...)."""
    lib = load_library()
    cfg = Config()
    lib.a1mpc_default_config(C.byref(cfg))
    cfg.horizon = int(horizon)
    cfg.dt, cfg.mu, cfg.fz_min, cfg.fz_max, cfg.mass = params["dt"], params["mu"], params["fz_min"], params["fz_max"], params["mass"]
    cfg.q[:] = [float(v) for v in params["q"]]
    cfg.r[:] = [float(v) for v in params["r"]]
    cfg.inertia_body[:] = [float(v) for v in np.asarray(params["inertia"], dtype=float).reshape(9)]
    for k, v in osqp.items():
        if not hasattr(cfg, k):
            raise KeyError(k)
        setattr(cfg, k, v)
    return cfg


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _u8p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _dev(t):
    """a device pointer: a torch tensor, an integer address, or None"""
    return None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(shape)


class HeightfieldOnDevice:
    """What Engine.heightfield returns: heights (ny, nx) on the engine's device with the a1mpc_heightfield that points at them.  .struct is what the _device entries
    take, .host the same descriptor over the host copy for the host-pointer entries; .tensor and .heights keep both alive as long as the object lives"""

    def __init__(self, engine, heights, x0=0.0, y0=0.0, dx=1.0, dy=1.0, interp=0):
        import torch
        h = np.ascontiguousarray(heights, dtype=np.float64)
        if h.ndim != 2:
            raise ValueError("heights must be (ny, nx)")
        self.heights = h
        self.ny, self.nx = h.shape
        self.tensor = torch.from_numpy(h if h.flags.writeable else h.copy()).to(f"cuda:{engine.device}")   # (torch does not take a read-only array)
        self.struct, self.host = Heightfield(), Heightfield()
        for s, ptr in ((self.struct, self.tensor.data_ptr()), (self.host, h.ctypes.data)):
            engine.lib.a1mpc_default_heightfield(C.byref(s))
            s.nx, s.ny, s.x0, s.y0, s.dx, s.dy, s.interp, s.height = self.nx, self.ny, float(x0), float(y0), float(dx), float(dy), int(interp), ptr


class Engine:
    """One a1mpc handle: a fixed (robot constants, horizon, OSQP settings) configuration on one GPU."""

    def __init__(self, cfg, max_batch, device=0):
        self.lib = load_library()
        self.cfg = cfg
        self.horizon = int(cfg.horizon)
        self.max_batch = int(max_batch)
        self.device = int(device)
        self._h = C.c_void_p()
        _check(self.lib, self.lib.a1mpc_create(C.byref(cfg), self.max_batch, self.device, C.byref(self._h)), "a1mpc_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.a1mpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- host arrays (the drop-in path: S/A1RobotControl.cpp:446-562 for n ticks) ----
    def solve(self, x0, xref, R, foot, contact, want_u=False):
        h = self.horizon
        x0 = _f64(x0, (-1, NS)); n = x0.shape[0]
        xref = _f64(xref, (n, NS * h)); R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12))
        contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4)
        grf = np.zeros((n, 12)); u = np.zeros((n, NU * h)) if want_u else None
        iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_solve_batch(self._h, n, _dp(x0), _dp(xref), _dp(R), _dp(foot),
                                        contact.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(grf), _dp(u), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_solve_batch")
        return dict(grf=grf, u=u, iters=iters, status=status)

    # ---- the general case of the ConvexMpc interface: per-step feet (B_mat_d_list) and / or a per-step contact schedule ----
    def solve_strided(self, x0, xref, R, foot, foot_stride, contact, contact_stride, want_u=False, yaw_A=None):
        h = self.horizon
        x0 = _f64(x0, (-1, NS)); n = x0.shape[0]
        xref = _f64(xref, (n, NS * h)); R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12 * h if foot_stride else 12))
        contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4 * h if contact_stride else 4)
        grf = np.zeros((n, 12)); u = np.zeros((n, NU * h)) if want_u else None
        iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_solve_batch_strided(self._h, n, _dp(x0), _dp(xref), _dp(R), _dp(foot), int(foot_stride),
                                                contact.ctypes.data_as(C.POINTER(C.c_uint8)), int(contact_stride),
                                                None if yaw_A is None else _dp(np.ascontiguousarray(yaw_A, dtype=np.float64)), _dp(grf), _dp(u), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_solve_batch_strided")
        return dict(grf=grf, u=u, iters=iters, status=status)

    def form_qp(self, x0, xref, R, foot, contact, foot_stride=0, contact_stride=0, yaw_A=None):
        """the dense (P, g, l, u) the reference's ConvexMpc members hold, formed on the GPU (debug / verification)"""
        h = self.horizon
        x0 = _f64(x0, (-1, NS)); n = x0.shape[0]
        xref = _f64(xref, (n, NS * h)); R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12 * h if foot_stride else 12))
        contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4 * h if contact_stride else 4)
        P = np.zeros((n, 12 * h, 12 * h)); g = np.zeros((n, 12 * h)); l = np.zeros((n, 20 * h)); u = np.zeros((n, 20 * h))
        rc = self.lib.a1mpc_form_qp_batch(self._h, n, _dp(x0), _dp(xref), _dp(R), _dp(foot), int(foot_stride), contact.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          int(contact_stride), None if yaw_A is None else _dp(np.ascontiguousarray(yaw_A, dtype=np.float64)), _dp(P), _dp(g), _dp(l), _dp(u))
        _check(self.lib, rc, "a1mpc_form_qp_batch")
        return dict(P=P, g=g, l=l, u=u)

    def terrain(self, foot_pos_recent_contact, root_pos_z, root_euler_d_pitch, use_terrain_adapt=1):
        rec = _f64(foot_pos_recent_contact, (-1, 12)); n = rec.shape[0]
        z = _f64(root_pos_z, (n,)); pd = _f64(root_euler_d_pitch, (n,)).copy(); ta = np.zeros(n)
        _check(self.lib, self.lib.a1mpc_terrain_batch(self._h, int(use_terrain_adapt), n, _dp(rec), _dp(z), _dp(pd), _dp(ta)), "a1mpc_terrain_batch")
        return pd, ta

    def update_config(self, cfg):
        """replace everything but the horizon (dt, weights, mass / inertia, limits, OSQP settings); the warm start is kept"""
        _check(self.lib, self.lib.a1mpc_update_config(self._h, C.byref(cfg)), "a1mpc_update_config")
        self.cfg = cfg

    def set_warm_start(self, x=None, y=None, rho=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, rho)]
        n = next(a for a in arrs if a is not None).shape[0]
        _check(self.lib, self.lib.a1mpc_warm_start(self._h, n, _dp(arrs[0]), _dp(arrs[1]), _dp(arrs[2])), "a1mpc_warm_start")

    def get_warm_start(self, n):
        h = self.horizon
        x = np.zeros((n, NU * h)); y = np.zeros((n, 20 * h)); rho = np.zeros(n)
        _check(self.lib, self.lib.a1mpc_get_warm_start(self._h, int(n), _dp(x), _dp(y), _dp(rho)), "a1mpc_get_warm_start")
        return x, y, rho

    def set_timing(self, on=True):
        """a1mpc_set_timing: the handle's HIP timing events on / off (off: last_kernel_ms & co. are unavailable, every tick is a few event records lighter)"""
        _check(self.lib, self.lib.a1mpc_set_timing(self._h, 1 if on else 0), "a1mpc_set_timing")

    def set_profiling(self, on=True):
        _check(self.lib, self.lib.a1mpc_set_profiling(self._h, 1 if on else 0), "a1mpc_set_profiling")

    def last_stage_cycles(self):
        """dict(factor, iterate, check: shader-clock cycles summed over the QPs of the last profiled solve; qps) -- a1mpc_last_stage_cycles"""
        c = np.zeros(3); q = C.c_int32(0)
        _check(self.lib, self.lib.a1mpc_last_stage_cycles(self._h, _dp(c), C.byref(q)), "a1mpc_last_stage_cycles")
        return dict(factor=float(c[0]), iterate=float(c[1]), check=float(c[2]), qps=int(q.value))

    def control_tick_device(self, params, buffers, n, stream=None):
        """a1mpc_control_tick_device: one whole control tick of n robots (device pointers in a TickBuffers), asynchronous on `stream`"""
        _check(self.lib, self.lib.a1mpc_control_tick_device(self._h, C.byref(params), C.byref(buffers), int(n), C.c_void_p(stream) if stream else None), "a1mpc_control_tick_device")

    def control_tick_preview_device(self, params, preview, buffers, n, stream=None):
        """a1mpc_control_tick_preview_device: the control tick with the gait-aware horizon (a PreviewConfig) between the contacts stage and the MPC launch"""
        _check(self.lib, self.lib.a1mpc_control_tick_preview_device(self._h, C.byref(params), C.byref(preview), C.byref(buffers), int(n), C.c_void_p(stream) if stream else None),
               "a1mpc_control_tick_preview_device")

    def control_tick_preview_footholds_device(self, params, preview, buffers, n, stream=None):
        """a1mpc_control_tick_preview_footholds_device: control_tick_preview_device in which a leg that lands inside the horizon stands at buffers.foot_pos_target_abs"""
        _check(self.lib, self.lib.a1mpc_control_tick_preview_footholds_device(self._h, C.byref(params), C.byref(preview), C.byref(buffers), int(n),
                                                                              C.c_void_p(stream) if stream else None), "a1mpc_control_tick_preview_footholds_device")

    def preview_config(self, **fields):
        """a1mpc_default_preview_config ({1, 0, 1}) with `fields` (contact_schedule, foot_preview, ticks_per_step) overridden"""
        pv = PreviewConfig(); self.lib.a1mpc_default_preview_config(C.byref(pv))
        for k, v in fields.items():
            if not hasattr(pv, k):
                raise KeyError(k)
            setattr(pv, k, int(v))
        return pv

    # ---- the gait-aware horizon: contact schedule (update_plan's counter rule run forward) and per-step feet, the inputs of solve_strided / solve_ticks_strided ----
    def horizon_preview(self, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs=None, R=None, root_lin_vel_d=None, preview=None, gait=None,
                        want_schedule=True, foot_target_abs=None):
        """dict(contact_sched (n, 4 H) uint8 or None, foot_steps (n, 12 H) or None): a1mpc_horizon_preview_batch.  The feet are produced when preview.foot_preview is 1 or 2.
        foot_target_abs (n, 12: update_plan's foot_pos_target_abs) selects a1mpc_horizon_preview_footholds_batch: a leg that lands inside the horizon stands at its target."""
        if gait is None:
            gait = GaitConfig(); self.lib.a1mpc_default_gait_config(C.byref(gait))
        pv = self.preview_config() if preview is None else preview
        h = self.horizon
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(-1, 4); n = ct.shape[0]
        mm = np.ascontiguousarray(movement_mode, dtype=np.uint8).reshape(n)
        gc = _f64(gait_counter, (n, 4)); spd = _f64(gait_counter_speed, (n, 4))
        fp = None if foot_pos_abs is None else _f64(foot_pos_abs, (n, 12)); Rw = None if R is None else _f64(R, (n, 9)); vd = None if root_lin_vel_d is None else _f64(root_lin_vel_d, (n, 3))
        sched = np.zeros((n, 4 * h), np.uint8) if want_schedule else None
        feet = np.zeros((n, 12 * h)) if pv.foot_preview != 0 else None
        if foot_target_abs is not None:
            tg = _f64(foot_target_abs, (n, 12))
            rc = self.lib.a1mpc_horizon_preview_footholds_batch(self._h, C.byref(pv), C.byref(gait), n, _u8p(mm), _dp(gc), _dp(spd), _u8p(ct), _dp(fp), _dp(Rw), _dp(vd), _dp(tg),
                                                                _u8p(sched), _dp(feet))
            _check(self.lib, rc, "a1mpc_horizon_preview_footholds_batch")
            return dict(contact_sched=sched, foot_steps=feet)
        rc = self.lib.a1mpc_horizon_preview_batch(self._h, C.byref(pv), C.byref(gait), n, _u8p(mm), _dp(gc), _dp(spd), _u8p(ct), _dp(fp), _dp(Rw), _dp(vd), _u8p(sched), _dp(feet))
        _check(self.lib, rc, "a1mpc_horizon_preview_batch")
        return dict(contact_sched=sched, foot_steps=feet)

    # ---- N1 + the general interface: tick records with per-step feet / a contact schedule / an A_c yaw of its own ----
    def solve_ticks_strided(self, tick, R, foot, foot_stride, contact, contact_stride, want_u=False, yaw_A=None):
        h = self.horizon
        tick = _f64(tick, (-1, 22)); n = tick.shape[0]
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12 * h if foot_stride else 12))
        contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4 * h if contact_stride else 4)
        grf = np.zeros((n, 12)); u = np.zeros((n, NU * h)) if want_u else None
        iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_solve_batch_ticks_strided(self._h, n, _dp(tick), _dp(R), _dp(foot), int(foot_stride), _u8p(contact), int(contact_stride),
                                                      None if yaw_A is None else _dp(np.ascontiguousarray(yaw_A, dtype=np.float64)), _dp(grf), _dp(u), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_solve_batch_ticks_strided")
        return dict(grf=grf, u=u, iters=iters, status=status)

    # ---- what the model does with a force plan: predicted states over the horizon (A_qp x0 + B_qp u of the reference's ConvexMpc members) and the plan's cost ----
    def horizon_states(self, x0, R, foot, u=None, xref=None, foot_stride=0, yaw_A=None):
        """dict(x_pred (n, H, 13): x_(t+1) at step t; cost (n, 2): [tracking, effort], or None without xref): a1mpc_horizon_states_batch.  u (n, 12 H) world-frame
        forces (u_full of a solve), None = zero forces: the free response"""
        h = self.horizon
        x0 = _f64(x0, (-1, NS)); n = x0.shape[0]
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12 * h if foot_stride else 12))
        u = None if u is None else _f64(u, (n, NU * h)); xref = None if xref is None else _f64(xref, (n, NS * h))
        x_pred = np.zeros((n, h, NS)); cost = None if xref is None else np.zeros((n, 2))
        rc = self.lib.a1mpc_horizon_states_batch(self._h, n, _dp(x0), _dp(xref), _dp(R), _dp(foot), int(foot_stride),
                                                 None if yaw_A is None else _dp(np.ascontiguousarray(yaw_A, dtype=np.float64)), _dp(u), _dp(x_pred), _dp(cost))
        _check(self.lib, rc, "a1mpc_horizon_states_batch")
        return dict(x_pred=x_pred, cost=cost)

    def horizon_states_ticks(self, tick, R, foot, u=None, foot_stride=0, yaw_A=None, want_cost=True):
        """the same from the compact tick records (x0 / x_ref built on the device as the ticks solve builds them): a1mpc_horizon_states_ticks_batch"""
        h = self.horizon
        tick = _f64(tick, (-1, 22)); n = tick.shape[0]
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12 * h if foot_stride else 12))
        u = None if u is None else _f64(u, (n, NU * h))
        x_pred = np.zeros((n, h, NS)); cost = np.zeros((n, 2)) if want_cost else None
        rc = self.lib.a1mpc_horizon_states_ticks_batch(self._h, n, _dp(tick), _dp(R), _dp(foot), int(foot_stride),
                                                       None if yaw_A is None else _dp(np.ascontiguousarray(yaw_A, dtype=np.float64)), _dp(u), _dp(x_pred), _dp(cost))
        _check(self.lib, rc, "a1mpc_horizon_states_ticks_batch")
        return dict(x_pred=x_pred, cost=cost)

    def horizon_states_device(self, n, d_x0, d_xref, d_R, d_foot, foot_stride, d_u, d_x_pred=None, d_cost=None, d_yaw_A=None, stream=None):
        """device pointers (torch tensors), asynchronous on `stream`: on the stream of the preceding solve_device it reads that solve's d_u"""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_horizon_states_batch_device(self._h, int(n), ptr(d_x0), ptr(d_xref), ptr(d_R), ptr(d_foot), int(foot_stride), ptr(d_yaw_A), ptr(d_u),
                                                        ptr(d_x_pred), ptr(d_cost), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_horizon_states_batch_device")

    def horizon_states_ticks_device(self, n, d_tick, d_R, d_foot, foot_stride, d_u, d_x_pred=None, d_cost=None, d_yaw_A=None, stream=None):
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_horizon_states_ticks_batch_device(self._h, int(n), ptr(d_tick), ptr(d_R), ptr(d_foot), int(foot_stride), ptr(d_yaw_A), ptr(d_u),
                                                              ptr(d_x_pred), ptr(d_cost), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_horizon_states_ticks_batch_device")

    # ---- what a robot does with the solved forces: one control period of the nonlinear single rigid body (the plant that closes the loop on the device) ----
    def plant_config(self, **fields):
        """a1mpc_default_plant_config ({0.0025, 1, -9.8}) with `fields` (dt, substeps, gravity_z) overridden"""
        pc = PlantConfig(); self.lib.a1mpc_default_plant_config(C.byref(pc))
        for k, v in fields.items():
            if not hasattr(pc, k):
                raise KeyError(k)
            setattr(pc, k, int(v) if k == "substeps" else float(v))
        return pc

    def plant_step(self, state, R, foot, grf, contacts, ext_wrench=None, plant=None):
        """dict(state (n, stride): [euler, pos, omega, v] stepped, words [12:stride) as they came; R (n, 9); foot (n, 12)): a1mpc_plant_step_batch.  state (n, 12 | 13 | 22)
        rows of [euler (not read), pos, omega (world), v], R body -> world, foot = foot_pos_abs, grf = the BODY-frame grf of a solve, ext_wrench (n, 6) world frame or None"""
        pc = self.plant_config() if plant is None else plant
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6))
        state_out = state.copy(); R_out = np.zeros((n, 9)); foot_out = np.zeros((n, 12))
        rc = self.lib.a1mpc_plant_step_batch(self._h, C.byref(pc), n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(state_out), _dp(R_out),
                                             _dp(foot_out))
        _check(self.lib, rc, "a1mpc_plant_step_batch")
        return dict(state=state_out, R=R_out, foot=foot_out)

    def plant_step_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_ext_wrench=None, d_state_out=None, d_R_out=None, d_foot_out=None, plant=None,
                          stream=None):
        """device pointers (torch tensors), asynchronous on `stream`: on the stream of the preceding solve_*_device it reads that solve's d_grf.  An output left None is
        its input: the step runs in place"""
        pc = self.plant_config() if plant is None else plant
        out = lambda o, i: _dev(i if o is None else o)
        rc = self.lib.a1mpc_plant_step_batch_device(self._h, C.byref(pc), int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf), _dev(d_contacts),
                                                    _dev(d_ext_wrench), out(d_state_out, d_state), out(d_R_out, d_R), out(d_foot_out, d_foot),
                                                    C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_plant_step_batch_device")

    # ---- what the robot's sensors read on that plant: the inverse of the tick's front stages, so that sensors -> tick -> plant -> sensors closes on the device ----
    SYNTHESIS_OUTPUTS = ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force", "reach", "foot_pos_rel", "foot_vel_rel")

    def sensor_synthesis(self, state, R, foot, grf, contacts, ext_wrench=None, rho_fix=None, rho_opt=None, want_foot_rel=True):
        """dict(quat (n, 4) as w, x, y, z; imu_acc_raw, imu_gyro_raw (n, 3); joint_pos, joint_vel (n, 12); foot_force (n, 4); reach (n, 4) uint8; foot_pos_rel, foot_vel_rel
        (n, 12), or None without want_foot_rel): a1mpc_sensor_synthesis_batch.  The inputs of plant_step (state (n, 12 | 13 | 22), of which omega and v are read) and the
        leg geometry of leg_state"""
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6))
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        out = dict(quat=np.zeros((n, 4)), imu_acc_raw=np.zeros((n, 3)), imu_gyro_raw=np.zeros((n, 3)), joint_pos=np.zeros((n, 12)), joint_vel=np.zeros((n, 12)),
                   foot_force=np.zeros((n, 4)), reach=np.zeros((n, 4), np.uint8), foot_pos_rel=np.zeros((n, 12)) if want_foot_rel else None,
                   foot_vel_rel=np.zeros((n, 12)) if want_foot_rel else None)
        rc = self.lib.a1mpc_sensor_synthesis_batch(self._h, n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(fix), _dp(opt), _dp(out["quat"]),
                                                   _dp(out["imu_acc_raw"]), _dp(out["imu_gyro_raw"]), _dp(out["joint_pos"]), _dp(out["joint_vel"]), _dp(out["foot_force"]),
                                                   _u8p(out["reach"]), _dp(out["foot_pos_rel"]), _dp(out["foot_vel_rel"]))
        _check(self.lib, rc, "a1mpc_sensor_synthesis_batch")
        return out

    def sensor_synthesis_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_joint_pos, d_joint_vel, d_foot_force,
                                d_reach, d_foot_pos_rel=None, d_foot_vel_rel=None, d_ext_wrench=None, rho_fix=None, rho_opt=None, stream=None):
        """device pointers (torch tensors), asynchronous on `stream`: on the stream of the preceding plant_step_device it reads that step's outputs; rho_fix / rho_opt are
        host arrays"""
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        rc = self.lib.a1mpc_sensor_synthesis_batch_device(self._h, int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf), _dev(d_contacts),
                                                          _dev(d_ext_wrench), _dp(fix), _dp(opt), _dev(d_quat), _dev(d_imu_acc_raw), _dev(d_imu_gyro_raw), _dev(d_joint_pos),
                                                          _dev(d_joint_vel), _dev(d_foot_force), _dev(d_reach), _dev(d_foot_pos_rel), _dev(d_foot_vel_rel),
                                                          C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_sensor_synthesis_batch_device")

    # ---- the walking plant: swing feet that move to the tick's swing target, a flat ground, and the sensors that know the swing feet move ----
    def walk_config(self, **fields):
        """a1mpc_default_walk_config (the default plant config, swing_track 1, flat_ground 0, ground_z 0) with `fields` overridden: dt, substeps, gravity_z (the plant's),
        swing_track, flat_ground, ground_z"""
        wc = WalkConfig(); self.lib.a1mpc_default_walk_config(C.byref(wc))
        for k, v in fields.items():
            tgt = wc.plant if hasattr(wc.plant, k) else wc
            if not hasattr(tgt, k):
                raise KeyError(k)
            setattr(tgt, k, int(v) if k in ("substeps", "flat_ground") else float(v))
        return wc

    def walk_step(self, state, R, foot, grf, contacts, R_z=None, foot_target=None, ext_wrench=None, walk=None):
        """dict(state, R, foot as plant_step; foot_vel_body (n, 12): the commanded body-frame velocity of the swing feet): a1mpc_walk_step_batch.  The inputs of plant_step,
        R_z (n, 9) the tick's root_rot_mat_z and foot_target (n, 12) its foot_pos_target_last_time (both may be None with swing_track == 0)"""
        wc = self.walk_config() if walk is None else walk
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6))
        Rz = None if R_z is None else _f64(R_z, (n, 9)); tg = None if foot_target is None else _f64(foot_target, (n, 12))
        state_out = state.copy(); R_out = np.zeros((n, 9)); foot_out = np.zeros((n, 12)); vel_out = np.zeros((n, 12))
        rc = self.lib.a1mpc_walk_step_batch(self._h, C.byref(wc), n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(Rz), _dp(tg), _dp(state_out),
                                            _dp(R_out), _dp(foot_out), _dp(vel_out))
        _check(self.lib, rc, "a1mpc_walk_step_batch")
        return dict(state=state_out, R=R_out, foot=foot_out, foot_vel_body=vel_out)

    def walk_step_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_R_z, d_foot_target, d_foot_vel_body, d_ext_wrench=None, d_state_out=None,
                         d_R_out=None, d_foot_out=None, walk=None, stream=None):
        """device pointers (torch tensors), asynchronous on `stream`: on the stream of the preceding control_tick_*_device it reads that tick's grf, contacts, R_z and
        foot_pos_target_last_time.  An output left None is its input: the step runs in place; d_foot_vel_body is written"""
        wc = self.walk_config() if walk is None else walk
        out = lambda o, i: _dev(i if o is None else o)
        rc = self.lib.a1mpc_walk_step_batch_device(self._h, C.byref(wc), int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf), _dev(d_contacts),
                                                   _dev(d_ext_wrench), _dev(d_R_z), _dev(d_foot_target), out(d_state_out, d_state), out(d_R_out, d_R), out(d_foot_out, d_foot),
                                                   _dev(d_foot_vel_body), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_walk_step_batch_device")

    def walk_sensors(self, state, R, foot, grf, contacts, foot_vel_body=None, ext_wrench=None, rho_fix=None, rho_opt=None, want_foot_rel=True):
        """the dict of sensor_synthesis: a1mpc_walk_sensors_batch.  foot_vel_body (n, 12) or None: the walk step's commanded swing-foot velocity"""
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6)); vel = None if foot_vel_body is None else _f64(foot_vel_body, (n, 12))
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        out = dict(quat=np.zeros((n, 4)), imu_acc_raw=np.zeros((n, 3)), imu_gyro_raw=np.zeros((n, 3)), joint_pos=np.zeros((n, 12)), joint_vel=np.zeros((n, 12)),
                   foot_force=np.zeros((n, 4)), reach=np.zeros((n, 4), np.uint8), foot_pos_rel=np.zeros((n, 12)) if want_foot_rel else None,
                   foot_vel_rel=np.zeros((n, 12)) if want_foot_rel else None)
        rc = self.lib.a1mpc_walk_sensors_batch(self._h, n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(vel), _dp(fix), _dp(opt), _dp(out["quat"]),
                                               _dp(out["imu_acc_raw"]), _dp(out["imu_gyro_raw"]), _dp(out["joint_pos"]), _dp(out["joint_vel"]), _dp(out["foot_force"]),
                                               _u8p(out["reach"]), _dp(out["foot_pos_rel"]), _dp(out["foot_vel_rel"]))
        _check(self.lib, rc, "a1mpc_walk_sensors_batch")
        return out

    def walk_sensors_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_joint_pos, d_joint_vel, d_foot_force,
                            d_reach, d_foot_pos_rel=None, d_foot_vel_rel=None, d_ext_wrench=None, d_foot_vel_body=None, rho_fix=None, rho_opt=None, stream=None):
        """sensor_synthesis_device with d_foot_vel_body: on the stream of the preceding walk_step_device it reads that step's outputs"""
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        rc = self.lib.a1mpc_walk_sensors_batch_device(self._h, int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf), _dev(d_contacts),
                                                      _dev(d_ext_wrench), _dev(d_foot_vel_body), _dp(fix), _dp(opt), _dev(d_quat), _dev(d_imu_acc_raw), _dev(d_imu_gyro_raw),
                                                      _dev(d_joint_pos), _dev(d_joint_vel), _dev(d_foot_force), _dev(d_reach), _dev(d_foot_pos_rel), _dev(d_foot_vel_rel),
                                                      C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_walk_sensors_batch_device")

    # ---- sloped ground and sensed touchdowns: a ground plane per robot under the walk step, a touch sensor on the feet of the walk sensors ----
    def walk_step_ground(self, state, R, foot, grf, contacts, R_z=None, foot_target=None, ground=None, ext_wrench=None, walk=None):
        """walk_step's dict and touch (n, 4) uint8: a1mpc_ground_step_batch.  ground (n, 3) = (z0, sx, sy) per robot, the plane (z0 + sx X) + sy Y of the world, or
        None (the walk config's own plane, or none); touch is 1 on a stance leg and on a swing leg the ground stopped"""
        wc = self.walk_config() if walk is None else walk
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6)); gr = None if ground is None else _f64(ground, (n, 3))
        Rz = None if R_z is None else _f64(R_z, (n, 9)); tg = None if foot_target is None else _f64(foot_target, (n, 12))
        state_out = state.copy(); R_out = np.zeros((n, 9)); foot_out = np.zeros((n, 12)); vel_out = np.zeros((n, 12)); touch = np.zeros((n, 4), np.uint8)
        rc = self.lib.a1mpc_ground_step_batch(self._h, C.byref(wc), n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(Rz), _dp(tg), _dp(gr),
                                                   _dp(state_out), _dp(R_out), _dp(foot_out), _dp(vel_out), _u8p(touch))
        _check(self.lib, rc, "a1mpc_ground_step_batch")
        return dict(state=state_out, R=R_out, foot=foot_out, foot_vel_body=vel_out, touch=touch)

    def walk_step_ground_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_R_z, d_foot_target, d_foot_vel_body, d_touch, d_ground=None,
                                d_ext_wrench=None, d_state_out=None, d_R_out=None, d_foot_out=None, walk=None, stream=None):
        """walk_step_device with d_ground (n, 3; None: the walk config's plane) and d_touch (n, 4 bytes, written)"""
        wc = self.walk_config() if walk is None else walk
        out = lambda o, i: _dev(i if o is None else o)
        rc = self.lib.a1mpc_ground_step_batch_device(self._h, C.byref(wc), int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf),
                                                          _dev(d_contacts), _dev(d_ext_wrench), _dev(d_R_z), _dev(d_foot_target), _dev(d_ground), out(d_state_out, d_state),
                                                          out(d_R_out, d_R), out(d_foot_out, d_foot), _dev(d_foot_vel_body), _dev(d_touch),
                                                          C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_ground_step_batch_device")

    def walk_sensors_touch(self, state, R, foot, grf, contacts, foot_vel_body=None, touch=None, touch_force=0.0, ext_wrench=None, rho_fix=None, rho_opt=None,
                           want_foot_rel=True):
        """walk_sensors' dict: a1mpc_touch_sensors_batch.  touch (n, 4) bytes or None: a swing leg with a non-zero byte reports touch_force as its foot force"""
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        tc = None if touch is None else np.ascontiguousarray(touch, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6)); vel = None if foot_vel_body is None else _f64(foot_vel_body, (n, 12))
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        out = dict(quat=np.zeros((n, 4)), imu_acc_raw=np.zeros((n, 3)), imu_gyro_raw=np.zeros((n, 3)), joint_pos=np.zeros((n, 12)), joint_vel=np.zeros((n, 12)),
                   foot_force=np.zeros((n, 4)), reach=np.zeros((n, 4), np.uint8), foot_pos_rel=np.zeros((n, 12)) if want_foot_rel else None,
                   foot_vel_rel=np.zeros((n, 12)) if want_foot_rel else None)
        rc = self.lib.a1mpc_touch_sensors_batch(self._h, n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(vel),
                                                     None if tc is None else _u8p(tc), float(touch_force), _dp(fix), _dp(opt), _dp(out["quat"]), _dp(out["imu_acc_raw"]),
                                                     _dp(out["imu_gyro_raw"]), _dp(out["joint_pos"]), _dp(out["joint_vel"]), _dp(out["foot_force"]), _u8p(out["reach"]),
                                                     _dp(out["foot_pos_rel"]), _dp(out["foot_vel_rel"]))
        _check(self.lib, rc, "a1mpc_touch_sensors_batch")
        return out

    def walk_sensors_touch_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_joint_pos, d_joint_vel,
                                  d_foot_force, d_reach, d_foot_pos_rel=None, d_foot_vel_rel=None, d_ext_wrench=None, d_foot_vel_body=None, d_touch=None, touch_force=0.0,
                                  rho_fix=None, rho_opt=None, stream=None):
        """walk_sensors_device with d_touch and touch_force: on the stream of the preceding walk_step_ground_device it reads that step's touch bytes"""
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        rc = self.lib.a1mpc_touch_sensors_batch_device(self._h, int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf), _dev(d_contacts),
                                                            _dev(d_ext_wrench), _dev(d_foot_vel_body), _dev(d_touch), float(touch_force), _dp(fix), _dp(opt), _dev(d_quat),
                                                            _dev(d_imu_acc_raw), _dev(d_imu_gyro_raw), _dev(d_joint_pos), _dev(d_joint_vel), _dev(d_foot_force), _dev(d_reach),
                                                            _dev(d_foot_pos_rel), _dev(d_foot_vel_rel), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_touch_sensors_batch_device")

    # ---- height-field terrain: one gridded field of heights under the walk step (stairs, rough ground), reached by every robot through an optional origin row ----
    def heightfield(self, heights, x0=0.0, y0=0.0, dx=1.0, dy=1.0, interp=0):
        """a HeightfieldOnDevice of heights (ny, nx): the heights as a device tensor and the a1mpc_heightfield that points at it, both kept alive by the object.  Its
        .host is the same descriptor over the host copy, for the host-pointer entries"""
        return HeightfieldOnDevice(self, heights, x0, y0, dx, dy, interp)

    @staticmethod
    def _field(field, device):
        if isinstance(field, HeightfieldOnDevice):
            return field.struct if device else field.host
        return field   # an engine.Heightfield filled by the caller

    def walk_step_heightfield(self, state, R, foot, grf, contacts, R_z=None, foot_target=None, field=None, origin=None, ext_wrench=None, walk=None, ground_out=True):
        """walk_step_ground's dict and ground (n, 3) = (hf under the body, 0, 0), or None with ground_out False: a1mpc_heightfield_step_batch.  field: what heightfield()
        returns (or an engine.Heightfield over host memory); origin (n, 3) = (ox, oy, oz) per robot or None"""
        wc = self.walk_config() if walk is None else walk
        state = np.ascontiguousarray(state, dtype=np.float64)
        n, stride = state.shape
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); grf = _f64(grf, (n, 12))
        ct = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        ext = None if ext_wrench is None else _f64(ext_wrench, (n, 6)); og = None if origin is None else _f64(origin, (n, 3))
        Rz = None if R_z is None else _f64(R_z, (n, 9)); tg = None if foot_target is None else _f64(foot_target, (n, 12))
        state_out = state.copy(); R_out = np.zeros((n, 9)); foot_out = np.zeros((n, 12)); vel_out = np.zeros((n, 12)); touch = np.zeros((n, 4), np.uint8)
        gout = np.zeros((n, 3)) if ground_out else None
        f = self._field(field, False)
        rc = self.lib.a1mpc_heightfield_step_batch(self._h, C.byref(wc), n, _dp(state), int(stride), _dp(R), _dp(foot), _dp(grf), _u8p(ct), _dp(ext), _dp(Rz), _dp(tg),
                                                   None if f is None else C.byref(f), _dp(og), _dp(state_out), _dp(R_out), _dp(foot_out), _dp(vel_out), _u8p(touch),
                                                   _dp(gout))
        _check(self.lib, rc, "a1mpc_heightfield_step_batch")
        return dict(state=state_out, R=R_out, foot=foot_out, foot_vel_body=vel_out, touch=touch, ground=gout)

    def walk_step_heightfield_device(self, n, d_state, state_stride, d_R, d_foot, d_grf, d_contacts, d_R_z, d_foot_target, d_foot_vel_body, d_touch, field=None,
                                     d_origin=None, d_ext_wrench=None, d_state_out=None, d_R_out=None, d_foot_out=None, walk=None, stream=None, d_ground_out=None):
        """walk_step_ground_device with field, d_origin (n, 3; optional) where d_ground is, and d_ground_out (n, 3; optional, written) last"""
        wc = self.walk_config() if walk is None else walk
        out = lambda o, i: _dev(i if o is None else o)
        f = self._field(field, True)
        rc = self.lib.a1mpc_heightfield_step_batch_device(self._h, C.byref(wc), int(n), _dev(d_state), int(state_stride), _dev(d_R), _dev(d_foot), _dev(d_grf),
                                                          _dev(d_contacts), _dev(d_ext_wrench), _dev(d_R_z), _dev(d_foot_target), None if f is None else C.byref(f),
                                                          _dev(d_origin), out(d_state_out, d_state), out(d_R_out, d_R), out(d_foot_out, d_foot), _dev(d_foot_vel_body),
                                                          _dev(d_touch), _dev(d_ground_out), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_heightfield_step_batch_device")

    def heightfield_sample(self, field, xy, origin=None):
        """hf at xy (n, 2), with origin (n, 3) or None -> (n,) heights: a1mpc_heightfield_sample_batch"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        og = None if origin is None else _f64(origin, (n, 3))
        out = np.zeros(n)
        f = self._field(field, False)
        rc = self.lib.a1mpc_heightfield_sample_batch(self._h, None if f is None else C.byref(f), n, _dp(xy), _dp(og), _dp(out))
        _check(self.lib, rc, "a1mpc_heightfield_sample_batch")
        return out

    def heightfield_sample_device(self, field, n, d_xy, d_height_out, d_origin=None, stream=None):
        """device pointers, asynchronous on `stream`: d_xy (n, 2), d_origin (n, 3; optional), d_height_out (n), written"""
        f = self._field(field, True)
        rc = self.lib.a1mpc_heightfield_sample_batch_device(self._h, None if f is None else C.byref(f), int(n), _dev(d_xy), _dev(d_origin), _dev(d_height_out),
                                                            C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_heightfield_sample_batch_device")

    # ---- sensor noise and IMU bias: counter-based Gaussian noise on the synthesised sensors, in place, the same bits for a robot and tick in every batch ----
    def noise_config(self, **fields):
        """a1mpc_default_noise_config (seed 0, every level 0: off) with `fields` overridden: seed, gyro_sigma, acc_sigma, gyro_bias_walk, acc_bias_walk, att_sigma,
        joint_pos_sigma, joint_vel_sigma, foot_force_sigma"""
        nc = NoiseConfig(); self.lib.a1mpc_default_noise_config(C.byref(nc))
        for k, v in fields.items():
            if not hasattr(nc, k):
                raise KeyError(k)
            setattr(nc, k, int(v) if k == "seed" else float(v))
        return nc

    def sensor_noise(self, noise, tick, quat=None, imu_acc_raw=None, imu_gyro_raw=None, joint_pos=None, joint_vel=None, foot_force=None, imu_bias=None, robot0=0, want_z=False):
        """a1mpc_sensor_noise_batch: the sensor arrays given (C-contiguous float64, n rows each, the layouts of sensor_synthesis' dict) and imu_bias (n, 6) are changed IN
        PLACE; robot0 is the global index of row 0 -> z (n, 44), the unit normals drawn, or None"""
        arrs = dict(quat=quat, imu_acc_raw=imu_acc_raw, imu_gyro_raw=imu_gyro_raw, joint_pos=joint_pos, joint_vel=joint_vel, foot_force=foot_force, imu_bias=imu_bias)
        given = {k: v for k, v in arrs.items() if v is not None}
        if not given:
            raise ValueError("sensor_noise needs one array at the least")
        n = next(iter(given.values())).shape[0]
        for k, v in given.items():
            if not (isinstance(v, np.ndarray) and v.dtype == np.float64 and v.flags.c_contiguous and v.flags.writeable and v.shape == (n, NOISE_WIDTHS[k])):
                raise ValueError(f"{k} must be a writeable C-contiguous float64 array of shape ({n}, {NOISE_WIDTHS[k]}): it is changed in place")
        z = np.zeros((n, NOISE_WIDTHS["z"])) if want_z else None
        rc = self.lib.a1mpc_sensor_noise_batch(self._h, C.byref(noise), n, int(robot0), int(tick), *[_dp(arrs[k]) for k in NOISE_SENSORS], _dp(imu_bias), _dp(z))
        _check(self.lib, rc, "a1mpc_sensor_noise_batch")
        return z

    def sensor_noise_device(self, noise, n, tick, d_quat=None, d_imu_acc_raw=None, d_imu_gyro_raw=None, d_joint_pos=None, d_joint_vel=None, d_foot_force=None, d_imu_bias=None,
                            d_z=None, robot0=0, stream=None):
        """device pointers (torch tensors), asynchronous on `stream`, in place: behind walk_sensors_device (or either of its siblings) and in front of
        control_tick_sensors_device on one stream it puts noise on that tick's sensors; tick and robot0 are passed by value"""
        rc = self.lib.a1mpc_sensor_noise_batch_device(self._h, C.byref(noise), int(n), int(robot0), int(tick), _dev(d_quat), _dev(d_imu_acc_raw), _dev(d_imu_gyro_raw),
                                                      _dev(d_joint_pos), _dev(d_joint_vel), _dev(d_foot_force), _dev(d_imu_bias), _dev(d_z),
                                                      C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_sensor_noise_batch_device")

    # ---- episode record and batch summary: what happened to each robot of a closed loop, kept on the device and read with one small copy at the end ----
    def episode_config(self, **fields):
        """a1mpc_default_episode_config (min_up 0.5, min_height 0.12) with `fields` overridden"""
        ec = EpisodeConfig(); self.lib.a1mpc_default_episode_config(C.byref(ec))
        for k, v in fields.items():
            if not hasattr(ec, k):
                raise KeyError(k)
            setattr(ec, k, float(v))
        return ec

    def episode_update(self, episode, tick, state, R_world, root_pos=None, root_lin_vel=None, root_lin_vel_d=None, root_pos_d_z=None, ground=None, grf_body=None, contacts=None,
                       status=None, reach=None, config=None):
        """a1mpc_episode_update_batch: `episode` (n, 16), a writeable C-contiguous float64 array, is updated IN PLACE with this tick's truth (state (n, 12 / 13 / 22),
        R_world (n, 9)) and whichever of the optional inputs are given (EPISODE_INPUTS) -> episode"""
        if not (isinstance(episode, np.ndarray) and episode.dtype == np.float64 and episode.flags.c_contiguous and episode.flags.writeable and episode.ndim == 2
                and episode.shape[1] == EPISODE_WORDS):
            raise ValueError(f"episode must be a writeable C-contiguous float64 array of shape (n, {EPISODE_WORDS}): it is changed in place")
        n = episode.shape[0]
        state = np.ascontiguousarray(state, dtype=np.float64); R_world = np.ascontiguousarray(R_world, dtype=np.float64).reshape(n, 9)
        if state.shape[0] != n:
            raise ValueError("state must have one row per record")
        given = dict(root_pos=root_pos, root_lin_vel=root_lin_vel, root_lin_vel_d=root_lin_vel_d, root_pos_d_z=root_pos_d_z, ground=ground, grf_body=grf_body,
                     contacts=contacts, status=status, reach=reach)
        args = []
        for k, cols, dt in EPISODE_INPUTS:
            v = given[k]
            if v is not None:
                v = np.ascontiguousarray(v, dtype=dt).reshape((n, cols) if cols else (n,))
            given[k] = v   # (kept alive over the call)
            args.append(None if v is None else v.ctypes.data_as(C.POINTER({np.float64: C.c_double, np.uint8: C.c_uint8, np.int32: C.c_int32}[dt])))
        ec = config if config is not None else self.episode_config()
        rc = self.lib.a1mpc_episode_update_batch(self._h, C.byref(ec), n, int(tick), _dp(state), int(state.shape[1]), _dp(R_world), *args, _dp(episode))
        _check(self.lib, rc, "a1mpc_episode_update_batch")
        return episode

    def episode_update_device(self, n, tick, d_episode, d_state, state_stride, d_R_world, d_root_pos=None, d_root_lin_vel=None, d_root_lin_vel_d=None, d_root_pos_d_z=None,
                              d_ground=None, d_grf_body=None, d_contacts=None, d_status=None, d_reach=None, config=None, stream=None):
        """device pointers (torch tensors), asynchronous on `stream`: behind the plant step of a tick on the loop's stream it folds that tick into the n records of
        d_episode (n x 16 float64, zeroed at the start of an episode); tick is passed by value"""
        ec = config if config is not None else self.episode_config()
        rc = self.lib.a1mpc_episode_update_batch_device(self._h, C.byref(ec), int(n), int(tick), _dev(d_state), int(state_stride), _dev(d_R_world), _dev(d_root_pos),
                                                        _dev(d_root_lin_vel), _dev(d_root_lin_vel_d), _dev(d_root_pos_d_z), _dev(d_ground), _dev(d_grf_body), _dev(d_contacts),
                                                        _dev(d_status), _dev(d_reach), _dev(d_episode), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_episode_update_batch_device")

    def episode_summary(self, episode):
        """a1mpc_episode_summary_batch: n records (n, 16) -> the 20 words of SUMMARY_FIELDS"""
        episode = np.ascontiguousarray(episode, dtype=np.float64)
        if episode.ndim != 2 or episode.shape[1] != EPISODE_WORDS:
            raise ValueError(f"episode must have shape (n, {EPISODE_WORDS})")
        out = np.zeros(len(SUMMARY_FIELDS))
        _check(self.lib, self.lib.a1mpc_episode_summary_batch(self._h, episode.shape[0], _dp(episode), _dp(out)), "a1mpc_episode_summary_batch")
        return out

    def episode_summary_device(self, n, d_episode, d_summary, stream=None):
        """device pointers, asynchronous on `stream`: d_summary (20 float64) receives the summary of the n records of d_episode"""
        rc = self.lib.a1mpc_episode_summary_batch_device(self._h, int(n), _dev(d_episode), _dev(d_summary), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_episode_summary_batch_device")

    # ---- respawn: a robot whose episode is over gets its lane back on the device -- the decision with its hold, the masked reset of the handle's state, the caller's rows ----
    def respawn_config(self, **fields):
        """a1mpc_default_respawn_config (codes 0xE, max_ticks 0, hold_ticks 10, what 0xF) with `fields` overridden"""
        rc = RespawnConfig(); self.lib.a1mpc_default_respawn_config(C.byref(rc))
        for k, v in fields.items():
            if k not in [f for f, _ in RespawnConfig._fields_]:
                raise KeyError(k)
            setattr(rc, k, v)
        return rc

    def respawn_reset(self, mask, what=15):
        """a1mpc_respawn_reset_batch: the state of every robot b with mask[b] & 1 is cleared in the blocks `what` names (RESPAWN_*); synchronises like every host entry"""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        _check(self.lib, self.lib.a1mpc_respawn_reset_batch(self._h, mask.shape[0], _u8p(mask), int(what)), "a1mpc_respawn_reset_batch")

    def respawn_reset_device(self, n, d_mask, what=15, stream=None):
        """device pointer, asynchronous on `stream`: d_mask is n bytes"""
        rc = self.lib.a1mpc_respawn_reset_batch_device(self._h, int(n), _dev(d_mask), int(what), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_respawn_reset_batch_device")

    def respawn(self, episode, life, finished=None, config=None):
        """a1mpc_respawn_batch: episode (n, 16) float64, life (n, 2) int32 and, when given, finished (n, 16) float64 are changed IN PLACE (writeable C-contiguous
        arrays) -> mask (n,) uint8: 0 left alone, 1 respawned, 2 held"""
        for a, dt, w, name in ((episode, np.float64, EPISODE_WORDS, "episode"), (life, np.int32, 2, "life"), (finished, np.float64, EPISODE_WORDS, "finished")):
            if a is None and name == "finished":
                continue
            if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.flags.writeable and a.ndim == 2 and a.shape == (episode.shape[0], w)):
                raise ValueError(f"{name} must be a writeable C-contiguous {np.dtype(dt).name} array of shape (n, {w}): it is changed in place")
        mask = np.zeros(episode.shape[0], dtype=np.uint8)
        rc = config if config is not None else self.respawn_config()
        _check(self.lib, self.lib.a1mpc_respawn_batch(self._h, C.byref(rc), episode.shape[0], _dp(episode), _ip(life), _dp(finished), _u8p(mask)), "a1mpc_respawn_batch")
        return mask

    def respawn_device(self, n, d_episode, d_life, d_mask, d_finished=None, config=None, stream=None):
        """device pointers, asynchronous on `stream`: d_episode n x 16 float64, d_life n x 2 int32, d_mask n bytes (out), d_finished n x 16 float64 or None"""
        rc = config if config is not None else self.respawn_config()
        st = self.lib.a1mpc_respawn_batch_device(self._h, C.byref(rc), int(n), _dev(d_episode), _dev(d_life), _dev(d_finished), _dev(d_mask),
                                                 C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, st, "a1mpc_respawn_batch_device")

    def respawn_rows_device(self, n, d_mask, rows, stream=None):
        """a1mpc_respawn_rows_device: rows is a list of (dst, src, when) torch tensors on the device -- dst has n rows at the least, src one row (the template of every
        robot) or n at the least; the row is dst's row in bytes; when: 1 on respawn, 2 on a held tick, 3 on both"""
        table = (RespawnRows * max(len(rows), 1))()
        for k, (dst, src, when) in enumerate(rows):
            row_bytes = dst[0].numel() * dst.element_size()
            if not (dst.is_contiguous() and src.is_contiguous() and src.numel() * src.element_size() % row_bytes == 0):
                raise ValueError(f"rows[{k}]: dst and src must be contiguous, src a whole number of dst's rows")
            table[k] = RespawnRows(dst.data_ptr(), src.data_ptr(), row_bytes, src.numel() * src.element_size() // row_bytes, int(when))
        rc = self.lib.a1mpc_respawn_rows_device(self._h, int(n), _dev(d_mask), table, len(rows), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_respawn_rows_device")

    def last_control_tick_ms(self):
        ms = C.c_float(0); fused = C.c_int32(0)
        _check(self.lib, self.lib.a1mpc_last_control_tick_ms(self._h, C.byref(ms), C.byref(fused)), "a1mpc_last_control_tick_ms")
        return float(ms.value), bool(fused.value)

    TICK_STAGES = ("formation", "ruiz", "handoff", "factor", "iterate", "check", "outputs", "total")

    def last_tick_stage_cycles(self):
        """dict(stage -> shader-clock cycles summed over the QPs of the last profiled fused / latency tick; qps) -- a1mpc_last_tick_stage_cycles"""
        c = np.zeros(8); q = C.c_int32(0)
        _check(self.lib, self.lib.a1mpc_last_tick_stage_cycles(self._h, _dp(c), C.byref(q)), "a1mpc_last_tick_stage_cycles")
        return dict(zip(self.TICK_STAGES, map(float, c)), qps=int(q.value))

    def last_warm_start_mode(self):
        m = C.c_int32(-9)
        _check(self.lib, self.lib.a1mpc_last_warm_start_mode(self._h, C.byref(m)), "a1mpc_last_warm_start_mode")
        return int(m.value)

    def get_workspace_scaling(self, n):
        """warm_start = 2: (D (n, 12 h), E (n, 20 h), c (n)) of the last update-path tick (a1mpc_get_workspace_scaling)"""
        h = self.horizon
        D = np.zeros((n, NU * h)); E = np.zeros((n, 20 * h)); c = np.zeros(n)
        _check(self.lib, self.lib.a1mpc_get_workspace_scaling(self._h, int(n), _dp(D), _dp(E), _dp(c)), "a1mpc_get_workspace_scaling")
        return D, E, c

    def get_workspace_z(self, n):
        """warm_start = 2: the unscaled z the update path keeps beside (x, y, rho), (n, 20 h) in the reference's row order (a1mpc_get_workspace_z)"""
        z = np.zeros((n, 20 * self.horizon))
        _check(self.lib, self.lib.a1mpc_get_workspace_z(self._h, int(n), _dp(z)), "a1mpc_get_workspace_z")
        return z

    # ---- N1: compact tick records (x0 / x_ref built on the device, S/A1RobotControl.cpp:452-488) ----
    def solve_ticks(self, tick, R, foot, contact, want_u=False):
        h = self.horizon
        tick = _f64(tick, (-1, 22)); n = tick.shape[0]
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12))
        contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4)
        grf = np.zeros((n, 12)); u = np.zeros((n, NU * h)) if want_u else None
        iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_solve_batch_ticks(self._h, n, _dp(tick), _dp(R), _dp(foot), contact.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(grf),
                                              _dp(u), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_solve_batch_ticks")
        return dict(grf=grf, u=u, iters=iters, status=status)

    # ---- device pointers (torch tensors already resident in HBM), asynchronous on `stream` ----
    def solve_device(self, n, d_x0, d_xref, d_R, d_foot, d_contact, d_grf, d_u=None, d_iters=None, d_status=None, stream=None):
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_solve_batch_device(self._h, int(n), ptr(d_x0), ptr(d_xref), ptr(d_R), ptr(d_foot), ptr(d_contact),
                                               ptr(d_grf), ptr(d_u), ptr(d_iters), ptr(d_status),
                                               C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_solve_batch_device")

    def balance_solve(self, root_acc, R, Rz, foot, contact, qp=None):
        if qp is None:
            qp = BalanceConfig(); self.lib.a1mpc_default_balance_config(C.byref(qp))
        root_acc = _f64(root_acc, (-1, 6)); n = root_acc.shape[0]
        R = _f64(R, (n, 9)); Rz = _f64(Rz, (n, 9)); foot = _f64(foot, (n, 12))
        contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4)
        grf = np.zeros((n, 12)); f = np.zeros((n, 12)); iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_balance_solve_batch(self._h, C.byref(qp), n, _dp(root_acc), _dp(R), _dp(Rz), _dp(foot),
                                                contact.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(grf), _dp(f), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_balance_solve_batch")
        return dict(grf=grf, f_world=f, iters=iters, status=status)

    # ---- the balance-QP stance controller (stance_leg_control_type 0, S/A1RobotControl.cpp:325-332, 377-444): PD wrench, device solve, contact block, one-call tick ----
    def balance_gains(self, **fields):
        """a1mpc_default_balance_gains with `fields` (kp_linear, kd_linear, kp_angular, kd_angular: three numbers each) overridden"""
        g = BalanceGains(); self.lib.a1mpc_default_balance_gains(C.byref(g))
        for k, v in fields.items():
            getattr(g, k)[:] = [float(x) for x in v]
        return g

    def balance_wrench(self, root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, root_ang_vel, R, gains=None):
        """root_acc (n, 6) of a1mpc_balance_wrench_batch: host arrays, *_d velocities in the body frame, the others in the world frame; mass is the handle's"""
        g = self.balance_gains() if gains is None else gains
        pd = _f64(root_pos_d, (-1, 3)); n = pd.shape[0]
        arrs = [pd] + [_f64(a, (n, 3)) for a in (root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, root_ang_vel)] + [_f64(R, (n, 9))]
        acc = np.zeros((n, 6))
        _check(self.lib, self.lib.a1mpc_balance_wrench_batch(self._h, C.byref(g), n, *[_dp(a) for a in arrs], _dp(acc)), "a1mpc_balance_wrench_batch")
        return acc

    def balance_wrench_device(self, n, d_root_pos_d, d_root_pos, d_root_lin_vel_d, d_root_lin_vel, d_root_euler_d, d_root_euler, d_root_ang_vel_d, d_root_ang_vel, d_R,
                              d_root_acc, gains=None, stream=None):
        """a1mpc_balance_wrench_batch_device: device pointers (torch tensors), asynchronous on `stream`"""
        g = self.balance_gains() if gains is None else gains
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_balance_wrench_batch_device(self._h, C.byref(g), int(n), ptr(d_root_pos_d), ptr(d_root_pos), ptr(d_root_lin_vel_d), ptr(d_root_lin_vel),
                                                        ptr(d_root_euler_d), ptr(d_root_euler), ptr(d_root_ang_vel_d), ptr(d_root_ang_vel), ptr(d_R), ptr(d_root_acc),
                                                        C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_balance_wrench_batch_device")

    def balance_wrench_kp(self, kp_linear_xy, root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, root_ang_vel, R, gains=None):
        """root_acc (n, 6) of a1mpc_balance_wrench_kp_batch: balance_wrench with kp_linear[0:2] per robot (kp_linear_xy (n, 2), the command stage's)"""
        g = self.balance_gains() if gains is None else gains
        kp = _f64(kp_linear_xy, (-1, 2)); n = kp.shape[0]
        arrs = [kp] + [_f64(a, (n, 3)) for a in (root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, root_ang_vel)] + [_f64(R, (n, 9))]
        acc = np.zeros((n, 6))
        _check(self.lib, self.lib.a1mpc_balance_wrench_kp_batch(self._h, C.byref(g), n, *[_dp(a) for a in arrs], _dp(acc)), "a1mpc_balance_wrench_kp_batch")
        return acc

    def balance_wrench_kp_device(self, n, d_kp_linear_xy, d_root_pos_d, d_root_pos, d_root_lin_vel_d, d_root_lin_vel, d_root_euler_d, d_root_euler, d_root_ang_vel_d,
                                 d_root_ang_vel, d_R, d_root_acc, gains=None, stream=None):
        """a1mpc_balance_wrench_kp_batch_device: device pointers (torch tensors), asynchronous on `stream`"""
        g = self.balance_gains() if gains is None else gains
        rc = self.lib.a1mpc_balance_wrench_kp_batch_device(self._h, C.byref(g), int(n), *[_dev(t) for t in (d_kp_linear_xy, d_root_pos_d, d_root_pos, d_root_lin_vel_d,
                                                           d_root_lin_vel, d_root_euler_d, d_root_euler, d_root_ang_vel_d, d_root_ang_vel, d_R, d_root_acc)],
                                                           C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_balance_wrench_kp_batch_device")

    # ---- the sensor and command front end (gt_pose_callback, imu_callback and the first half of main_update, S/GazeboA1ROS.cpp:235-262, 284-300, 124-188) ----
    def sensor_config(self, imu_window=None):
        c = SensorConfig(); self.lib.a1mpc_default_sensor_config(C.byref(c))
        if imu_window is not None:
            c.imu_window = int(imu_window)
        return c

    def command_config(self, **fields):
        """a1mpc_default_command_config with `fields` overridden"""
        c = CommandConfig(); self.lib.a1mpc_default_command_config(C.byref(c))
        for k, v in fields.items():
            if not hasattr(c, k):
                raise KeyError(k)
            setattr(c, k, v)
        return c

    def sensor_frontend(self, quat, imu_acc_raw, imu_gyro_raw, cfg=None):
        """a1mpc_sensor_frontend_batch on host arrays: quat (n, 4) as w, x, y, z and the raw IMU sample -> dict(R_world, R_z (n, 9), root_euler, imu_acc, imu_ang_vel,
        root_ang_vel (n, 3)); the six filters' state of every robot lives in the handle (reset_sensor_state)"""
        cfg = self.sensor_config() if cfg is None else cfg
        q = _f64(quat, (-1, 4)); n = q.shape[0]; acc = _f64(imu_acc_raw, (n, 3)); gyro = _f64(imu_gyro_raw, (n, 3))
        out = {k: np.zeros((n, w)) for k, w in (("R_world", 9), ("R_z", 9), ("root_euler", 3), ("imu_acc", 3), ("imu_ang_vel", 3), ("root_ang_vel", 3))}
        rc = self.lib.a1mpc_sensor_frontend_batch(self._h, C.byref(cfg), n, _dp(q), _dp(acc), _dp(gyro), *[_dp(v) for v in out.values()])
        _check(self.lib, rc, "a1mpc_sensor_frontend_batch")
        return out

    def sensor_frontend_device(self, n, d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_R_world, d_R_z, d_root_euler, d_imu_acc, d_imu_ang_vel, d_root_ang_vel, cfg=None, stream=None):
        """a1mpc_sensor_frontend_batch_device: device pointers (torch tensors), asynchronous on `stream`"""
        cfg = self.sensor_config() if cfg is None else cfg
        rc = self.lib.a1mpc_sensor_frontend_batch_device(self._h, C.byref(cfg), int(n), *[_dev(t) for t in (d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_R_world, d_R_z, d_root_euler,
                                                         d_imu_acc, d_imu_ang_vel, d_root_ang_vel)], C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_sensor_frontend_batch_device")

    def reset_sensor_state(self):
        _check(self.lib, self.lib.a1mpc_reset_sensor_state(self._h), "a1mpc_reset_sensor_state")

    @staticmethod
    def command_state(n):
        """the command stage's carried state of n robots at the reference's initial values: body_height 0.3 (S/GazeboA1ROS.h:130), joy_cmd_ctrl_state 0, root_euler_d and
        root_pos_d zero (S/A1CtrlStates.h:35-36), kp_linear[0:2] = the lock values 120 (S/A1CtrlStates.h:273-274, 301), mpc_init_counter 0 (S/A1RobotControl.cpp:25)"""
        n = int(n)
        return dict(body_height=np.full(n, 0.3), ctrl_state=np.zeros(n, np.uint8), root_euler_d=np.zeros((n, 3)), root_pos_d=np.zeros((n, 3)),
                    kp_linear_xy=np.full((n, 2), 120.0), mpc_init_counter=np.zeros(n, np.int32))

    def command(self, cmd, mode_toggle, root_pos, dt, state, cfg=None):
        """a1mpc_command_batch on host arrays: cmd (n, 6), mode_toggle (n,), root_pos (n, 3); `state` (command_state(n)) is updated IN PLACE; returns
        dict(root_lin_vel_d, root_ang_vel_d (n, 3), movement_mode, mpc_active (n,) uint8, root_pos_d_z (n,))"""
        cfg = self.command_config() if cfg is None else cfg
        c = _f64(cmd, (-1, 6)); n = c.shape[0]; tg = np.ascontiguousarray(mode_toggle, dtype=np.uint8).reshape(n); pos = _f64(root_pos, (n, 3))
        for k, dt_, shape in (("body_height", np.float64, (n,)), ("ctrl_state", np.uint8, (n,)), ("root_euler_d", np.float64, (n, 3)), ("root_pos_d", np.float64, (n, 3)),
                              ("kp_linear_xy", np.float64, (n, 2)), ("mpc_init_counter", np.int32, (n,))):
            a = state[k]
            assert a.dtype == dt_ and a.flags["C_CONTIGUOUS"] and a.shape == shape, k
        out = dict(root_lin_vel_d=np.zeros((n, 3)), root_ang_vel_d=np.zeros((n, 3)), movement_mode=np.zeros(n, np.uint8), mpc_active=np.zeros(n, np.uint8), root_pos_d_z=np.zeros(n))
        rc = self.lib.a1mpc_command_batch(self._h, C.byref(cfg), n, _dp(c), _u8p(tg), _dp(pos), float(dt), _dp(state["body_height"]), _u8p(state["ctrl_state"]),
                                          _dp(state["root_euler_d"]), _dp(state["root_pos_d"]), _dp(state["kp_linear_xy"]), _ip(state["mpc_init_counter"]),
                                          _dp(out["root_lin_vel_d"]), _dp(out["root_ang_vel_d"]), _u8p(out["movement_mode"]), _u8p(out["mpc_active"]), _dp(out["root_pos_d_z"]))
        _check(self.lib, rc, "a1mpc_command_batch")
        return out

    def command_device(self, n, d_cmd, d_mode_toggle, d_root_pos, dt, d_body_height, d_ctrl_state, d_root_euler_d, d_root_pos_d, d_kp_linear_xy, d_mpc_init_counter,
                       d_root_lin_vel_d, d_root_ang_vel_d, d_movement_mode, d_mpc_active, d_root_pos_d_z, cfg=None, stream=None):
        """a1mpc_command_batch_device: device pointers (torch tensors), asynchronous on `stream`"""
        cfg = self.command_config() if cfg is None else cfg
        rc = self.lib.a1mpc_command_batch_device(self._h, C.byref(cfg), int(n), _dev(d_cmd), _dev(d_mode_toggle), _dev(d_root_pos), float(dt),
                                                 *[_dev(t) for t in (d_body_height, d_ctrl_state, d_root_euler_d, d_root_pos_d, d_kp_linear_xy, d_mpc_init_counter, d_root_lin_vel_d,
                                                                     d_root_ang_vel_d, d_movement_mode, d_mpc_active, d_root_pos_d_z)], C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_command_batch_device")

    def tick_sensors(self, sensor=None, command=None, **pointers):
        """a TickSensors: default configs unless given, device pointers (torch tensors) for TICK_SENSOR_POINTERS"""
        ts = TickSensors()
        ts.sensor = self.sensor_config() if sensor is None else sensor; ts.command = self.command_config() if command is None else command
        for k in TICK_SENSOR_POINTERS:
            t = pointers.pop(k)
            setattr(ts, k, t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        assert not pointers, pointers
        return ts

    def control_tick_sensors_device(self, params, sensors, buffers, n, stream=None):
        """a1mpc_control_tick_sensors_device: the sensor stage, the command stage and control_tick_device in one call, from raw inputs (a TickSensors)"""
        _check(self.lib, self.lib.a1mpc_control_tick_sensors_device(self._h, C.byref(params), C.byref(sensors), C.byref(buffers), int(n),
                                                                    C.c_void_p(stream) if stream else None), "a1mpc_control_tick_sensors_device")

    def balance_solve_device(self, n, d_root_acc, d_R, d_Rz, d_foot, d_contact, d_grf, d_f_world=None, d_iters=None, d_status=None, qp=None, stream=None):
        """a1mpc_balance_solve_batch_device: balance_solve on device pointers (torch tensors), asynchronous on `stream`"""
        if qp is None:
            qp = BalanceConfig(); self.lib.a1mpc_default_balance_config(C.byref(qp))
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_balance_solve_batch_device(self._h, C.byref(qp), int(n), ptr(d_root_acc), ptr(d_R), ptr(d_Rz), ptr(d_foot), ptr(d_contact), ptr(d_grf),
                                                       ptr(d_f_world), ptr(d_iters), ptr(d_status), C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_balance_solve_batch_device")

    def contacts(self, gait_counter, plan_contacts, foot_force, foot_pos_abs, cfg=None):
        """a1mpc_contacts_batch: the contact block of contact_terrain alone, on the same state; the terrain-angle filter is left as it is"""
        if cfg is None:
            cfg = ContactConfig(); self.lib.a1mpc_default_contact_config(C.byref(cfg))
        gc = _f64(gait_counter, (-1, 4)); n = gc.shape[0]; pc = np.ascontiguousarray(plan_contacts, dtype=np.uint8).reshape(n, 4)
        ff = _f64(foot_force, (n, 4)); fp = _f64(foot_pos_abs, (n, 12))
        ct = np.zeros((n, 4), np.uint8); rec = np.zeros((n, 12))
        _check(self.lib, self.lib.a1mpc_contacts_batch(self._h, C.byref(cfg), n, _dp(gc), _u8p(pc), _dp(ff), _dp(fp), _u8p(ct), _dp(rec)), "a1mpc_contacts_batch")
        return dict(contacts=ct, foot_pos_recent_contact=rec)

    def balance_tick(self, d_root_pos_d, d_root_acc=None, d_f_world=None, gains=None, qp=None):
        """a BalanceTick: default gains / QP constants unless given, device pointers (torch tensors) for root_pos_d (n, 3) and the optional outputs"""
        bt = BalanceTick()
        self.lib.a1mpc_default_balance_gains(C.byref(bt.gains)); self.lib.a1mpc_default_balance_config(C.byref(bt.qp))
        if gains is not None:
            bt.gains = gains
        if qp is not None:
            bt.qp = qp
        for k, t in (("root_pos_d", d_root_pos_d), ("root_acc", d_root_acc), ("f_world", d_f_world)):
            setattr(bt, k, None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t)))
        return bt

    def control_tick_balance_device(self, params, balance, buffers, n, stream=None):
        """a1mpc_control_tick_balance_device: one whole control tick of n robots on the balance-QP controller (a BalanceTick beside TickParams / TickBuffers)"""
        _check(self.lib, self.lib.a1mpc_control_tick_balance_device(self._h, C.byref(params), C.byref(balance), C.byref(buffers), int(n),
                                                                    C.c_void_p(stream) if stream else None), "a1mpc_control_tick_balance_device")

    # ---- N2a: gait plan + Raibert foothold (S/A1RobotControl.cpp:148-202) ----
    def update_plan(self, movement_mode, gait_counter, gait_counter_speed, root_lin_vel, Rz, R, root_pos, root_lin_vel_d, gait=None):
        if gait is None:
            gait = GaitConfig(); self.lib.a1mpc_default_gait_config(C.byref(gait))
        gc = np.array(gait_counter, dtype=np.float64).reshape(-1, 4); n = gc.shape[0]
        mm = np.ascontiguousarray(movement_mode, dtype=np.uint8).reshape(n)
        spd = _f64(gait_counter_speed, (n, 4)); v = _f64(root_lin_vel, (n, 3)); Rz = _f64(Rz, (n, 9)); R = _f64(R, (n, 9))
        pos = _f64(root_pos, (n, 3)); vd = _f64(root_lin_vel_d, (n, 3))
        pc = np.zeros((n, 4), np.uint8); rel = np.zeros((n, 12)); ab = np.zeros((n, 12)); wo = np.zeros((n, 12))
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = self.lib.a1mpc_update_plan_batch(self._h, C.byref(gait), n, u8(mm), _dp(gc), _dp(spd), _dp(v), _dp(Rz), _dp(R), _dp(pos), _dp(vd), u8(pc),
                                              _dp(rel), _dp(ab), _dp(wo))
        _check(self.lib, rc, "a1mpc_update_plan_batch")
        return dict(gait_counter=gc, plan_contacts=pc, foot_pos_target_rel=rel, foot_pos_target_abs=ab, foot_pos_target_world=wo)

    # ---- N3: GRF -> joint torques (S/A1RobotControl.cpp:289-319) ----
    def joint_torques(self, active, contacts, j_foot_blocks, grf, f_kin, km_foot, torques_gravity, joint_torques_prev):
        tau = np.array(joint_torques_prev, dtype=np.float64).reshape(-1, 12); n = tau.shape[0]
        act = np.ascontiguousarray(active, dtype=np.uint8).reshape(n); c = np.ascontiguousarray(contacts, dtype=np.uint8).reshape(n, 4)
        Jb = _f64(j_foot_blocks, (n, 36)); g = _f64(grf, (n, 12)); fk = _f64(f_kin, (n, 12)); km = _f64(km_foot, (3,)); tg = _f64(torques_gravity, (n, 12))
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = self.lib.a1mpc_joint_torques_batch(self._h, n, u8(act), u8(c), _dp(Jb), _dp(g), _dp(fk), _dp(km), _dp(tg), _dp(tau))
        _check(self.lib, rc, "a1mpc_joint_torques_batch")
        return tau

    # ---- N2b: contacts, recent-contact filters, terrain pitch (S/A1RobotControl.cpp:256-282, 566-582, 335-376); state lives on the device ----
    def contact_terrain(self, gait_counter, plan_contacts, foot_force, foot_pos_abs, root_pos_z, root_euler_d_pitch, cfg=None):
        if cfg is None:
            cfg = ContactConfig(); self.lib.a1mpc_default_contact_config(C.byref(cfg))
        gc = np.ascontiguousarray(gait_counter, dtype=np.float64).reshape(-1, 4); n = gc.shape[0]; pc = np.ascontiguousarray(plan_contacts, dtype=np.uint8).reshape(n, 4)
        ff = _f64(foot_force, (n, 4)); fp = _f64(foot_pos_abs, (n, 12)); z = _f64(root_pos_z, (n,))
        pd = np.array(root_euler_d_pitch, dtype=np.float64).reshape(n)
        ct = np.zeros((n, 4), np.uint8); rec = np.zeros((n, 12)); ta = np.zeros(n)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = self.lib.a1mpc_contact_terrain_batch(self._h, C.byref(cfg), n, _dp(gc), u8(pc), _dp(ff), _dp(fp), _dp(z), _dp(pd), u8(ct), _dp(rec), _dp(ta))
        _check(self.lib, rc, "a1mpc_contact_terrain_batch")
        return dict(contacts=ct, foot_pos_recent_contact=rec, terrain_angle=ta, root_euler_d_pitch=pd)

    # ---- N4a: swing-leg targets + foot PD force (S/A1RobotControl.cpp:204-254); the three state arrays are updated in place ----
    def swing_legs(self, Rz, foot_pos_abs, gait_counter, foot_pos_target_rel, foot_pos_start, rel_last, target_last, kp=(300.0, 400.0, 400.0),
                   kd=(8.0, 8.0, 8.0), counter_per_swing=120.0, dt=0.0025):
        n = foot_pos_start.shape[0]
        for st in (foot_pos_start, rel_last, target_last):
            assert st.dtype == np.float64 and st.flags["C_CONTIGUOUS"] and st.shape == (n, 12)
        Rz = _f64(Rz, (n, 9)); fa = _f64(foot_pos_abs, (n, 12)); gc = _f64(gait_counter, (n, 4)); tr = _f64(foot_pos_target_rel, (n, 12))
        kp = _f64(kp, (3,)); kd = _f64(kd, (3,)); cur = np.zeros((n, 12)); kin = np.zeros((n, 12))
        rc = self.lib.a1mpc_swing_legs_batch(self._h, n, counter_per_swing, dt, _dp(Rz), _dp(fa), _dp(gc), _dp(tr), _dp(kp), _dp(kd), _dp(foot_pos_start),
                                             _dp(rel_last), _dp(target_last), _dp(cur), _dp(kin))
        _check(self.lib, rc, "a1mpc_swing_legs_batch")
        return cur, kin

    # ---- N4b: leg kinematics (S/GazeboA1ROS.cpp:264-279) ----
    A1_RHO_FIX = np.array([[0.1805, 0.047, 0.0838, 0.21, 0.21], [0.1805, -0.047, -0.0838, 0.21, 0.21], [-0.1805, 0.047, 0.0838, 0.21, 0.21],
                           [-0.1805, -0.047, -0.0838, 0.21, 0.21]])

    def leg_state(self, joint_pos, joint_vel, R, root_pos, root_lin_vel, rho_fix=None, rho_opt=None):
        q = _f64(joint_pos, (-1, 12)); n = q.shape[0]
        qd = _f64(joint_vel, (n, 12)); R = _f64(R, (n, 9)); pos = _f64(root_pos, (n, 3)); vel = _f64(root_lin_vel, (n, 3))
        fix = _f64(self.A1_RHO_FIX if rho_fix is None else rho_fix, (4, 5)); opt = _f64(np.zeros((4, 3)) if rho_opt is None else rho_opt, (4, 3))
        names = ("foot_pos_rel", "Jb", "foot_vel_rel", "foot_pos_abs", "foot_vel_abs", "foot_pos_world", "foot_vel_world")
        out = {k: np.zeros((n, 36 if k == "Jb" else 12)) for k in names}
        rc = self.lib.a1mpc_leg_state_batch(self._h, n, _dp(q), _dp(qd), _dp(R), _dp(pos), _dp(vel), _dp(fix), _dp(opt), *[_dp(out[k]) for k in names])
        _check(self.lib, rc, "a1mpc_leg_state_batch")
        return out

    # ---- N4c: A1BasicEKF (S/A1BasicEKF.cpp); filter state per robot on the device, first call = init_state ----
    def ekf_update(self, dt, movement_mode, foot_force, R, imu_acc, imu_ang_vel, foot_pos_rel, foot_vel_rel, assume_flat_ground=1):
        ff = _f64(foot_force, (-1, 4)); n = ff.shape[0]
        mm = np.ascontiguousarray(movement_mode, dtype=np.uint8).reshape(n)
        R = _f64(R, (n, 9)); acc = _f64(imu_acc, (n, 3)); w = _f64(imu_ang_vel, (n, 3)); fk = _f64(foot_pos_rel, (n, 12)); fv = _f64(foot_vel_rel, (n, 12))
        pos = np.zeros((n, 3)); vel = np.zeros((n, 3)); ec = np.zeros((n, 4), np.uint8)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = self.lib.a1mpc_ekf_update_batch(self._h, n, float(dt), int(assume_flat_ground), u8(mm), _dp(ff), _dp(R), _dp(acc), _dp(w), _dp(fk), _dp(fv),
                                             _dp(pos), _dp(vel), u8(ec))
        _check(self.lib, rc, "a1mpc_ekf_update_batch")
        return pos, vel, ec

    def reset_ekf_state(self):
        _check(self.lib, self.lib.a1mpc_reset_ekf_state(self._h), "a1mpc_reset_ekf_state")

    def reset_contact_state(self):
        _check(self.lib, self.lib.a1mpc_reset_contact_state(self._h), "a1mpc_reset_contact_state")

    def set_schedule(self, history=True):
        """queue order of batches beyond the resident set: previous solve's longest-first (default) or index order"""
        _check(self.lib, self.lib.a1mpc_set_schedule(self._h, 1 if history else 0), "a1mpc_set_schedule")

    def reset_warm_start(self):
        _check(self.lib, self.lib.a1mpc_reset_warm_start(self._h), "a1mpc_reset_warm_start")

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(self.lib, self.lib.a1mpc_last_kernel_ms(self._h, C.byref(ms)), "a1mpc_last_kernel_ms")
        return float(ms.value)

    def last_stage_ms(self):
        a = C.c_float(); b = C.c_float()
        _check(self.lib, self.lib.a1mpc_last_stage_ms(self._h, C.byref(a), C.byref(b)), "a1mpc_last_stage_ms")
        return float(a.value), float(b.value)

    def last_nfact(self, n):
        out = np.zeros(int(n), np.int32)
        _check(self.lib, self.lib.a1mpc_last_nfact(self._h, int(n), _ip(out)), "a1mpc_last_nfact")
        return out

    def kernel_info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.lib, self.lib.a1mpc_kernel_info(self._h, C.byref(a), C.byref(b), C.byref(c)), "a1mpc_kernel_info")
        return dict(lds_bytes_per_workgroup=a.value, qps_per_workgroup=b.value, threads_per_workgroup=c.value)


# ---- work model used for roofline.achieved (DESIGN.md "Measurement") --------------
class Pipeline:
    """a1mpc_pipeline: `depth` engine handles on `depth` HIP streams of one GPU, batches submitted round-robin so that the next batch's
    set-up kernel and persistent rows fill the tail of the one before (include/a1mpc.h).  Device pointers (torch tensors) or host arrays."""

    def __init__(self, cfg, max_batch, device=0, depth=2):
        self.lib = load_library()
        self.cfg = cfg; self.horizon = int(cfg.horizon); self.max_batch = int(max_batch); self.device = int(device)
        self._p = C.c_void_p()
        _check(self.lib, self.lib.a1mpc_pipeline_create(C.byref(cfg), self.max_batch, self.device, int(depth), C.byref(self._p)), "a1mpc_pipeline_create")
        d = C.c_int32(0)
        _check(self.lib, self.lib.a1mpc_pipeline_depth(self._p, C.byref(d)), "a1mpc_pipeline_depth")
        self.depth = int(d.value)

    def submit_device(self, n, d_x0, d_xref, d_R, d_foot, d_contact, d_grf, d_u=None, d_iters=None, d_status=None, slot=-1, fresh=True, after_stream=None):
        """returns the slot the batch went to; outputs are valid after wait(slot) / join(slot, stream)"""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        k = C.c_int32(-1)
        rc = self.lib.a1mpc_pipeline_submit_device(self._p, int(slot), 1 if fresh else 0, int(n), ptr(d_x0), ptr(d_xref), ptr(d_R), ptr(d_foot), ptr(d_contact),
                                                   ptr(d_grf), ptr(d_u), ptr(d_iters), ptr(d_status), C.c_void_p(int(after_stream)) if after_stream else None, C.byref(k))
        _check(self.lib, rc, "a1mpc_pipeline_submit_device")
        return int(k.value)

    def submit(self, x0, xref, R, foot, contact, out, slot=-1, fresh=True):
        """host arrays in (a1mpc_solve_batch's layouts; snapshotted before the call returns), host arrays out: `out` = dict(grf=, [u=], [iters=], [status=]) of
        preallocated C-contiguous numpy arrays that wait(slot) -- or the next submit to the slot -- fills.  Returns the slot."""
        n = int(x0.shape[0])
        x0 = np.ascontiguousarray(x0, np.float64); xref = np.ascontiguousarray(xref, np.float64); R = np.ascontiguousarray(R, np.float64)
        foot = np.ascontiguousarray(foot, np.float64); contact = np.ascontiguousarray(contact, np.uint8)
        # the C side memcpys n*12 (grf) / n*12*H (u) doubles and n int32 (iters, status) into these arrays LATER (wait / the next submit): a wrong dtype or a short
        # array would be a deferred heap overflow, so dtype and total size are checked here, before the call
        need = {"grf": (np.float64, n * NU), "u": (np.float64, n * NU * self.horizon), "iters": (np.int32, n), "status": (np.int32, n)}
        for k_, a_ in out.items():
            if a_ is None:
                continue
            if k_ not in need:
                raise ValueError(f"unknown output array {k_!r}")
            dt_, size_ = need[k_]
            if not (isinstance(a_, np.ndarray) and a_.flags["C_CONTIGUOUS"] and a_.dtype == dt_ and a_.size >= size_):
                raise ValueError(f"output array {k_!r} must be a C-contiguous numpy array of {np.dtype(dt_).name} with at least {size_} elements")
        if out.get("grf") is None:
            raise ValueError("output array 'grf' is required")
        k = C.c_int32(-1)
        rc = self.lib.a1mpc_pipeline_submit(self._p, int(slot), 1 if fresh else 0, n, _dp(x0), _dp(xref), _dp(R), _dp(foot), _u8p(contact), _dp(out["grf"]),
                                            _dp(out["u"]) if out.get("u") is not None else None, _ip(out["iters"]) if out.get("iters") is not None else None,
                                            _ip(out["status"]) if out.get("status") is not None else None, C.byref(k))
        _check(self.lib, rc, "a1mpc_pipeline_submit")
        self._keep = getattr(self, "_keep", {}); self._keep[int(k.value)] = out   # the output arrays must outlive the slot's batch
        return int(k.value)

    def submit_strided_device(self, n, d_x0, d_xref, d_R, d_foot, foot_stride, d_contact, contact_stride, d_grf, d_u=None, d_iters=None, d_status=None, d_yaw_A=None,
                              slot=-1, fresh=True, after_stream=None):
        """a1mpc_pipeline_submit_strided_device: per-step feet / contact schedules / an A_c yaw of its own (the general path) with batches in flight together"""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        k = C.c_int32(-1)
        rc = self.lib.a1mpc_pipeline_submit_strided_device(self._p, int(slot), 1 if fresh else 0, int(n), ptr(d_x0), ptr(d_xref), ptr(d_R), ptr(d_foot), int(foot_stride),
                                                           ptr(d_contact), int(contact_stride), ptr(d_yaw_A), ptr(d_grf), ptr(d_u), ptr(d_iters), ptr(d_status),
                                                           C.c_void_p(int(after_stream)) if after_stream else None, C.byref(k))
        _check(self.lib, rc, "a1mpc_pipeline_submit_strided_device")
        return int(k.value)

    def submit_ticks_device(self, n, d_tick, d_R, d_foot, d_contact, d_grf, d_u=None, d_iters=None, d_status=None, slot=-1, fresh=True, after_stream=None):
        """a1mpc_pipeline_submit_ticks_device: the compact 22-number tick records (x0 / x_ref are built on the device) with batches in flight together"""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        k = C.c_int32(-1)
        rc = self.lib.a1mpc_pipeline_submit_ticks_device(self._p, int(slot), 1 if fresh else 0, int(n), ptr(d_tick), ptr(d_R), ptr(d_foot), ptr(d_contact), ptr(d_grf), ptr(d_u),
                                                         ptr(d_iters), ptr(d_status), C.c_void_p(int(after_stream)) if after_stream else None, C.byref(k))
        _check(self.lib, rc, "a1mpc_pipeline_submit_ticks_device")
        return int(k.value)

    def submit_ticks_strided_device(self, n, d_tick, d_R, d_foot, foot_stride, d_contact, contact_stride, d_grf, d_u=None, d_iters=None, d_status=None, d_yaw_A=None,
                                    slot=-1, fresh=True, after_stream=None):
        """a1mpc_pipeline_submit_ticks_strided_device: tick records with per-step feet / a contact schedule / an A_c yaw of its own, batches in flight together"""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        k = C.c_int32(-1)
        rc = self.lib.a1mpc_pipeline_submit_ticks_strided_device(self._p, int(slot), 1 if fresh else 0, int(n), ptr(d_tick), ptr(d_R), ptr(d_foot), int(foot_stride),
                                                                 ptr(d_contact), int(contact_stride), ptr(d_yaw_A), ptr(d_grf), ptr(d_u), ptr(d_iters), ptr(d_status),
                                                                 C.c_void_p(int(after_stream)) if after_stream else None, C.byref(k))
        _check(self.lib, rc, "a1mpc_pipeline_submit_ticks_strided_device")
        return int(k.value)

    def submit_strided(self, x0, xref, R, foot, foot_stride, contact, contact_stride, out, yaw_A=None, slot=-1, fresh=True):
        """a1mpc_pipeline_submit_strided: host arrays in (a1mpc_solve_batch_strided's layouts; snapshotted before the call returns), host arrays out like submit()"""
        n = int(x0.shape[0])
        x0 = np.ascontiguousarray(x0, np.float64); xref = np.ascontiguousarray(xref, np.float64); R = np.ascontiguousarray(R, np.float64)
        foot = np.ascontiguousarray(foot, np.float64); contact = np.ascontiguousarray(contact, np.uint8)
        ya = None if yaw_A is None else np.ascontiguousarray(yaw_A, np.float64)
        assert foot.size == n * (NU * self.horizon if foot_stride else NU) and contact.size == n * (4 * self.horizon if contact_stride else 4)
        need = {"grf": (np.float64, n * NU), "u": (np.float64, n * NU * self.horizon), "iters": (np.int32, n), "status": (np.int32, n)}
        for k_, a_ in out.items():
            if a_ is None:
                continue
            if k_ not in need:
                raise ValueError(f"unknown output array {k_!r}")
            dt_, size_ = need[k_]
            if not (isinstance(a_, np.ndarray) and a_.flags["C_CONTIGUOUS"] and a_.dtype == dt_ and a_.size >= size_):
                raise ValueError(f"output array {k_!r} must be a C-contiguous numpy array of {np.dtype(dt_).name} with at least {size_} elements")
        if out.get("grf") is None:
            raise ValueError("output array 'grf' is required")
        k = C.c_int32(-1)
        rc = self.lib.a1mpc_pipeline_submit_strided(self._p, int(slot), 1 if fresh else 0, n, _dp(x0), _dp(xref), _dp(R), _dp(foot), int(foot_stride), _u8p(contact), int(contact_stride),
                                                    _dp(ya), _dp(out["grf"]), _dp(out["u"]) if out.get("u") is not None else None,
                                                    _ip(out["iters"]) if out.get("iters") is not None else None, _ip(out["status"]) if out.get("status") is not None else None, C.byref(k))
        _check(self.lib, rc, "a1mpc_pipeline_submit_strided")
        self._keep = getattr(self, "_keep", {}); self._keep[int(k.value)] = out   # the output arrays must outlive the slot's batch
        return int(k.value)

    def wait(self, slot=-1):
        _check(self.lib, self.lib.a1mpc_pipeline_wait(self._p, int(slot)), "a1mpc_pipeline_wait")

    def join(self, stream, slot=-1):
        _check(self.lib, self.lib.a1mpc_pipeline_join(self._p, int(slot), C.c_void_p(int(stream)) if stream else None), "a1mpc_pipeline_join")

    def handle(self, slot):
        h = C.c_void_p()
        _check(self.lib, self.lib.a1mpc_pipeline_handle(self._p, int(slot), C.byref(h)), "a1mpc_pipeline_handle")
        return h

    def last_nfact(self, slot, n):
        out = np.zeros(int(n), np.int32)
        _check(self.lib, self.lib.a1mpc_last_nfact(self.handle(slot), int(n), _ip(out)), "a1mpc_last_nfact")
        return out

    def close(self):
        if getattr(self, "_p", None) is not None and self._p:
            self.lib.a1mpc_pipeline_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ShardedEngine:
    """a1mpc_sharded_*: one handle, the batch cut into contiguous shards over `devices` (None = all visible), transport 0 = pinned copies, 1 = RCCL"""

    def __init__(self, cfg, max_batch, devices=None, transport=0):
        self.lib = load_library(); self.horizon = int(cfg.horizon); self._h = C.c_void_p()
        dv = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        _check(self.lib, self.lib.a1mpc_sharded_create(C.byref(cfg), int(max_batch), _ip(dv), 0 if dv is None else len(dv), int(transport), C.byref(self._h)), "a1mpc_sharded_create")

    def info(self):
        n = C.c_int32(); t = C.c_int32(); d = np.zeros(64, np.int32)
        _check(self.lib, self.lib.a1mpc_sharded_info(self._h, C.byref(n), _ip(d), C.byref(t)), "a1mpc_sharded_info")
        return dict(n_shards=n.value, devices=d[:n.value].tolist(), transport=t.value)

    def solve(self, x0, xref, R, foot, contact):
        h = self.horizon
        x0 = _f64(x0, (-1, NS)); n = x0.shape[0]
        xref = _f64(xref, (n, NS * h)); R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4)
        grf = np.zeros((n, 12)); iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_sharded_solve_batch(self._h, n, _dp(x0), _dp(xref), _dp(R), _dp(foot), contact.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(grf), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_sharded_solve_batch")
        return dict(grf=grf, iters=iters, status=status)

    def solve_ticks(self, tick, R, foot, contact):
        """a1mpc_sharded_solve_batch_ticks: the compact 22-number tick records, host arrays"""
        tick = _f64(tick, (-1, 22)); n = tick.shape[0]
        R = _f64(R, (n, 9)); foot = _f64(foot, (n, 12)); contact = np.ascontiguousarray(contact, dtype=np.uint8).reshape(n, 4)
        grf = np.zeros((n, 12)); iters = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        rc = self.lib.a1mpc_sharded_solve_batch_ticks(self._h, n, _dp(tick), _dp(R), _dp(foot), contact.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(grf), _ip(iters), _ip(status))
        _check(self.lib, rc, "a1mpc_sharded_solve_batch_ticks")
        return dict(grf=grf, iters=iters, status=status)

    def solve_device(self, n, d_x0, d_xref, d_R, d_foot, d_contact, d_grf, d_iters=None, d_status=None, stream=None):
        """a1mpc_sharded_solve_batch_device: the batch resident on shard 0's GPU (torch tensors of that device)"""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_sharded_solve_batch_device(self._h, int(n), ptr(d_x0), ptr(d_xref), ptr(d_R), ptr(d_foot), ptr(d_contact), ptr(d_grf), ptr(d_iters), ptr(d_status),
                                                       C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_sharded_solve_batch_device")

    def solve_ticks_device(self, n, d_tick, d_R, d_foot, d_contact, d_grf, d_iters=None, d_status=None, stream=None):
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        rc = self.lib.a1mpc_sharded_solve_batch_ticks_device(self._h, int(n), ptr(d_tick), ptr(d_R), ptr(d_foot), ptr(d_contact), ptr(d_grf), ptr(d_iters), ptr(d_status),
                                                             C.c_void_p(int(stream)) if stream else None)
        _check(self.lib, rc, "a1mpc_sharded_solve_batch_ticks_device")

    def last_transfer(self):
        a = C.c_int64(); b = C.c_int64()
        _check(self.lib, self.lib.a1mpc_sharded_last_transfer(self._h, C.byref(a), C.byref(b)), "a1mpc_sharded_last_transfer")
        return dict(scatter_bytes=int(a.value), gather_bytes=int(b.value))

    def shard_handle(self, g):
        h = C.c_void_p()
        _check(self.lib, self.lib.a1mpc_sharded_handle(self._h, int(g), C.byref(h)), "a1mpc_sharded_handle")
        return h

    def reset_warm_start(self):
        n = self.info()["n_shards"]
        for g in range(n):
            _check(self.lib, self.lib.a1mpc_reset_warm_start(self.shard_handle(g)), "a1mpc_reset_warm_start")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.a1mpc_sharded_destroy(self._h); self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def algorithmic_flops(h, iters, nfact):
    """F(h, iters, nfact) of the structured dense-condensed algorithm, per solve (numpy-broadcastable)."""
    iters = np.asarray(iters, dtype=np.float64); nfact = np.asarray(nfact, dtype=np.float64)
    f_cond = 3744.0 * h * (h + 1) * (h + 2) / 6.0 + 4056.0 * (h - 1) + 312.0 * h * h + 364.0 * h
    f_fact = 576.0 * h ** 3
    f_iter = 288.0 * h * h + 464.0 * h
    f_chk = 288.0 * h * h + 336.0 * h
    return f_cond + nfact * f_fact + iters * f_iter + np.ceil(iters / 25.0) * f_chk


def algorithmic_bytes(h):
    """Compulsory HBM bytes per solve: input record + 12 GRF doubles."""
    return 8 * (38 + 13 * h) + 96
