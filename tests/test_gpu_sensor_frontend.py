"""GPU: the sensor / command front end through the C ABI -- a1mpc_sensor_frontend_batch(_device) against the reference's own compiled quat_to_euler and
MovingWindowFilter (oracle/_ref) and the numpy restatement of the two rotation matrices, a1mpc_command_batch(_device) against the restatement of main_update's first
half (tests/frontend_ref.py), a1mpc_control_tick_sensors_device against the three entries chained by hand, a1mpc_balance_wrench_kp_batch(_device) against the
batch-wide entry and the oracle.  Sizes 1 / 63 / 64 / 65 / 257 on handles of 512, NaN-poisoned tails behind every device output.  Device memory is torch tensors."""
import ctypes as C

import numpy as np
import pytest

import balance_common as BC
import frontend_ref as FR
import ref as REF
from gpu_common import tick_buffers, tick_inputs, tick_world

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not REF.build(), reason="oracle/_ref not built and the reference's sources absent")]

OK, INVALID, TOO_LARGE = 0, 1, 5
CALLS = 12                    # the fill phase, the first full window, two wrap-arounds of window 5
SENSOR_OUT = (("R_world", 9), ("R_z", 9), ("root_euler", 3), ("imu_acc", 3), ("imu_ang_vel", 3), ("root_ang_vel", 3))   # the C ABI's order
TAIL = 7


def _cfg(pkg, scen, h=10, **over):
    return pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h, **over)


def _dev():
    import torch
    dev = torch.device("cuda", 0)
    return torch, dev, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))


def _ulps(a, b):
    """distance in units of the last place of b, elementwise (finite entries)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.spacing(np.abs(b))


def _poisoned(torch, dev, rows, shapes):
    return {k: torch.full((rows, w), float("nan"), dtype=torch.float64, device=dev) for k, w in shapes}


def _sensor_device(torch, dev, T, eng, q, acc, gyro, n, cfg=None, stream=None):
    d = [T(q), T(acc), T(gyro)]
    out = _poisoned(torch, dev, n + TAIL, SENSOR_OUT)
    torch.cuda.synchronize()
    eng.sensor_frontend_device(n, *d, *out.values(), cfg=cfg, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_sensor(out, n, q, eul_ref, filt_ref, label, worst):
    """one call's outputs against the reference (rows n .. : the poisoned tail)"""
    nan = np.isnan(q).any(1)
    assert np.array_equal(out["R_world"][:n], FR.quat_to_rotation(q), equal_nan=True), label
    e = out["root_euler"][:n]
    assert np.array_equal(np.isnan(e).any(1), nan) and np.abs(e[~nan] - eul_ref[~nan]).max() <= 1e-12, (label, np.abs(e[~nan] - eul_ref[~nan]).max())
    worst["euler_abs"] = max(worst["euler_abs"], float(np.abs(e[~nan] - eul_ref[~nan]).max()))
    worst["euler_ulp"] = max(worst["euler_ulp"], float(np.nanmax(_ulps(e[~nan], eul_ref[~nan]))))
    worst["Rz_abs"] = max(worst["Rz_abs"], FR.assert_yaw_rotation(out["R_z"][:n], eul_ref[:, 2], 1e-12))
    want_z = FR.yaw_rotation(eul_ref[~nan, 2])
    big = np.abs(want_z) > 0.5     # (ulps of the entries that are not close to a zero of sin / cos, where one ulp of the angle is many of the entry)
    worst["Rz_ulp"] = max(worst["Rz_ulp"], float(_ulps(out["R_z"][:n][~nan][big], want_z[big]).max()))
    assert np.array_equal(out["imu_acc"][:n], filt_ref[:, :3]) and np.array_equal(out["imu_ang_vel"][:n], filt_ref[:, 3:]), label
    assert np.array_equal(out["root_ang_vel"][:n], FR.rotate(out["R_world"][:n], out["imu_ang_vel"][:n]), equal_nan=True), label
    for k, v in out.items():
        assert np.isnan(v[n:]).all(), (label, k)


# ---------------------------------------------------------------------------------------------------------------- the sensor stage
@pytest.mark.parametrize("n", FR.SIZES)
def test_sensor_stage_equals_the_reference_over_twelve_calls(pkg, scen, n):
    """the rows and samples of tests/test_frontend_host.py through a1mpc_sensor_frontend_batch_device on a handle of 512: R_world, the filters and root_ang_vel bit for
    bit, root_euler and R_z within 1e-12 (the device library's atan2 / asin / sin / cos on bit-identical arguments); the host entry on a second handle gives the
    device entry's bits.  Prints the largest distance in ulp."""
    torch, dev, T = _dev()
    rng = np.random.default_rng(100 + n)
    q = FR.quaternion_rows(rng, n); FR.assert_special_rows_are_special(q)
    seq = FR.imu_sequence(rng, CALLS, n); FR.assert_samples_take_both_branches(seq, (1, 3, 5))
    filt = FR.reference_filters(REF, 5, seq); eul = FR.reference_euler(REF, q)
    worst = dict(euler_abs=0.0, euler_ulp=0.0, Rz_abs=0.0, Rz_ulp=0.0)
    with pkg.Engine(_cfg(pkg, scen), 512, 0) as eng, pkg.Engine(_cfg(pkg, scen), 512, 0) as e_host:
        st = torch.cuda.Stream(device=dev)
        for t in range(CALLS):
            out = _sensor_device(torch, dev, T, eng, q, seq[t, :, :3], seq[t, :, 3:], n, stream=st.cuda_stream if t % 2 else None)
            _check_sensor(out, n, q, eul, filt[t], (n, t), worst)
            host = e_host.sensor_frontend(q, seq[t, :, :3], seq[t, :, 3:])
            for k, _ in SENSOR_OUT:
                assert np.array_equal(host[k], out[k][:n], equal_nan=True), (t, k, "host entry")
    print(f"sensor stage n {n}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("window", [1, 3, 5])
def test_filter_windows_reset_smaller_batch_and_a_changed_window(pkg, scen, window):
    """windows 1, 3 and 5 against ref_filter_run on every call; calls 3 and 4 run 20 of the 65 robots only and every position keeps its own state; a reset after call 7
    restarts the fill phase; another window without a reset is refused and leaves state and outputs alone, after a reset it is taken"""
    torch, dev, T = _dev()
    rng = np.random.default_rng(7 + window); n, small = 65, 20
    q = FR.quaternion_rows(rng, n)
    seq = FR.imu_sequence(rng, CALLS, n)
    with pkg.Engine(_cfg(pkg, scen), 512, 0) as eng:
        cfg = eng.sensor_config(window)
        fed = [[] for _ in range(n)]
        for t in range(CALLS):
            if t == 7:
                eng.reset_sensor_state(); fed = [[] for _ in range(n)]
            m = small if t in (3, 4) else n
            out = _sensor_device(torch, dev, T, eng, q[:m], seq[t, :m, :3], seq[t, :m, 3:], m, cfg=cfg)
            for b in range(m):
                fed[b].append(seq[t, b])
            want = np.array([[REF.filter_run(window, np.ascontiguousarray(np.array(fed[b])[:, k]))[-1] for k in range(6)] for b in range(m)])
            assert np.array_equal(np.c_[out["imu_acc"][:m], out["imu_ang_vel"][:m]], want), t
            assert all(np.isnan(v[m:]).all() for v in out.values())
        # a changed window: refused before any launch, named; the state goes on as if the call had not been made
        other = eng.sensor_config(window + 1)
        d = [T(q), T(seq[0, :, :3]), T(seq[0, :, 3:])]; o = _poisoned(torch, dev, n, SENSOR_OUT)
        torch.cuda.synchronize()
        rc = eng.lib.a1mpc_sensor_frontend_batch_device(eng._h, C.byref(other), n, *[C.c_void_p(x.data_ptr()) for x in d + list(o.values())], None)
        assert rc == INVALID and b"imu_window" in eng.lib.a1mpc_last_error()
        torch.cuda.synchronize()
        assert all(torch.isnan(v).all() for v in o.values())
        out = _sensor_device(torch, dev, T, eng, q, seq[0, :, :3], seq[0, :, 3:], n, cfg=cfg)
        for b in range(n):
            fed[b].append(seq[0, b])
        want = np.array([[REF.filter_run(window, np.ascontiguousarray(np.array(fed[b])[:, k]))[-1] for k in range(6)] for b in range(n)])
        assert np.array_equal(np.c_[out["imu_acc"][:n], out["imu_ang_vel"][:n]], want)
        eng.reset_sensor_state()
        out = _sensor_device(torch, dev, T, eng, q, seq[1, :, :3], seq[1, :, 3:], n, cfg=other)
        assert np.array_equal(np.c_[out["imu_acc"][:n], out["imu_ang_vel"][:n]], seq[1] / float(window + 1))   # a first sample: (0 + x + 0) / window, exactly


# ---------------------------------------------------------------------------------------------------------------- the command stage
def _command_device(torch, dev, T, eng, state_d, cmd, toggle, root_pos, dt, n, stream=None):
    out = dict(root_lin_vel_d=torch.full((n + TAIL, 3), float("nan"), dtype=torch.float64, device=dev),
               root_ang_vel_d=torch.full((n + TAIL, 3), float("nan"), dtype=torch.float64, device=dev),
               movement_mode=torch.full((n + TAIL,), 255, dtype=torch.uint8, device=dev), mpc_active=torch.full((n + TAIL,), 255, dtype=torch.uint8, device=dev),
               root_pos_d_z=torch.full((n + TAIL,), float("nan"), dtype=torch.float64, device=dev))
    d = [T(cmd), T(toggle), T(root_pos)]
    torch.cuda.synchronize()
    eng.command_device(n, *d, dt, *[state_d[k] for k in FR.STATE_KEYS], *[out[k] for k in FR.OUT_KEYS], stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _padded_state(torch, dev, n):
    """the command state on the device, TAIL poisoned rows behind the n robots' (NaN / 255 / -1)"""
    st = FR.initial_state(n); out = {}
    for k, v in st.items():
        pad = np.full((TAIL,) + v.shape[1:], np.nan if v.dtype == np.float64 else (255 if v.dtype == np.uint8 else -1), dtype=v.dtype)
        out[k] = torch.from_numpy(np.concatenate([v, pad])).to(dev)
    return out


@pytest.mark.parametrize("n", FR.SIZES)
def test_command_stage_equals_the_restatement_on_every_tick(pkg, scen, n):
    """the 16-tick scripts of tests/frontend_ref.command_script (eight scripts interleaved lane by lane: the lanes of a wavefront diverge at every branch) through the
    _device entry and, on a second handle, the host entry: every in/out and output array equals the restatement of S/GazeboA1ROS.cpp:124-188 on every tick, and the two
    entries each other; the poisoned rows behind n stay as they were"""
    torch, dev, T = _dev()
    dt = 0.0025
    cmd, toggle, root_pos = FR.command_script(np.random.default_rng(31 + n), n, dt)
    want, host = FR.initial_state(n), FR.initial_state(n)
    seen = dict(modes=set(), kp=set(), active=[], heights=set())
    with pkg.Engine(_cfg(pkg, scen), 512, 0) as eng, pkg.Engine(_cfg(pkg, scen), 512, 0) as e_host:
        assert all(np.array_equal(v, want[k]) for k, v in eng.command_state(n).items())
        sd = _padded_state(torch, dev, n)
        st = torch.cuda.Stream(device=dev)
        for t in range(FR.TICKS):
            o_want = FR.command_step(want, cmd[t], toggle[t], root_pos[t], dt)
            o_dev = _command_device(torch, dev, T, eng, sd, cmd[t], toggle[t], root_pos[t], dt, n, stream=st.cuda_stream if t % 2 else None)
            o_host = e_host.command(cmd[t], toggle[t], root_pos[t], dt, host)
            for k in FR.STATE_KEYS:
                got = sd[k].cpu().numpy()
                assert np.array_equal(got[:n], want[k]) and np.array_equal(host[k], want[k]), (t, k)
                tail = got[n:]
                assert np.isnan(tail).all() if tail.dtype == np.float64 else (tail == (255 if tail.dtype == np.uint8 else -1)).all(), (t, k)
            for k in FR.OUT_KEYS:
                assert np.array_equal(o_dev[k][:n], o_want[k]) and np.array_equal(o_host[k], o_want[k]), (t, k)
                tail = o_dev[k][n:]
                assert (tail == 255).all() if tail.dtype == np.uint8 else np.isnan(tail).all(), (t, k)
            seen["modes"] |= set(o_want["movement_mode"]); seen["kp"] |= {tuple(r) for r in want["kp_linear_xy"]}; seen["active"].append(int(o_want["mpc_active"][0]))
            seen["heights"] |= set(want["body_height"])
    assert seen["active"] == [0] * 9 + [1] * 7                                     # mpc_active turns on at the tenth tick
    if n >= 8:
        assert seen["modes"] == {0, 1} and seen["kp"] == {(0.0, 0.0), (120.0, 120.0)} and {0.1, 0.32} < seen["heights"]


def test_speed_threshold_decisions_are_numpys_on_the_device(pkg, scen):
    """(0.05, 0), (0.03, 0.04) and their neighbours one ulp either side, walking: kp_linear_xy is zeroed and the xy target refreshed exactly where numpy's correctly
    rounded sqrt(vx * vx + vy * vy) > 0.05 says"""
    n = len(FR.SPEEDS)
    cmd = np.zeros((n, 6)); cmd[:, :2] = FR.SPEEDS
    with pkg.Engine(_cfg(pkg, scen), 512, 0) as eng:
        st = eng.command_state(n); st["ctrl_state"][:] = 1
        eng.command(cmd, np.zeros(n, np.uint8), np.ones((n, 3)), 0.0025, st)
    above = np.sqrt(cmd[:, 0] * cmd[:, 0] + cmd[:, 1] * cmd[:, 1]) > 0.05
    assert np.array_equal(st["kp_linear_xy"][:, 0] == 0.0, above) and np.array_equal(st["root_pos_d"][:, 0] == 1.0, above) and above.any() and (~above).any()
    assert not above[0] and above[1] and not above[2]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_live_handle(pkg, scen):
    """every refusal of include/a1mpc.h with its message, none of which touches an output: a null config or array (each in turn, named), a window out of range, a
    non-finite config value or dt, body_height_min > max, n < 0, n > max_batch; n == 0 is OK and launches nothing"""
    torch, dev, T = _dev()
    with pkg.Engine(_cfg(pkg, scen), 8, 0) as eng:
        lib, h = eng.lib, eng._h
        err = lambda: lib.a1mpc_last_error()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        f64 = lambda w: torch.full((8, w), float("nan"), dtype=torch.float64, device=dev)
        u8 = lambda: torch.full((8,), 255, dtype=torch.uint8, device=dev)
        # ---- sensor stage
        sc = eng.sensor_config()
        s_t = [f64(4), f64(3), f64(3)] + [f64(w) for _, w in SENSOR_OUT]
        s_names = ["quat", "imu_acc_raw", "imu_gyro_raw", "R_world", "R_z", "root_euler", "imu_acc", "imu_ang_vel", "root_ang_vel"]
        full = [ptr(t) for t in s_t]
        for k, name in enumerate(s_names):
            a = list(full); a[k] = None
            assert lib.a1mpc_sensor_frontend_batch_device(h, C.byref(sc), 4, *a, None) == INVALID and ("null " + name).encode() in err(), name
        assert lib.a1mpc_sensor_frontend_batch_device(h, None, 4, *full, None) == INVALID and b"a1mpc_sensor_config" in err()
        for w in (0, -3, 65):
            assert lib.a1mpc_sensor_frontend_batch_device(h, C.byref(eng.sensor_config(w)), 4, *full, None) == INVALID and b"imu_window" in err(), w
        assert lib.a1mpc_sensor_frontend_batch_device(h, C.byref(sc), -1, *full, None) == INVALID and b"negative n" in err()
        assert lib.a1mpc_sensor_frontend_batch_device(h, C.byref(sc), 9, *full, None) == TOO_LARGE and b"max_batch" in err()
        assert lib.a1mpc_sensor_frontend_batch_device(h, C.byref(sc), 0, *full, None) == OK
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        hs = [np.zeros((9, 4)), np.zeros((9, 3)), np.zeros((9, 3))] + [np.zeros((9, w)) for _, w in SENSOR_OUT]
        assert lib.a1mpc_sensor_frontend_batch(h, C.byref(sc), 9, *[dp(a) for a in hs]) == TOO_LARGE
        assert lib.a1mpc_sensor_frontend_batch(h, C.byref(sc), 4, dp(hs[0]), None, *[dp(a) for a in hs[2:]]) == INVALID and b"imu_acc_raw" in err()
        # ---- command stage
        cc = eng.command_config()
        c_t = [f64(6), u8(), f64(3), f64(1), u8(), f64(3), f64(3), f64(2), torch.full((8,), -1, dtype=torch.int32, device=dev), f64(3), f64(3), u8(), u8(), f64(1)]
        c_names = ["cmd", "mode_toggle", "root_pos", "body_height", "ctrl_state", "root_euler_d", "root_pos_d", "kp_linear_xy", "mpc_init_counter", "root_lin_vel_d",
                   "root_ang_vel_d", "movement_mode", "mpc_active", "root_pos_d_z"]
        call = lambda cfg, n, ps, dt=0.0025: lib.a1mpc_command_batch_device(h, cfg, n, *ps[:3], dt, *ps[3:], None)
        cfull = [ptr(t) for t in c_t]
        for k, name in enumerate(c_names):
            a = list(cfull); a[k] = None
            assert call(C.byref(cc), 4, a) == INVALID and ("null " + name).encode() in err(), name
        assert call(None, 4, cfull) == INVALID and b"a1mpc_command_config" in err()
        for field in ("body_height_max", "body_height_min", "kp_linear_lock_x", "kp_linear_lock_y", "lock_speed"):
            for bad in (np.nan, np.inf):
                assert call(C.byref(eng.command_config(**{field: bad})), 4, cfull) == INVALID and b"non-finite" in err(), field
        assert call(C.byref(eng.command_config(body_height_min=0.4)), 4, cfull) == INVALID and b"body_height_min > body_height_max" in err()
        assert call(C.byref(cc), 4, cfull, dt=float("nan")) == INVALID and b"dt" in err()
        assert call(C.byref(cc), -1, cfull) == INVALID and b"negative n" in err()
        assert call(C.byref(cc), 9, cfull) == TOO_LARGE and b"max_batch" in err()
        assert call(C.byref(cc), 0, cfull) == OK
        # ---- the per-robot wrench: a null kp_linear_xy, and the batch-wide entry's refusals
        g = eng.balance_gains()
        w_t = [f64(2)] + [f64(3) for _ in range(8)] + [f64(9), f64(6)]
        wfull = [ptr(t) for t in w_t]
        for k, name in enumerate(["kp_linear_xy"] + list(BC.WRENCH_KEYS) + ["R_world", "root_acc_out"]):
            a = list(wfull); a[k] = None
            assert lib.a1mpc_balance_wrench_kp_batch_device(h, C.byref(g), 4, *a, None) == INVALID and ("null " + name).encode() in err(), name
        assert lib.a1mpc_balance_wrench_kp_batch_device(h, None, 4, *wfull, None) == INVALID and b"a1mpc_balance_gains" in err()
        assert lib.a1mpc_balance_wrench_kp_batch_device(h, C.byref(g), -1, *wfull, None) == INVALID
        assert lib.a1mpc_balance_wrench_kp_batch_device(h, C.byref(g), 9, *wfull, None) == TOO_LARGE and b"max_batch" in err()
        assert lib.a1mpc_balance_wrench_kp_batch_device(h, C.byref(g), 0, *wfull, None) == OK
        # ---- the tick from raw inputs: its own null struct, and the stages' refusals through it
        E = pkg.engine
        prm = E.TickParams(); lib.a1mpc_default_tick_params(C.byref(prm))
        ts = E.TickSensors(); bf = E.TickBuffers()
        assert lib.a1mpc_control_tick_sensors_device(h, C.byref(prm), None, C.byref(bf), 4, None) == INVALID and b"sensors" in err()
        lib.a1mpc_default_sensor_config(C.byref(ts.sensor)); lib.a1mpc_default_command_config(C.byref(ts.command))
        assert lib.a1mpc_control_tick_sensors_device(h, C.byref(prm), C.byref(ts), C.byref(bf), 4, None) == INVALID and b"null quat" in err()
        ts.sensor.imu_window = 0
        assert lib.a1mpc_control_tick_sensors_device(h, C.byref(prm), C.byref(ts), C.byref(bf), 4, None) == INVALID and b"imu_window" in err()
        torch.cuda.synchronize()
        for t in s_t[3:] + [c_t[3]] + c_t[5:8] + c_t[9:11] + [c_t[13]] + [w_t[-1]]:
            assert torch.isnan(t).all()
        assert (c_t[4] == 255).all() and (c_t[11] == 255).all() and (c_t[12] == 255).all() and (c_t[8] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- one call against the chain
FRONT_F64 = dict(R_world=9, R_z=9, root_euler=3, root_ang_vel=3, imu_acc=3, imu_ang_vel=3, root_lin_vel_d=3, root_ang_vel_d=3, root_pos_d_z=1)   # + movement_mode, mpc_active:
FRONT_U8 = ("movement_mode", "mpc_active")                                                                                                      # the eleven produced fields
RAW_KEYS = ("joint_pos", "joint_vel", "foot_force", "gait_counter_speed", "torques_gravity")


def _quat_of_euler(eul):
    """zyx euler angles (n, 3) -> unit quaternions (n, 4) as w, x, y, z"""
    cr, sr, cp, sp, cy, sy = np.cos(eul[:, 0] / 2), np.sin(eul[:, 0] / 2), np.cos(eul[:, 1] / 2), np.sin(eul[:, 1] / 2), np.cos(eul[:, 2] / 2), np.sin(eul[:, 2] / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=1)


def _front_world(torch, dev, n):
    """a world's storage for the eleven produced fields (poisoned: the front end must write every one before the tick reads it) and its command state"""
    w = {k: torch.full((n, m) if m > 1 else (n,), float("nan"), dtype=torch.float64, device=dev) for k, m in FRONT_F64.items()}
    w.update({k: torch.full((n,), 255, dtype=torch.uint8, device=dev) for k in FRONT_U8})
    cs = {k: torch.from_numpy(v).to(dev) for k, v in FR.initial_state(n).items() if k != "root_euler_d"}   # (root_euler_d is the tick world's)
    return w, cs


@pytest.mark.parametrize("n,ticks", [(65, 12), (1, 1)])
def test_tick_from_raw_inputs_in_one_call_equals_the_three_entries_chained(pkg, scen, n, ticks):
    """a1mpc_control_tick_sensors_device on one handle against a1mpc_sensor_frontend_batch_device, a1mpc_command_batch_device and a1mpc_control_tick_device called by
    hand on a second one, from raw inputs (quaternion, raw IMU, stick command), the mode toggled on at tick 3 (and off again at tick 9 in the odd lanes), mpc_active
    turning on at tick 10: every field of a1mpc_tick_buffers, every command-state array, iters and status equal on every tick (NaN-aware)"""
    torch, dev, T = _dev()
    rng = np.random.default_rng(2024 + n)
    E = pkg.engine
    cfg = _cfg(pkg, scen, 10, warm_start=1)
    with pkg.Engine(cfg, 512, 0) as e1, pkg.Engine(cfg, 512, 0) as e3:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        worlds = [tick_world(n, dev, [0.0, 120.0, 120.0, 0.0]) for _ in range(2)]
        fronts = [_front_world(torch, dev, n) for _ in range(2)]
        modes = []
        for t in range(ticks):
            raw = tick_inputs(scen, rng, n)
            eul = raw["root_euler"]
            quat = _quat_of_euler(eul)
            cmd = np.c_[rng.uniform(-0.4, 0.4, (n, 2)), rng.normal(0, 0.02, n), rng.normal(0, 0.05, (n, 2)), rng.uniform(-0.4, 0.4, n)]
            cmd[::5, :2] = 0.01                                   # below lock_speed: these robots lock
            toggle = np.zeros(n, np.uint8)
            if t == 3: toggle[:] = 1
            if t == 9: toggle[1::2] = 1
            d = dict(quat=T(quat), imu_acc_raw=T(raw["imu_acc"]), imu_gyro_raw=T(raw["imu_ang_vel"]), cmd=T(cmd), mode_toggle=T(toggle))
            inp = {k: T(raw[k]) for k in RAW_KEYS}
            torch.cuda.synchronize()
            # ---- one call
            (f1, c1), w1 = fronts[0], worlds[0]
            ts = e1.tick_sensors(**d, **c1)
            e1.control_tick_sensors_device(prm, ts, tick_buffers(E, {**inp, **f1}, w1), n)
            # ---- the three entries by hand
            (f3, c3), w3 = fronts[1], worlds[1]
            e3.sensor_frontend_device(n, d["quat"], d["imu_acc_raw"], d["imu_gyro_raw"], f3["R_world"], f3["R_z"], f3["root_euler"], f3["imu_acc"], f3["imu_ang_vel"], f3["root_ang_vel"])
            e3.command_device(n, d["cmd"], d["mode_toggle"], w3["state"]["root_pos"], prm.control_dt, c3["body_height"], c3["ctrl_state"], w3["state"]["root_euler_d"],
                              c3["root_pos_d"], c3["kp_linear_xy"], c3["mpc_init_counter"], f3["root_lin_vel_d"], f3["root_ang_vel_d"], f3["movement_mode"], f3["mpc_active"],
                              f3["root_pos_d_z"])
            e3.control_tick_device(prm, tick_buffers(E, {**inp, **f3}, w3), n)
            torch.cuda.synchronize()
            for grp in ("state", "outs", "u8", "i32"):
                for k in w1[grp]:
                    a, b = w1[grp][k].cpu().numpy(), w3[grp][k].cpu().numpy()
                    assert np.array_equal(a, b, equal_nan=True), (t, k)
            for k in list(f1) + list(c1):
                a, b = (f1.get(k, c1.get(k))).cpu().numpy(), (f3.get(k, c3.get(k))).cpu().numpy()
                assert np.array_equal(a, b, equal_nan=True), (t, k)
                assert not np.isnan(a.astype(float)).any(), (t, k)          # the front end wrote every produced field
            # independent anchors: the attitude is the restatement's, the mode follows the toggles, the gate opens at the tenth tick
            assert np.array_equal(f1["R_world"].cpu().numpy(), FR.quat_to_rotation(quat))
            want_mode = np.zeros(n, np.uint8) if t < 3 else np.ones(n, np.uint8)
            if t >= 9: want_mode[1::2] = 0
            assert np.array_equal(f1["movement_mode"].cpu().numpy(), want_mode) and (f1["mpc_active"].cpu().numpy() == (1 if t >= 9 else 0)).all(), t
            modes.append(int(want_mode.sum()))
        if ticks > 9:
            assert modes[2] == 0 and modes[3] == n and 0 < modes[9] < n


# ---------------------------------------------------------------------------------------------------------------- the wrench with per-robot kp
@pytest.mark.parametrize("n", BC.WRENCH_SIZES)
def test_wrench_with_per_robot_kp(pkg, oracle, scen, n):
    """a1mpc_balance_wrench_kp_batch(_device): rows that repeat the gains' kp_linear[0:2] give the batch-wide entry's bits; mixed rows (0 and the lock values, what the
    command stage writes) give the oracle's answer to each robot's own gains; 19 poisoned rows behind the device output"""
    torch, dev, T = _dev()
    cfg = _cfg(pkg, scen)
    inp = BC.wrench_inputs(scen, np.random.default_rng(40 + n), n)
    arrs = [inp[k] for k in BC.WRENCH_KEYS] + [inp["R"]]
    with pkg.Engine(cfg, 512, 0) as eng:
        def device(kp, gains):
            d = [T(kp)] + [T(a) for a in arrs]
            out = torch.full((n + 19, 6), float("nan"), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            eng.balance_wrench_kp_device(n, *d, out, gains=gains)
            torch.cuda.synchronize()
            return out.cpu().numpy()
        for name, gd in (("default", BC.DEFAULT_GAINS), ("mixed", BC.MIXED_GAINS)):
            gains = eng.balance_gains(**gd)
            plain = eng.balance_wrench(*arrs, gains=gains)
            same = np.tile(gd["kp_linear"][:2], (n, 1))
            got = device(same, gains)
            assert np.array_equal(got[:n], plain, equal_nan=True) and np.isnan(got[n:]).all(), name
            assert np.array_equal(eng.balance_wrench_kp(same, *arrs, gains=gains), plain, equal_nan=True), name
            rows = np.where((np.arange(n) % 3 == 0)[:, None], 0.0, 120.0) * np.ones((n, 2)); rows[1::4, 1] = 0.0
            ref = np.full((n + 19, 6), np.nan)
            for b in range(n):
                g_b = dict(gd, kp_linear=(rows[b, 0], rows[b, 1], gd["kp_linear"][2]))
                ref[b] = BC.oracle_wrench(oracle, g_b, {k: v[b:b + 1] for k, v in inp.items()}, float(cfg.mass))[0]
            BC.assert_wrench_equals_oracle(device(rows, gains), ref, inp, (n, name, "device"))
            BC.assert_wrench_equals_oracle(eng.balance_wrench_kp(rows, *arrs, gains=gains), ref[:n], inp, (n, name, "host"))
