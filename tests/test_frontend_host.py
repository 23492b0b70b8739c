"""The sensor / command front end on the CPU: the product's kernel text compiled for the host (tests/emu/frontend_host.py, -ffp-contract=off) against the reference --
Utils::quat_to_euler and MovingWindowFilter::CalculateAverage of the reference's own compiled code (oracle/_ref), and the numpy restatement of the two rotation matrices
and of main_update's first half (tests/frontend_ref.py).  Everything is np.array_equal: the kernels use IEEE operations in the reference's order, and on the host the
four libm calls are the reference's too.  tests/test_gpu_sensor_frontend.py runs the same rows through the C ABI on the GPU."""
import os, sys
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import frontend_host as host
import frontend_ref as FR
import ref as REF

pytestmark = pytest.mark.skipif(not REF.build(), reason="oracle/_ref not built and the reference's sources absent")

CALLS = 12   # the fill phase, the first full window, two wrap-arounds of window 5


@pytest.mark.parametrize("n", FR.SIZES)
def test_sensor_kernel_text_equals_the_reference(n):
    """identity, w < 0, a non-unit quaternion, both gimbal-lock poles beyond the clamp, a NaN row, random rows; 12 calls of IMU samples from 1e-8 to 1e8 with alternating
    signs; 7 NaN-poisoned rows beyond n stay NaN"""
    rng = np.random.default_rng(100 + n)
    q = FR.quaternion_rows(rng, n); FR.assert_special_rows_are_special(q)
    seq = FR.imu_sequence(rng, CALLS, n); FR.assert_samples_take_both_branches(seq, (1, 3, 5))
    want_f = FR.reference_filters(REF, 5, seq)
    R = FR.quat_to_rotation(q); eul = FR.reference_euler(REF, q)
    nan = np.isnan(q).any(1)
    assert not np.isnan(eul[~nan]).any() and np.isnan(eul[nan]).any(1).all()
    H = host.HostSensor(n + 40)
    for t in range(CALLS):
        out = H.run(q, seq[t, :, :3], seq[t, :, 3:], rows=n + 7)
        assert np.array_equal(out["R_world"][:n], R, equal_nan=True) and np.array_equal(np.isnan(out["R_world"][:n]).any(1), nan)
        assert np.array_equal(out["root_euler"][:n], eul, equal_nan=True), np.abs(out["root_euler"][:n] - eul).max()   # the same glibc, the same arguments: bit-equal
        FR.assert_yaw_rotation(out["R_z"][:n], eul[:, 2], 1e-15)
        assert np.array_equal(out["imu_acc"][:n], want_f[t, :, :3]) and np.array_equal(out["imu_ang_vel"][:n], want_f[t, :, 3:]), t
        assert np.array_equal(out["root_ang_vel"][:n], FR.rotate(out["R_world"][:n], out["imu_ang_vel"][:n]), equal_nan=True)
        for v in out.values():
            assert np.isnan(v[n:]).all()
    assert np.array_equal(H.cursor[0, :n], np.full(n, 5)) and not H.cursor[:, n:].any() and not H.filt[:, :, n:].any()   # the state beyond n was never touched


@pytest.mark.parametrize("window", [1, 3, 5, 8])
def test_filter_windows_resets_and_a_smaller_batch_in_between(window):
    """windows 1, 3, 5 and 8; a reset after call 7 restarts the fill phase; calls 3 and 4 run 20 of the 65 robots only, whose cursors then lead the others': every
    position keeps its own state, and the robots' cursors part"""
    rng = np.random.default_rng(7 + window); n, small = 65, 20
    q = FR.quaternion_rows(rng, n)
    seq = FR.imu_sequence(rng, CALLS, n)
    H = host.HostSensor(80, window)
    fed = [[] for _ in range(n)]    # what each robot's filters have been fed since the last reset
    for t in range(CALLS):
        if t == 7:
            H.reset(); fed = [[] for _ in range(n)]
        m = small if t in (3, 4) else n
        out = H.run(q[:m], seq[t, :m, :3], seq[t, :m, 3:])
        for b in range(m):
            fed[b].append(seq[t, b])
            want = np.array([REF.filter_run(window, np.ascontiguousarray(np.array(fed[b])[:, k]))[-1] for k in range(6)])
            assert np.array_equal(np.r_[out["imu_acc"][b], out["imu_ang_vel"][b]], want), (t, b)
        if t == 6 and window > 2:
            assert H.cursor[1, 0] != H.cursor[1, n - 1]


def test_command_kernel_text_equals_the_restatement_on_every_tick():
    """the 16-tick scripts of tests/frontend_ref.command_script, eight of them interleaved lane by lane: toggle on, walk above and below lock_speed, toggle off (the
    one-tick lock), stand; speeds on and one ulp beside the threshold; both height clamps; mpc_active from the tenth tick"""
    n = 257; dt = 0.0025
    rng = np.random.default_rng(31)
    cmd, toggle, root_pos = FR.command_script(rng, n, dt)
    got, want = FR.initial_state(n), FR.initial_state(n)
    seen = dict(modes=set(), kp=set(), locks=0, active=[], heights=set())
    for t in range(FR.TICKS):
        before = {k: v.copy() for k, v in want.items()}
        o_want = FR.command_step(want, cmd[t], toggle[t], root_pos[t], dt)
        o_got = host.command(got, cmd[t], toggle[t], root_pos[t], dt, FR.COMMAND_DEFAULTS, rows=n + 5)
        for k in FR.STATE_KEYS:
            assert np.array_equal(got[k], want[k]), (t, k)
        for k in FR.OUT_KEYS:
            assert np.array_equal(o_got[k][:n], o_want[k]), (t, k)
            tail = o_got[k][n:]
            assert (tail == 255).all() if tail.dtype == np.uint8 else np.isnan(tail).all()
        seen["modes"] |= set(o_want["movement_mode"]); seen["kp"] |= {tuple(r) for r in want["kp_linear_xy"]}
        seen["locks"] += int(((before["ctrl_state"] == 1) & (want["ctrl_state"] == 0)).sum()); seen["active"].append(int(o_want["mpc_active"][0])); seen["heights"] |= set(want["body_height"])
    # the script went where it claims to go
    assert seen["modes"] == {0, 1} and seen["kp"] == {(0.0, 0.0), (120.0, 120.0)} and seen["locks"] > 0
    assert seen["active"] == [0] * 9 + [1] * 7
    assert {0.1, 0.32} < seen["heights"]          # both clamps were reached (and sat on, ticks 7-8 of scripts 2 and 3), and left again


def test_speed_threshold_decisions_are_numpys():
    """(0.05, 0), (0.03, 0.04) and their neighbours one ulp either side, walking: kp_linear_xy is zeroed exactly where numpy's sqrt(vx * vx + vy * vy) > 0.05 says"""
    n = len(FR.SPEEDS)
    cmd = np.zeros((n, 6)); cmd[:, :2] = FR.SPEEDS
    st = FR.initial_state(n); st["ctrl_state"][:] = 1
    host.command(st, cmd, np.zeros(n, np.uint8), np.ones((n, 3)), 0.0025, FR.COMMAND_DEFAULTS)
    above = np.sqrt(cmd[:, 0] * cmd[:, 0] + cmd[:, 1] * cmd[:, 1]) > 0.05
    assert np.array_equal(st["kp_linear_xy"][:, 0] == 0.0, above) and above.any() and (~above).any()
    assert not above[0] and above[1] and not above[2]          # 0.05 itself locks, the next double does not
    assert np.array_equal(st["root_pos_d"][:, 0] == 1.0, above)


def test_heights_land_on_and_beyond_both_clamps():
    cfg = FR.COMMAND_DEFAULTS
    h0 = np.array([0.32, 0.1, 0.31, 0.11, 0.2, np.nextafter(0.32, 0), np.nextafter(0.1, 1)]); n = len(h0)
    velz = np.array([0.0, 0.0, 40.0, -40.0, 0.0, 0.0, 0.0])
    cmd = np.zeros((n, 6)); cmd[:, 2] = velz
    got, want = FR.initial_state(n), FR.initial_state(n)
    got["body_height"][:] = h0; want["body_height"][:] = h0
    o = host.command(got, cmd, np.zeros(n, np.uint8), np.zeros((n, 3)), 0.0025, cfg)
    FR.command_step(want, cmd, np.zeros(n, np.uint8), np.zeros((n, 3)), 0.0025, cfg)
    assert np.array_equal(got["body_height"], want["body_height"]) and np.array_equal(got["body_height"], [0.32, 0.1, 0.32, 0.1, 0.2, h0[5], h0[6]])
    assert np.array_equal(o["root_pos_d_z"], got["body_height"]) and np.array_equal(got["root_pos_d"][:, 2], got["body_height"])
