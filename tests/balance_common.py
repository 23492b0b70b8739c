"""Shared by the balance-QP controller's tests (tests/test_balance_wrench_host.py on the CPU, tests/test_gpu_balance_tick.py on the GPU): the PD wrench's inputs with
the rows that sit on its branches, and the oracle's answer to them (orc_balance_root_acc, pinned to the reference by tests/test_ref_pin.py)."""
import numpy as np

WRENCH_SIZES = (1, 63, 64, 65, 257)        # one lane, either side of a wavefront edge, past one 256-thread workgroup
WRAP = 3.1415926 * 1.5                      # S/A1RobotControl.cpp:328-332: the yaw error wraps beyond +-WRAP (strict comparisons)
WRENCH_KEYS = ("root_pos_d", "root_pos", "root_lin_vel_d", "root_lin_vel", "root_euler_d", "root_euler", "root_ang_vel_d", "root_ang_vel")   # the C ABI's order; then R
DEFAULT_GAINS = dict(kp_linear=(1000.0, 1000.0, 1000.0), kd_linear=(200.0, 70.0, 120.0), kp_angular=(650.0, 35.0, 1.0), kd_angular=(4.5, 4.5, 30.0))   # S/A1CtrlStates.h:117-120
ZERO_GAINS = {k: (0.0, 0.0, 0.0) for k in DEFAULT_GAINS}
MIXED_GAINS = dict(kp_linear=(1000.0, 0.0, 730.5), kd_linear=(0.0, 70.0, 120.0), kp_angular=(650.0, 35.0, 0.0), kd_angular=(4.5, 0.0, 30.0))

# yaw (euler_d[2], euler[2]) pairs of the special rows and whether the reference wraps them.  Row k of a batch takes pair k % 8 while k < 8 (n = 1 takes the first);
# in rows 2-5 the error is the mark itself or its neighbour, computed exactly (x - 0 and 0 - x are exact)
_UP, _DOWN = np.nextafter(WRAP, np.inf), np.nextafter(WRAP, 0.0)
YAW_ROWS = [(5.0, 0.0, True), (-5.0, 0.25, True), (WRAP, 0.0, False), (0.0, WRAP, False), (_UP, 0.0, True), (0.0, _UP, True), (_DOWN, 0.0, False), (3.0, -3.0, True)]


def wrench_inputs(scen, rng, n, nan_row=True):
    """dict of the nine input arrays (WRENCH_KEYS + R) for n robots: random attitudes and states; the first rows carry YAW_ROWS; row n // 2 (n >= 16) has a NaN in
    root_lin_vel -- `nan_row` -- so that NaN goes in in exactly one row"""
    eul = rng.normal(0, 0.3, (n, 3)); eul[:, 2] = rng.uniform(-3.0, 3.0, n)
    inp = dict(root_pos_d=np.array([0.0, 0.0, 0.3]) + rng.normal(0, 0.02, (n, 3)), root_pos=np.array([0.0, 0.0, 0.3]) + rng.normal(0, 0.05, (n, 3)),
               root_lin_vel_d=rng.uniform(-0.5, 0.5, (n, 3)), root_lin_vel=rng.normal(0, 0.4, (n, 3)), root_euler_d=rng.normal(0, 0.1, (n, 3)), root_euler=eul,
               root_ang_vel_d=rng.uniform(-0.5, 0.5, (n, 3)), root_ang_vel=rng.normal(0, 0.5, (n, 3)),
               R=np.ascontiguousarray(scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)))
    inp["root_euler_d"][:, 2] = eul[:, 2] + rng.normal(0, 0.2, n)
    for k, (yd, y, _) in enumerate(YAW_ROWS[:n]):
        inp["root_euler_d"][k, 2], inp["root_euler"][k, 2] = yd, y
    if nan_row and n >= 16:
        inp["root_lin_vel"][n // 2, 1] = np.nan
    return inp


def nan_rows(inp):
    return np.flatnonzero(np.any([np.isnan(v).reshape(len(v), -1).any(1) for v in inp.values()], axis=0))


def yaw_rows_take_their_branch(inp):
    """the input-side assertion: in float64 the special rows' yaw errors wrap exactly where YAW_ROWS says, and the marks themselves are hit"""
    ee = inp["root_euler_d"][:, 2] - inp["root_euler"][:, 2]
    k = min(len(ee), len(YAW_ROWS))
    assert [bool(abs(e) > WRAP) for e in ee[:k]] == [w for _, _, w in YAW_ROWS[:k]]
    if k == len(YAW_ROWS):
        assert ee[2] == WRAP and ee[3] == -WRAP


def oracle_wrench(oracle, gains, inp, mass, rows=None):
    """oracle.balance_root_acc row by row -> (n, 6); rows > n: a NaN tail is appended (what an entry must leave of a poisoned output)"""
    n = len(inp["R"])
    out = np.full((n if rows is None else rows, 6), np.nan)
    for b in range(n):
        out[b] = oracle.balance_root_acc(gains["kp_linear"], gains["kd_linear"], gains["kp_angular"], gains["kd_angular"], inp["root_pos_d"][b], inp["root_pos"][b],
                                         inp["root_lin_vel_d"][b], inp["root_lin_vel"][b], inp["root_euler_d"][b], inp["root_euler"][b], inp["root_ang_vel_d"][b],
                                         inp["root_ang_vel"][b], inp["R"][b], mass)
    return out


def assert_wrench_equals_oracle(got, ref, inp, label=""):
    """bit for bit; NaN only where the oracle has it, and the oracle has it only in the rows that were fed one"""
    n = len(inp["R"])
    bad = nan_rows(inp)
    clean = np.setdiff1d(np.arange(n), bad)
    assert not np.isnan(ref[clean]).any() and all(np.isnan(ref[b]).any() for b in bad), label
    assert np.array_equal(got[clean], ref[clean]), (label, np.argwhere(got[clean] != ref[clean])[:4])
    assert np.array_equal(got[bad], ref[bad], equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(ref)), label
    assert np.isnan(got[n:]).all(), label   # (the poisoned tail beyond n)
