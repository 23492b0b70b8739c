"""The balance controller's PD-wrench kernel on the CPU: the product's kernel text compiled for the host (tests/emu/balance_wrench_host.py) against
oracle.balance_root_acc (S/A1RobotControl.cpp:325-332, 379-391), bit for bit -- the kernel uses IEEE add, subtract and multiply only, in the oracle's order, with
contraction off, so equality is derivable and np.array_equal is the bar.  tests/test_gpu_balance_tick.py runs the same rows through the C ABI on the GPU."""
import os, sys
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import balance_wrench_host as host
import balance_common as BC

MASS = 12.0


@pytest.mark.parametrize("n", BC.WRENCH_SIZES)
def test_kernel_text_on_the_host_equals_the_oracle_bit_for_bit(oracle, scen, n):
    """one lane, either side of a wavefront edge, past one workgroup; the first rows wrap the yaw error upwards, downwards, sit exactly on either mark (no wrap: the
    comparisons are strict) and one ulp beyond; a NaN input row gives NaN in that row only; 19 NaN-poisoned rows beyond n stay NaN"""
    inp = BC.wrench_inputs(scen, np.random.default_rng(40 + n), n)
    BC.yaw_rows_take_their_branch(inp)
    for name, gains in (("default", BC.DEFAULT_GAINS), ("mixed", BC.MIXED_GAINS)):
        got = host.run(gains, MASS, inp, rows=n + 19)
        BC.assert_wrench_equals_oracle(got, BC.oracle_wrench(oracle, gains, inp, MASS, rows=n + 19), inp, (n, name))
    if n >= 16:
        assert len(BC.nan_rows(inp)) == 1 and np.isnan(got[n // 2]).any() and not np.isnan(np.delete(got[:n], n // 2, 0)).any()


def test_zero_gains_leave_the_weight_alone(oracle, scen):
    """all twelve gains zero: every row is (0, 0, m * 9.8, 0, 0, 0) -- the NaN row excepted, 0 * NaN is NaN there and there only -- and equals the oracle's"""
    n = 65
    inp = BC.wrench_inputs(scen, np.random.default_rng(7), n)
    got = host.run(BC.ZERO_GAINS, MASS, inp, rows=n + 3)
    BC.assert_wrench_equals_oracle(got, BC.oracle_wrench(oracle, BC.ZERO_GAINS, inp, MASS, rows=n + 3), inp, "zero gains")
    clean = np.setdiff1d(np.arange(n), BC.nan_rows(inp))
    assert np.array_equal(got[clean], np.tile([0.0, 0.0, MASS * 9.8, 0.0, 0.0, 0.0], (len(clean), 1)))


def test_the_yaw_wrap_moves_the_torque_by_a_turn(oracle, scen):
    """what the branch is for: with kp_angular[2] = 1 and no damping, row 0 (error 5 rad) asks for 5 - 2 * 3.1415926 and row 2 (error = the mark) for the mark itself"""
    inp = BC.wrench_inputs(scen, np.random.default_rng(3), 8, nan_row=False)
    gains = dict(BC.ZERO_GAINS, kp_angular=(0.0, 0.0, 1.0))
    got = host.run(gains, MASS, inp)
    assert got[0, 5] == 5.0 - 3.1415926 * 2 - 0.0 and got[2, 5] == BC.WRAP and got[3, 5] == -BC.WRAP
    assert got[1, 5] == -5.0 + 3.1415926 * 2 - 0.25
