"""CPU: the ground tests/test_gpu_balance_constants.py stands on -- the balance QP (compute_grf's stance branch, S/A1RobotControl.cpp:377-444) OFF the reference's constants.
The reference keeps Q, R, mu, F_min and F_max private, so tests/test_ref_pin.py pins the balance branch at the defaults only; off them the yardstick is the oracle, anchored
here by the independent numpy formation (ref_numpy.balance_qp), the KKT conditions of its tight-mode solutions and its own extended-precision build (tests/x87.py).

1. formation and KKT on balance_common.GENERIC_BALANCE and every BALANCE_EDGE_CONSTANTS entry, the bars of test_oracle.py::test_balance_formation_and_kkt;
2. the oracle against x87 on every (constants, settings, batch) the GPU file solves: the same iteration count and status on every QP and NO QP further apart than
   TOL_FORCE_BALANCE_N -- the caps of balance_held_to_oracle are never needed by the yardstick itself;
3. max_iter = 30 gives MAX_ITER_REACHED, SOLVED_INACCURATE and SOLVED on both constant sets;
4. every balance_variants() entry moves the oracle's forces by more than 100 x TOL_FORCE_BALANCE_N on at least half of each batch, under every settings case;
5. the solver text on host fibers (tests/emu) against the oracle at the generic and the edge constants."""
import numpy as np
import pytest

import balance_common as BC
import emu
import ref_numpy as RN
from gpu_common import assert_all_three_outcomes, case_id
from helpers import TOL_FORCE_BALANCE_N

CASES = BC.balance_settings_cases()
CONSTANTS = dict(default=BC.DEFAULT_BALANCE, generic=BC.GENERIC_BALANCE)
_id = lambda c: case_id(c) or "default"


def test_the_sets_are_what_they_say():
    """the generic set has no two equal weights, a positive lower bound and an upper bound below the default's; every variant and every edge set differs from it in exactly
    the property it names; the nine variants are the ones the sensitivity check counts"""
    G = BC.GENERIC_BALANCE
    assert len(set(G["Q"])) == 6 and G["F_min"] > 0 and G["F_max"] < BC.DEFAULT_BALANCE["F_max"] and all(G[k] != BC.DEFAULT_BALANCE[k] for k in G)
    V = BC.balance_variants()
    assert len(V) == 9 and len(BC.BALANCE_EDGE_CONSTANTS) == 5
    for name, var in list(V.items()) + list(BC.BALANCE_EDGE_CONSTANTS.items()):
        assert [k for k in G if var[k] != G[k]] in (["Q"], ["R"], ["mu"], ["F_min"], ["F_max"], ["F_min", "F_max"]), name
    assert sorted(V["force and torque triples exchanged"]["Q"]) == sorted(G["Q"]) and all(sorted(v["Q"]) == sorted(G["Q"]) for v in V.values())


def test_the_batch_holds_every_contact_pattern(scen):
    """balance_batch: the first half all-stance, robot b of the second half pattern b % 16 -- all sixteen, all-swing among them; balance_random itself is unchanged"""
    for n, seed in (BC.BATCH_MAIN, BC.BATCH_EDGES, (64, 4245)):
        sc = BC.balance_batch(scen, n, seed); raw = scen.balance_random(n, seed=seed)
        code = (sc["contact"] * (1 << np.arange(4))).sum(1)
        assert (code[: n // 2] == 15).all() and np.array_equal(code[n // 2:], np.arange(n // 2, n) % 16) and set(code.tolist()) == set(range(16))
        assert all(np.array_equal(sc[k], raw[k]) for k in BC.BALANCE_INPUTS if k != "contact") and raw["contact"].any(1).all()


# ------------------------------------------------------------------------------------------------ 1. formation and KKT
@pytest.mark.parametrize("name", ["generic"] + list(BC.BALANCE_EDGE_CONSTANTS))
def test_formation_and_kkt(oracle, scen, name):
    """64 QPs with every contact pattern: the oracle's P, g, A, l, u against ref_numpy.balance_qp with the same constants, and the exact-mode solution a KKT point of the numpy
    matrices (test_oracle.py::test_balance_formation_and_kkt's bars)"""
    c = BC.GENERIC_BALANCE if name == "generic" else BC.BALANCE_EDGE_CONSTANTS[name]
    sc = BC.balance_batch(scen, 64, 4245)
    qp = BC.oracle_qp(oracle, c)
    worst = np.zeros(5)
    for b in range(64):
        P, g, A, l, u, _ = oracle.balance_form(qp, sc["root_acc"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
        P2, g2, A2, l2, u2 = RN.balance_qp(sc["root_acc"][b], sc["Rz"][b].reshape(3, 3), sc["foot"][b].reshape(4, 3), sc["contact"][b], Qw=c["Q"], Rw=c["R"], mu=c["mu"],
                                           Fmin=c["F_min"], Fmax=c["F_max"])
        r = oracle.balance_solve(qp, oracle.exact_settings(), sc["root_acc"][b], sc["R"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
        stat, viol, wrong = RN.kkt_violation(P2, g2, A2, l2, u2, r["f_world"], tol_active=1e-6)
        worst = np.maximum(worst, [np.abs(P - P2).max(), np.abs(g - g2).max(), stat, viol, wrong])
        assert np.abs(P - P2).max() < 1e-10 and np.abs(g - g2).max() < 1e-8 and (A == A2).all() and (l == l2).all() and (u == u2).all(), b
        assert stat < 1e-5 and viol < 1e-7 and wrong < 1e-5, (b, stat, viol, wrong)
    print(f"{name}: worst |dP| {worst[0]:.1e}, |dg| {worst[1]:.1e}, stationarity {worst[2]:.1e}, violation {worst[3]:.1e}")


# ------------------------------------------------------------------------------------------------ 2. the yardstick alone, on the GPU file's batches
@pytest.mark.parametrize("cname", list(CONSTANTS))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_and_x87_agree_under_every_settings_case(oracle, scen, case, cname):
    """the 256-QP batch of the GPU file's settings tests"""
    sc = BC.balance_batch(scen, *BC.BATCH_MAIN)
    ref = BC.oracle_balance(oracle, CONSTANTS[cname], oracle.default_settings(**case), sc)
    BC.balance_yardstick_alone(f"{cname} constants", ref, BC.x87_balance(CONSTANTS[cname], case, sc), case)


@pytest.mark.parametrize("name", list(BC.BALANCE_EDGE_CONSTANTS))
def test_oracle_and_x87_agree_on_the_edge_constants(oracle, scen, name):
    """every QP SOLVED at every edge set; the all-swing rows come back (near) zero"""
    sc = BC.balance_batch(scen, *BC.BATCH_MAIN)
    c = BC.BALANCE_EDGE_CONSTANTS[name]
    ref = BC.oracle_balance(oracle, c, oracle.default_settings(), sc)
    BC.balance_yardstick_alone(name, ref, BC.x87_balance(c, {}, sc), {})
    swing = ~sc["contact"].any(1)
    print(f"{name}: all-swing rows {int(swing.sum())}, their largest |f| {np.abs(ref['grf'][swing]).max():.1e} N")
    assert (ref["status"] == 1).all() and swing.sum() >= 8 and np.abs(ref["grf"][swing]).max() < TOL_FORCE_BALANCE_N


@pytest.mark.parametrize("batch,cname", [(BC.BATCH_SMALL, "generic"), (BC.BATCH_EDGES, "generic"), (BC.BATCH_EDGES, "default")], ids=str)
def test_oracle_and_x87_agree_on_the_other_batches(oracle, scen, batch, cname):
    """the small-batch rows of the host entry's test and the batch the device entry's sizes are cut from (its two-stream call solves it at both constant sets)"""
    sc = BC.balance_batch(scen, *batch)
    ref = BC.oracle_balance(oracle, CONSTANTS[cname], oracle.default_settings(), sc)
    BC.balance_yardstick_alone(f"{cname} constants", ref, BC.x87_balance(CONSTANTS[cname], {}, sc), {})


# ------------------------------------------------------------------------------------------------ 3. the three outcomes at max_iter = 30
@pytest.mark.parametrize("cname", list(CONSTANTS))
def test_max_iter_30_gives_all_three_outcomes(oracle, scen, cname):
    sc = BC.balance_batch(scen, *BC.BATCH_MAIN)
    ref = BC.oracle_balance(oracle, CONSTANTS[cname], oracle.default_settings(max_iter=30), sc)
    print(cname, "oracle statuses at max_iter = 30:", assert_all_three_outcomes(ref["status"]))


# ------------------------------------------------------------------------------------------------ 4. sensitivity
@pytest.mark.parametrize("case", [{}] + [c for c in CASES if c != dict(max_iter=30)], ids=_id)
def test_every_variant_moves_the_oracles_forces(oracle, scen, case):
    """the 256-QP batch under the default settings (the precondition the GPU file re-asserts on each of its batches) and under every settings case that lets the solve
    converge"""
    BC.assert_balance_variants_move(oracle, BC.balance_batch(scen, *BC.BATCH_MAIN), oracle.default_settings(**case), label=_id(case))


def test_after_30_iterations_seven_variants_have_moved_the_iterate(oracle, scen):
    """max_iter = 30 returns an iterate, not an optimum: it has not yet felt R (a 3e-3 / 1e-3 diagonal beside weights of 0.7 .. 520) nor the upper bound (the iterate of most
    QPs has not reached 50 N) -- the oracle moves on 26 % and 21 % of the batch for those two -- but the seven other variants each move it on more than 95 %.  The
    max_iter = 30 cases of the GPU file are therefore sensitive to the weight order, mu and F_min; R and F_max are held by the fifteen converging cases"""
    names = [k for k in BC.balance_variants() if k not in ("R -> 1e-3", "F_max 50 -> 60")]
    BC.assert_balance_variants_move(oracle, BC.balance_batch(scen, *BC.BATCH_MAIN), oracle.default_settings(max_iter=30), label="max_iter=30", names=names)


@pytest.mark.parametrize("batch", [BC.BATCH_SMALL, BC.BATCH_EDGES], ids=str)
def test_every_variant_moves_the_oracles_forces_on_the_other_batches(oracle, scen, batch):
    BC.assert_balance_variants_move(oracle, BC.balance_batch(scen, *batch))


# ------------------------------------------------------------------------------------------------ 5. the solver text on host fibers
_EMU_NAMES = dict(scaling="scaling_iters", check_termination="check_every", adaptive_rho_interval="adaptive_rho_every", rho="rho0", adaptive_rho_tolerance="adaptive_rho_tol")


def _emulated(oracle, scen, c, case, label):
    sc = BC.balance_batch(scen, 64, 4245)
    out = emu.balance_solve(sc, qp=c, **{_EMU_NAMES.get(k, k): v for k, v in case.items()})
    ref = BC.oracle_balance(oracle, c, oracle.default_settings(**case), sc)
    d = np.maximum(np.abs(out["grf"] - ref["grf"]).max(1), np.abs(out["f_world"] - ref["f_world"]).max(1))
    print(f"{label} {_id(case)}: 64 QPs on host fibers, worst force distance to the oracle {d.max():.2e} N, statuses {dict(zip(*np.unique(ref['status'], return_counts=True)))}")
    assert np.array_equal(out["iters"], ref["iters"]) and np.array_equal(out["status"], ref["status"]), np.flatnonzero(out["iters"] != ref["iters"])[:8]
    assert (d <= TOL_FORCE_BALANCE_N).all(), float(d.max())
    return ref


@pytest.mark.parametrize("case", [{}, dict(scaling=0), dict(max_iter=30), dict(check_termination=10, adaptive_rho_interval=35)], ids=_id)
def test_emulated_balance_qp_at_the_generic_constants(oracle, scen, case):
    """a1mpc_solver.hpp's H = 1 rows compiled for the host, handed emu.balance_params(GENERIC_BALANCE): formation, gradient, bounds and the failure statuses of the kernel
    TEXT against the oracle -- same iteration count and status, forces within TOL_FORCE_BALANCE_N.  The torque-first order of q2 is written out a second time in
    emu.balance_params, so this does NOT cover the library's own argument fill (balance_kernel_args); only tests/test_gpu_balance_constants.py does."""
    ref = _emulated(oracle, scen, BC.GENERIC_BALANCE, case, "generic")
    if case.get("max_iter") == 30:
        assert (ref["status"] == -2).any() and (ref["status"] == 1).any()     # (64 QPs: the failure status and SOLVED both occur; all three on the 256-QP batch above)


@pytest.mark.parametrize("name", list(BC.BALANCE_EDGE_CONSTANTS))
def test_emulated_balance_qp_at_the_edge_constants(oracle, scen, name):
    """the same at the edge sets under the default settings (not the argument fill either)"""
    _emulated(oracle, scen, BC.BALANCE_EDGE_CONSTANTS[name], {}, name)
