"""CPU: the re-initialisation rule of the update path (warm_start = 2, a changed Hessian pattern) on the kernel text itself, run by tests/emu, against the oracle -- the
cases of tests/test_gpu_update_reinit.py at sizes the emulation affords, so the CPU suite guards the rule without a GPU: general-path changes on the fused pair, the
latency kernel and the quad of rows, the fast path's fused and split pipelines, the leg-to-leg move of a zero (class 2 of every fleet), mixed batches, path switches
with and without a change, zero weights, a failed tick -- and the condition under which the GPU file's distances mean anything: the oracle's two linear-system back
ends stay within 1e-9 N of each other on the followed robots of every sequence it runs."""
import numpy as np
import pytest

import emu
from helpers import oracle_params
from update_reinit_common import (ALL_SEQUENCES, SWITCH_PATHS, Fleet, followed, hardware, oracle_tick, plan, switch_sets, unweighted, weighted_part, zero_weight_sets)

TOL_N = 1e-8        # kernel text vs oracle: the bar tests/test_emu_parity.py holds the update path to (test_emulated_update_path_matches_oracle) ...
TOL_T_N = 1e-7      # ... and, on the ill-conditioned `test_mpc` constants (r = 1e-6), its pattern-change test on fixture T
BACK_ENDS_N = 1e-9  # the oracle's linsys = 0 vs linsys = 1 over a whole sequence on the `hardware` constants (and on its `unweighted` variant)
BACK_ENDS_T_N = 1e-6  # ... and on `test_mpc`: r = 1e-6 makes the QP ill-conditioned whatever the sequence does (the back ends are 1e-7 N apart with and without
                      # re-initialisations); the yardstick is asked to be ten times finer than the bar it serves there, helpers.TOL_FORCE_N = 1e-5 N


def _emu_chain(oracle, fl, paths, fast=None, gen=None, want=None, nan_at=None, tol=TOL_N):
    """the fleet through the emulated kernel (`fast` / `gen`: keyword arguments of emu.solve / emu.solve_gen for 'F' / 'G' ticks) and the oracle, tick by tick"""
    n, h = fl.n, fl.h
    sc = dict(horizon=h, params=fl.p)
    pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1)
    carries = [oracle.update_carry(h) for _ in range(n)]
    wx = np.zeros((n, 12 * h)); wy = np.zeros((n, 20 * h)); rho = np.zeros(n); carry = emu.carry_buffer(h, n)
    want = fl.plan(len(paths)) if want is None else want
    worst = 0.0
    for t, path in enumerate(paths):
        q = fl.tick(t, general=path == "G")
        if nan_at is not None and t == nan_at[0]:
            q["x0"][nan_at[1], 4] = np.nan
        one = dict(sc, x0=q["x0"], xref=q["xref"], R=q["R"], foot=q["foot"], contact=q["contact"])
        if path == "G":
            e = emu.solve_gen(one, q["foot"], 12, q["contact"], 0, n=n, warm=(wx, wy, rho), carry=carry, warm_start=2, **gen)
        else:
            e = emu.solve(one, n=n, warm=(wx, wy, rho), carry=carry, warm_start=2, **fast)
        res = [oracle_tick(oracle, pr, st, q, b, carries[b]) for b in range(n)]
        got = np.array([bool(o["info"].reinit) for o in res])
        assert np.array_equal(got, want[t]), (t, path, "the oracle's re-initialisations are not the planned ones", got.astype(int), want[t].astype(int))
        for b, o in enumerate(res):
            assert e["iters"][b] == o["info"].iters and e["status"][b] == o["info"].status, (t, path, b, int(e["iters"][b]), o["info"].iters, "reinit", int(got[b]))
            d = float(np.abs(e["grf"][b] - o["grf"]).max()); worst = max(worst, d)
            assert d <= tol, (t, path, b, d)
    assert carry[:, 0].min() > 0.0 or nan_at is not None
    return worst, want


@pytest.mark.parametrize("kind,h,n,off,ticks,kw", [("twin", 10, 4, 0, 7, dict(twin=True)), ("latency", 10, 4, 0, 7, dict(latency=True)), ("quad", 16, 2, 2, 5, dict(twin=True, quad=True))],
                         ids=["twin", "latency", "quad"])
def test_emulated_general_path_reinitialises_with_the_oracle(oracle, scen, kind, h, n, off, ticks, kw):
    """general -> general changes, robots of different classes in one batch: a zero from horizon step 3 on (class 1), the leg-to-leg move (class 2), the cycle of four
    patterns (class 3), next to a robot that never changes (h = 16, where an emulated tick costs 0.7 s per robot: classes 2 and 3, five ticks)"""
    fl = Fleet(scen, hardware(scen), n, h, seed=8100 + h, class_offset=off)
    worst, want = _emu_chain(oracle, fl, "G" * ticks, gen=kw)
    assert want.sum() >= 5 and (want.any(axis=1) & ~want.all(axis=1)).any()
    print(kind, h, "worst", worst)


@pytest.mark.parametrize("kind,n,off,kw", [("fused_twin", 4, 0, dict(twin=True)), ("split_twin", 4, 0, dict(split_rows=1, twin=True)), ("latency", 3, 1, dict(latency=True)),
                                            ("two_robots", 2, 2, dict(twin=True)), ("two_robots_split", 2, 3, dict(split_rows=2, twin=True))],
                         ids=["fused_twin", "split_twin", "latency", "two_robots", "two_robots_split"])
def test_emulated_fast_path_reinitialises_with_the_oracle(oracle, scen, kind, n, off, kw):
    """fast -> fast changes in mixed batches (the two-robot ones hold classes 2 + 3 and 3 + 0: the pair re-initialises on different ticks), the leg-to-leg move
    among them"""
    fl = Fleet(scen, hardware(scen), n, 10, seed=8110 + n, class_offset=off)
    _, want = _emu_chain(oracle, fl, "F" * 7, fast=kw)
    assert (want.any(axis=1) & ~want.all(axis=1)).any()       # a tick on which one robot of the batch re-initialises and another does not


def test_emulated_path_switches_compare_the_pattern_across_the_switch(oracle, scen):
    """fast -> general and general -> fast, each with a change (re-initialise) and without (stay on the update path), and a change on the tick after a switch"""
    fl = Fleet(scen, hardware(scen), 4, 10, seed=8120, zero_of=switch_sets, late=False)
    want = fl.plan(len(SWITCH_PATHS))
    sw = [t for t in range(1, len(SWITCH_PATHS)) if SWITCH_PATHS[t] != SWITCH_PATHS[t - 1]]
    for a, b in (("F", "G"), ("G", "F")):
        at = [t for t in sw if SWITCH_PATHS[t - 1] == a and SWITCH_PATHS[t] == b]
        assert any(want[t, 1:3].any() for t in at) and any((~want[t, :3]).any() for t in at), (a, b)
    assert any(want[t + 1, 1:3].any() for t in sw if t + 1 < len(SWITCH_PATHS))
    _emu_chain(oracle, fl, SWITCH_PATHS, fast=dict(twin=True), gen=dict(twin=True), want=want)


@pytest.mark.parametrize("weights", ["unweighted", "test_mpc"])
@pytest.mark.parametrize("path", ["F", "G"])
def test_emulated_reinitialisation_follows_the_weighted_pattern(oracle, scen, weights, path):
    """`unweighted` (roll, pitch and their rates carry no weight): a foot's z set to 0.0 changes flags of B~ and no stored entry of the Hessian -- no re-initialisation
    on either path; a foot's y does.  `test_mpc`: every toggle is a change."""
    p = unweighted(scen) if weights == "unweighted" else dict(scen.PARAM_SETS["test_mpc"], **scen.MPC_CONSTANTS)
    fl = Fleet(scen, p, 4, 10, seed=8300, zero_of=zero_weight_sets, late=False)
    want = plan(fl.classes, 6, weighted_part if weights == "unweighted" else zero_weight_sets)
    if weights == "unweighted":
        assert not want[:, [1, 3]].any() and want[:, 2].any()
    _emu_chain(oracle, fl, path * 6, fast=dict(twin=True), gen=dict(twin=True), want=want, tol=TOL_N if weights == "unweighted" else TOL_T_N)


def test_emulated_change_on_the_tick_after_a_failed_tick(oracle, scen):
    """tick 2 fails on robots 2 and 3 (NaN in x0: NON_CVX, zeros out).  OSQP's workspace survives a failed solve with cold iterates, so tick 3 still compares patterns:
    robot 3 re-initialises (from zero iterates), robot 2 follows the update path"""
    fl = Fleet(scen, hardware(scen), 4, 10, seed=8130)
    want = fl.plan(6)
    assert want[3, 3] and not want[3, 2]
    _emu_chain(oracle, fl, "F" * 6, fast=dict(twin=True), want=want, nan_at=(2, [2, 3]))


@pytest.mark.parametrize("seq", ALL_SEQUENCES, ids=[q.name for q in ALL_SEQUENCES])
def test_oracle_back_ends_agree_over_the_sequences_of_the_gpu_tests(oracle, scen, seq):
    """the condition the GPU file's distances rest on: through every re-initialisation of each of its sequences the oracle's two linear-system back ends (reduced
    system | LDL' of the full KKT matrix: algebraically the same solve) give the same iteration counts and forces within 1e-9 N (`test_mpc` constants: 1e-6 N), on the robots the GPU test follows
    (all of them at h <= 10; every third at h = 16 and every fifth at h = 20, where the dense KKT factor of the second back end costs 30 and 60 ms a piece)"""
    fl = seq.fleet(scen); h = seq.h
    idx = followed(seq.n, fl.classes)
    if h > 10 and len(idx) > 16:
        idx = idx[::3 if h == 16 else 5]     # (a stride coprime to the four classes)
        assert set(fl.classes[idx]) == {0, 1, 2, 3}
    sc = dict(horizon=h, params=fl.p); pr = oracle_params(oracle, sc)
    sts = [oracle.default_settings(warm_start=1, linsys=k, **seq.settings) for k in (0, 1)]
    carries = [{int(b): oracle.update_carry(h) for b in idx} for _ in range(2)]
    want = seq.plan(fl.classes)
    worst, reinits = 0.0, 0
    for t, path in enumerate(seq.paths):
        q = fl.tick(t, general=path == "G")
        for b in idx:
            a, c = (oracle_tick(oracle, pr, sts[k], q, int(b), carries[k][int(b)]) for k in range(2))
            assert a["info"].iters == c["info"].iters and a["info"].status == c["info"].status == 1, (seq.name, t, int(b), a["info"].iters, c["info"].iters)
            assert a["info"].reinit == c["info"].reinit == int(want[t, b]), (seq.name, t, int(b))
            reinits += a["info"].reinit
            worst = max(worst, float(np.abs(a["grf"] - c["grf"]).max()))
    print(f"{seq.name}: {len(idx)} robots x {len(seq.paths)} ticks, {reinits} re-initialisations, back ends within {worst:.1e} N")
    assert reinits >= 1 and worst <= (BACK_ENDS_T_N if seq.weights == "test_mpc" else BACK_ENDS_N), (seq.name, worst)
