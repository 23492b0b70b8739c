"""GPU, through the C ABI: OSQP settings away from their defaults, other friction / force limits, the failure statuses (MAX_ITER_REACHED, SOLVED_INACCURATE, NON_CVX on
non-finite input) and warm_start = 1 / 2 on EVERY kernel family -- the fused kernel, the split pipeline (set-up kernel + persistent rows, CU-wide at h = 16, quads of rows at
h = 20), an extended horizon, the general path's three kernels -- vs the oracle run with the same settings.  tests/test_gpu_settings.py holds the same settings on the
latency kernel alone (n <= 256); the Ruiz blocks, the fz_min > 0 first iteration, the checkpoint arithmetic and the output stage are written per kernel family.

The gate (gpu_common.held_to_oracle): every QP stops at the oracle's iteration with the oracle's status; forces within TOL_FORCE_N, or -- for at most 6 % of a batch on the
three cases where ADMM amplifies the last bits of the linear solves (scaling = 0, rho = 1.0, check_termination = 10 with adaptive_rho_interval = 35) and under 1 % on the
others -- settled by the extended-precision build of the oracle (tests/x87.py), as test_settings_above_the_parity_bar_are_the_checkers_own_rounding does.  The share comes
from the oracle's own two linear-system back ends compared at these shapes (DESIGN.md "Parity"), not from the engine."""
import numpy as np
import pytest

from gpu_common import (FAMILY_CASES, FAMILY_SUBSET, _engine, _strided_inputs, assert_all_three_outcomes, case_id, family_scenario, held_to_oracle, oracle_sample,
                        oracle_strided, split_case)
from helpers import TOL_FORCE_BALANCE_N, TOL_FORCE_N, oracle_batch, oracle_params, take

pytestmark = pytest.mark.gpu

# (horizon, fused batch, split batch): the smallest batches the suite already uses to reach each kernel.  h = 16: fused quads / the CU-wide persistent workgroup; h = 20: the
# quads of rows; h = 12: one extended horizon (its fused kernel is the h = 10 family's instantiation, held at default settings by tests/test_gpu_extended_horizons.py).
FAST_SHAPES = [(10, 1500, 3000), (16, 700, 1500), (20, 300, 1300), (12, None, 2600)]
# the general path: (horizon, batch, kernel)
GEN_SHAPES_H10 = [(10, 128, "latency"), (10, 300, "fused"), (10, 4000, "split")]
GEN_SHAPES_LONG = [(16, 2100, "split"), (20, 1700, "split")]
KEYS = ("u", "grf", "iters", "status")


def _x87_cold(sc, h, osqp, foot=None, fs=0, contact=None, cs=0):
    import x87
    xpr = x87.params(sc["params"], h); xst = x87.settings(**osqp)
    foot = sc["foot"] if foot is None else foot; contact = sc["contact"] if contact is None else contact
    return lambda j: x87.mpc_solve(xpr, xst, sc["x0"][j], sc["xref"][j], sc["R"][j], foot[j], contact[j], foot_stride=fs, contact_stride=cs)


# ------------------------------------------------------------------------------------------------ 1. settings x kernel family, cold first solves (+ 4. statuses)
@pytest.mark.parametrize("h,n_fused,n_split", FAST_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", FAMILY_CASES, ids=case_id)
def test_settings_on_the_fused_kernel_and_the_split_pipeline(pkg, oracle, scen, case, h, n_fused, n_split):
    """one batch per (case, horizon), seed 9100 + h: all of it through the split pipeline, its first n_fused QPs through the fused kernel, its first 200 through the latency
    kernel.  Which kernel ran is asserted (a1mpc_last_stage_ms: only the split pipeline has a set-up stage of its own); the latency kernel's rows equal the split batch's bit
    for bit; split and fused batch are held to the oracle on every QP.  max_iter = 30: the oracle's answer holds MAX_ITER_REACHED, SOLVED_INACCURATE and SOLVED (asserted
    first, on every batch compared), and the engine returns the same status and iteration count on every QP."""
    osqp, par = split_case(case)
    sc = family_scenario(scen, h, n_split, par)
    ref = oracle_batch(oracle, sc, settings=oracle.default_settings(**osqp))
    sizes = [n for n in (n_split, n_fused) if n is not None]
    if osqp.get("max_iter") == 30:
        for n in sizes:
            print(h, n, "oracle statuses at max_iter = 30:", assert_all_three_outcomes(ref["status"][:n]))
    outs = {}
    with _engine(pkg, sc, n_split, warm_start=0, **osqp) as eng:
        for n in sizes + [200]:
            s = take(sc, n)
            outs[n] = eng.solve(s["x0"], s["xref"], s["R"], s["foot"], s["contact"], want_u=True)
            form_ms = eng.last_stage_ms()[0]
            assert (form_ms > 0.0) if n == n_split else (form_ms == 0.0), (h, n, form_ms)
    for k in KEYS:
        assert np.array_equal(outs[n_split][k][:200], outs[200][k]), (h, k)
    x87_solve = _x87_cold(sc, h, osqp)
    for n in sizes:
        held_to_oracle(outs[n], {k: ref[k][:n] for k in KEYS}, x87_solve, case, label=f"h{h} x {n} ({'split' if n == n_split else 'fused'})")


# ------------------------------------------------------------------------------------------------ 2. the same on the general path
@pytest.mark.parametrize("h,n,kernel", GEN_SHAPES_H10, ids=lambda v: str(v))
@pytest.mark.parametrize("case", FAMILY_CASES, ids=case_id)
def test_settings_on_the_general_path_h10(pkg, oracle, scen, case, h, n, kernel):
    """per-step feet and a contact schedule (_strided_inputs): the general path's latency kernel, fused kernel and split pipeline at h = 10, every case, vs the oracle's
    strided formation on a sample of >= 96 QPs that holds the first and the last.  max_iter = 30: every QP of the batch (a 30-iteration solve is cheap), and the oracle's
    answer must hold all three outcomes before the engine is looked at."""
    _general_path_case(pkg, oracle, scen, case, h, n, kernel)


@pytest.mark.parametrize("h,n,kernel", GEN_SHAPES_LONG, ids=lambda v: str(v))
@pytest.mark.parametrize("case", FAMILY_SUBSET, ids=case_id)
def test_settings_on_the_general_path_h16_h20(pkg, oracle, scen, case, h, n, kernel):
    """the general path's split pipeline at h = 16 and h = 20, the subset of cases that reaches each block the settings steer (Ruiz off / three passes, a fixed rho, the
    checkpoint arithmetic, the iteration limit, the fz_min > 0 first iteration)"""
    _general_path_case(pkg, oracle, scen, case, h, n, kernel)


def _general_path_case(pkg, oracle, scen, case, h, n, kernel):
    osqp, par = split_case(case)
    rng = np.random.default_rng(9200 + h + n)
    sc, foot, fs, contact, cs = _strided_inputs(scen, rng, h, n, True, True)
    sc["params"] = dict(sc["params"], **par)
    pr = oracle_params(oracle, sc); st = oracle.default_settings(**osqp)
    # max_iter = 30: EVERY QP of the batch (status and iteration count on every QP is what part of the contract this case holds; a 30-iteration solve is cheap)
    idx = np.arange(n) if osqp.get("max_iter") == 30 else oracle_sample(n, 96)
    assert len(idx) >= min(n, 96) and idx[0] == 0 and idx[-1] == n - 1
    ref = oracle_strided(oracle, pr, st, sc, foot, fs, contact, cs, idx)
    if osqp.get("max_iter") == 30:
        print(h, n, "oracle statuses at max_iter = 30:", assert_all_three_outcomes(ref["status"]))
    with _engine(pkg, sc, n, warm_start=0, **osqp) as eng:
        out = eng.solve_strided(sc["x0"], sc["xref"], sc["R"], foot, fs, contact, cs, want_u=True)
        form_ms = eng.last_stage_ms()[0]
    assert (form_ms > 0.0) if kernel == "split" else (form_ms == 0.0), (h, n, kernel, form_ms)
    x87_sub = _x87_cold(sc, h, osqp, foot, fs, contact, cs)
    held_to_oracle({k: out[k][idx] for k in KEYS}, ref, lambda j: x87_sub(int(idx[j])), case, label=f"general path h{h} x {n} ({kernel})")


# ------------------------------------------------------------------------------------------------ 3. warm_start = 1 and 2 with the subset
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("h,n", [(10, 64), (10, 2600), (16, 1500)])
@pytest.mark.parametrize("case", FAMILY_SUBSET, ids=case_id)
def test_warm_start_modes_with_non_default_settings(pkg, oracle, scen, case, h, n, mode):
    """the pattern of test_update_path_and_warm_start -- four ticks of slowly moving states, every leg changing role at tick 2, each robot with its own carry -- under
    non-default settings: warm_start = 1 (x, y, rho carried) and warm_start = 2 (the update path: re-equilibration with the carried scalings).  n = 64: every robot is
    chained through the oracle; 2600 x h10 and 1500 x h16: a sample of 24 that holds the first and the last.

    FOUND HERE AND FIXED: max_iter = 30 at h10 x 64, tick 1, robot 26.  Its tick 0 ends at the iteration limit with rho adapted down to OSQP's floor, 1e-6, and tick 1 STARTS
    at that rho.  RowSolver carried c P x + c g through the x-update identity only from a rho UPDATE that landed at or below 1e-3 onwards, so this solve re-evaluated it at its
    first checkpoint, where the Riccati solves' backward error dominates the dual residual: same 30 iterations and status as the oracle, the rho estimate of iteration 25 off by
    2.3e-6 relative, forces 2.2e-5 N (mode 1) / 1.7e-5 N (mode 2) from the oracle's while the oracle is 4.5e-9 / 9.3e-9 N from its x87 build -- 1 of 64 QPs above the bar where
    fewer than 1 % may be.  A solve that starts at such a rho now seeds the carried value at a checkpoint of its own after iteration 1 (RowSolver::advance)."""
    import x87
    osqp, par = split_case(case)
    rng = np.random.default_rng(9300 + 7 * h + n)
    sc = family_scenario(scen, h, n, par, seed=9300 + h + n)
    pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1, **osqp)
    xpr = x87.params(sc["params"], h); xst = x87.settings(warm_start=1, **osqp)
    chk = np.arange(n) if n <= 64 else oracle_sample(n, 24)
    carries = {b: oracle.update_carry(h) for b in chk}
    wx = {b: np.zeros(12 * h) for b in chk}; wy = {b: np.zeros(20 * h) for b in chk}; rho = {b: None for b in chk}
    with _engine(pkg, sc, n, warm_start=mode, **osqp) as eng:
        for t in range(4):
            if t > 0:
                sc["x0"][:, :12] += rng.normal(0, 2e-3, (n, 12)); sc["foot"] += rng.normal(0, 1e-3, (n, 12))
            if t == 2:
                sc["contact"][:] = 1 - sc["contact"]
                sc["contact"][sc["contact"].sum(1) == 0] = [1, 0, 0, 1]
            out = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
            before = {b: (carries[b].copy(), wx[b].copy(), wy[b].copy(), rho[b]) for b in chk}    # what the extended-precision run of a QP starts from
            ref = dict(u=np.zeros((len(chk), 12 * h)), grf=np.zeros((len(chk), 12)), iters=np.zeros(len(chk), np.int32), status=np.zeros(len(chk), np.int32))
            for j, b in enumerate(chk):
                a = (sc["x0"][b], sc["xref"][b], sc["R"][b], sc["foot"][b], sc["contact"][b])
                if mode == 2:
                    o = oracle.mpc_solve_update(pr, st, *a, carries[b])
                else:
                    o = oracle.mpc_solve(pr, st, *a, warm_x=wx[b], warm_y=wy[b], warm_rho=rho[b])
                    wx[b], wy[b], rho[b] = o["warm_x"], o["warm_y"], o["rho"]
                ref["u"][j], ref["grf"][j], ref["iters"][j], ref["status"][j] = o["u"], o["grf"], o["info"].iters, o["info"].status

            def x87_solve(j):
                b = chk[j]; c, x, y, r = before[b]
                a = (sc["x0"][b], sc["xref"][b], sc["R"][b], sc["foot"][b], sc["contact"][b])
                return x87.mpc_solve_update(xpr, xst, *a, c) if mode == 2 else x87.mpc_solve(xpr, xst, *a, warm_x=x, warm_y=y, warm_rho=r)
            held_to_oracle({k: out[k][chk] for k in KEYS}, ref, x87_solve, case, label=f"warm_start = {mode}, h{h} x {n}, tick {t}")
        if mode == 2:
            assert eng.last_warm_start_mode() == 2


# ------------------------------------------------------------------------------------------------ 5. non-finite inputs away from the fast path's h = 10 kernels
def _bad_rows(n, k):
    """k disjoint groups of robots spread over a batch: its first and last rows, wave-mates (63 / 64), the middle"""
    base = np.unique(np.array([0, 1, 2, 62, 63, 64, 65, n // 2, n // 2 + 1, n // 2 + 2, n - 3, n - 2, n - 1]))
    return [base[i::k] for i in range(k)]


def _assert_bad_rows_fail_and_leave_no_trace(bad_out, clean_out, bad, what):
    """status -7 and zero forces for the robots with a non-finite input; every other robot bit for bit what the batch gives with those inputs finite"""
    n = len(clean_out["iters"])
    isbad = np.zeros(n, bool); isbad[bad] = True
    assert (bad_out["status"][isbad] == -7).all() and not bad_out["grf"][isbad].any(), (what, bad_out["status"][isbad], np.abs(bad_out["grf"][isbad]).max())
    assert (clean_out["status"] == 1).all(), what
    for k in KEYS:
        if bad_out.get(k) is not None:
            assert np.array_equal(bad_out[k][~isbad], clean_out[k][~isbad]), (what, k, np.flatnonzero((bad_out[k] != clean_out[k]).reshape(n, -1).any(1) & ~isbad)[:8])


@pytest.mark.parametrize("h,n", [(16, 1500), (20, 1300), (12, 2600)])
def test_non_finite_inputs_on_the_split_pipelines(pkg, scen, h, n):
    """the CU-wide persistent workgroup (h = 16), the quads of rows (h = 20) and an extended horizon's persistent rows: a NaN in x0, an Inf in R, and a tick record with a NaN
    command field (a1mpc_solve_batch_ticks) -- NON_CVX and zero forces for those robots, every other robot of the batch bit for bit what it is without them"""
    sc = family_scenario(scen, h, n, {}, seed=9500 + h)
    nan_x0, inf_R, nan_cmd = _bad_rows(n, 3)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        x0 = sc["x0"].copy(); x0[nan_x0, 4] = np.nan
        R = sc["R"].copy(); R[inf_R, 5] = np.inf
        a = eng.solve(x0, sc["xref"], R, sc["foot"], sc["contact"], want_u=True)
        assert eng.last_stage_ms()[0] > 0.0
        clean = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
        _assert_bad_rows_fail_and_leave_no_trace(a, clean, np.concatenate([nan_x0, inf_R]), f"h{h} x {n}: NaN in x0 / Inf in R")
        tick = sc["tick"].copy(); tick[nan_cmd, 16] = np.nan     # root_lin_vel_d y
        b = eng.solve_ticks(tick, sc["R"], sc["foot"], sc["contact"], want_u=True)
        assert eng.last_stage_ms()[0] > 0.0
        clean_t = eng.solve_ticks(sc["tick"], sc["R"], sc["foot"], sc["contact"], want_u=True)
        _assert_bad_rows_fail_and_leave_no_trace(b, clean_t, nan_cmd, f"h{h} x {n}: tick records with a NaN command")


@pytest.mark.parametrize("n,kernel", [(300, "fused"), (4000, "split")])
def test_non_finite_inputs_on_the_general_path(pkg, scen, n, kernel):
    """the general path's fused kernel and split pipeline at h = 10: a NaN in x0, an Inf in R, and a NaN in the feet of a step k > 0 only (step 0 finite, under a leg that
    stands at step k) -- NON_CVX and zero forces for those robots, every other robot bit for bit what it is without them"""
    h = 10
    rng = np.random.default_rng(9600 + n)
    sc, foot, fs, contact, cs = _strided_inputs(scen, rng, h, n, True, True)
    nan_x0, inf_R, nan_feet = _bad_rows(n, 3)
    ct = contact.reshape(n, h, 4)
    nan_feet = np.array([b for b in nan_feet if ct[b, 1:].any()])     # a robot needs a stance leg at some step k > 0 to carry the NaN
    assert len(nan_feet) >= 2
    x0 = sc["x0"].copy(); x0[nan_x0, 7] = np.nan
    R = sc["R"].copy(); R[inf_R, 0] = np.inf
    feet = foot.copy()
    for b in nan_feet:
        k, leg = np.argwhere(ct[b, 1:] == 1)[-1]
        feet[b, 12 * (k + 1) + 3 * leg + 1] = np.nan
    assert np.isfinite(feet[:, :12]).all()
    with _engine(pkg, sc, n, warm_start=0) as eng:
        a = eng.solve_strided(x0, sc["xref"], R, feet, fs, contact, cs, want_u=True)
        form_ms = eng.last_stage_ms()[0]
        clean = eng.solve_strided(sc["x0"], sc["xref"], sc["R"], foot, fs, contact, cs, want_u=True)
    assert (form_ms > 0.0) if kernel == "split" else (form_ms == 0.0), (n, kernel, form_ms)
    _assert_bad_rows_fail_and_leave_no_trace(a, clean, np.concatenate([nan_x0, inf_R, nan_feet]), f"general path h10 x {n}")


def test_non_finite_inputs_in_a_depth_2_pipeline(pkg, scen):
    """two batches in flight on a depth-2 a1mpc_pipeline (h = 16 x 1500, the CU-wide persistent workgroup), the first with a NaN in x0 and an Inf in R: NON_CVX and zero
    forces for those robots; every other robot of either batch bit for bit what a lone handle gives for the finite batches"""
    h, n = 16, 1500
    scs = [family_scenario(scen, h, n, {}, seed=9700 + k) for k in range(2)]
    nan_x0, inf_R = _bad_rows(n, 2)
    x0 = scs[0]["x0"].copy(); x0[nan_x0, 4] = np.nan
    R = scs[0]["R"].copy(); R[inf_R, 5] = np.inf
    cfg = pkg.make_config(scs[0]["params"], h, warm_start=0)
    with pkg.Engine(cfg, n, 0) as eng:
        lone = [eng.solve(s["x0"], s["xref"], s["R"], s["foot"], s["contact"], want_u=True) for s in scs]
    outs = [dict(grf=np.full((n, 12), np.nan), u=np.full((n, 12 * h), np.nan), iters=np.full(n, -1, np.int32), status=np.full(n, -99, np.int32)) for _ in scs]
    with pkg.Pipeline(cfg, n, 0, depth=2) as pipe:
        pipe.submit(x0, scs[0]["xref"], R, scs[0]["foot"], scs[0]["contact"], outs[0])
        pipe.submit(scs[1]["x0"], scs[1]["xref"], scs[1]["R"], scs[1]["foot"], scs[1]["contact"], outs[1])
        pipe.wait()
    _assert_bad_rows_fail_and_leave_no_trace(outs[0], lone[0], np.concatenate([nan_x0, inf_R]), "pipeline slot 0")
    for k in KEYS:
        assert np.array_equal(outs[1][k], lone[1][k]), k


def test_failed_tick_leaves_a_cold_start_behind_h16(pkg, oracle, scen):
    """warm_start = 1 at h = 16 x 1500: a NaN tick for some robots -> NON_CVX and zero forces, a carried workspace of zeros with the rho the solver had reached, and the NEXT
    tick of those robots is the oracle's restarted from cold iterates with that rho (test_failed_tick_leaves_a_cold_start_behind holds this on the h = 10 latency kernel);
    the other robots' ticks are bit for bit those of a handle that never saw the NaN"""
    h, n = 16, 1500
    sc = family_scenario(scen, h, n, {}, seed=9800 + h)
    bad = np.concatenate(_bad_rows(n, 1)); isbad = np.zeros(n, bool); isbad[bad] = True
    args = lambda x0: (x0, sc["xref"], sc["R"], sc["foot"], sc["contact"])
    x0 = sc["x0"].copy(); x0[bad, 4] = np.nan
    x2 = sc["x0"].copy(); x2[:, :12] += np.random.default_rng(9800).normal(0, 2e-3, (n, 12))
    with _engine(pkg, sc, n, warm_start=1) as eng, _engine(pkg, sc, n, warm_start=1) as twin:
        eng.solve(*args(sc["x0"])); twin.solve(*args(sc["x0"]))
        _, _, rho0 = eng.get_warm_start(n)
        o1 = eng.solve(*args(x0), want_u=True); t1 = twin.solve(*args(sc["x0"]), want_u=True)
        _assert_bad_rows_fail_and_leave_no_trace(o1, t1, bad, "warm_start = 1, the failed tick")
        wx, wy, rho = eng.get_warm_start(n)
        assert np.isfinite(wx).all() and np.isfinite(wy).all() and not wx[isbad].any() and not wy[isbad].any()
        assert np.array_equal(rho[isbad], rho0[isbad]) and (rho0[isbad] > 0).all()     # the failed solve never got to adapt: the rho it was started with stays
        o2 = eng.solve(*args(x2), want_u=True); t2 = twin.solve(*args(x2), want_u=True)
    assert (o2["status"] == 1).all()
    for k in KEYS:
        assert np.array_equal(o2[k][~isbad], t2[k][~isbad]), k
    pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1)
    for i in bad:
        r = oracle.mpc_solve(pr, st, x2[i], sc["xref"][i], sc["R"][i], sc["foot"][i], sc["contact"][i], warm_x=np.zeros(12 * h), warm_y=np.zeros(20 * h), warm_rho=rho[i])
        assert o2["iters"][i] == r["info"].iters and o2["status"][i] == r["info"].status and np.abs(o2["u"][i] - r["u"]).max() <= TOL_FORCE_N, i


@pytest.mark.parametrize("n,bad", [(4, [1]), (64, [1, 37, 63])])
def test_balance_qp_with_a_non_finite_root_acc(pkg, oracle, scen, n, bad):
    """a1mpc_balance_solve_batch (n = 4: the pinned small-batch block; n = 64: staged copies): a NaN root_acc gives NON_CVX and zero GRFs for that row, the oracle's answer for
    the others"""
    sc = scen.balance_random(n, seed=9900 + n)
    acc = sc["root_acc"].copy(); acc[bad, 2] = np.nan
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, 10)
    with pkg.Engine(cfg, 64, 0) as eng:
        out = eng.balance_solve(acc, sc["R"], sc["Rz"], sc["foot"], sc["contact"])
    qp, st = oracle.default_qp_params(), oracle.default_settings()
    for b in range(n):
        if b in bad:
            assert out["status"][b] == -7 and not out["grf"][b].any(), (b, out["status"][b])     # (f_world is the solver's x like u_full_out: NaN, on the oracle too)
            continue
        r = oracle.balance_solve(qp, st, sc["root_acc"][b], sc["R"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
        assert out["iters"][b] == r["info"].iters and out["status"][b] == r["info"].status, b
        assert max(np.abs(out["f_world"][b] - r["f_world"]).max(), np.abs(out["grf"][b] - r["grf"]).max()) < TOL_FORCE_BALANCE_N, b
