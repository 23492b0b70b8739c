"""Shared by the balance-QP controller's tests (tests/test_balance_wrench_host.py on the CPU, tests/test_gpu_balance_tick.py on the GPU): the PD wrench's inputs with
the rows that sit on its branches, and the oracle's answer to them (orc_balance_root_acc, pinned to the reference by tests/test_ref_pin.py).  Below them: the balance
QP's own constants off the reference's defaults (tests/test_balance_constants_host.py, tests/test_gpu_balance_constants.py) -- a generic set, its one-property reversions,
the accepted edge sets, the batch with all sixteen contact patterns, and the gate that holds an engine's answer to the oracle's."""
import numpy as np

from helpers import TOL_FORCE_BALANCE_N

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


# ---------------------------------------------------------------------------------------------------------------- the balance QP's constants off their defaults
# The reference's constants (S/A1RobotControl.cpp:11-15) have Q[0] = Q[1] = Q[2], Q[3] = Q[4], F_min = 0 and an F_max that almost never binds, so a kernel (or the library's
# argument fill, which re-orders Q torque-first) that swaps weights inside a triple, reads a force weight for a torque weight, forgets to gate F_min by the contact flag or never
# applies F_max computes the same forces.  The generic set has none of that structure: every weight differs, the lower bound is positive and the upper bound binds.
DEFAULT_BALANCE = dict(Q=(1.0, 1.0, 1.0, 400.0, 400.0, 100.0), R=1e-3, mu=0.7, F_min=0.0, F_max=180.0)
GENERIC_BALANCE = dict(Q=(2.0, 3.5, 0.7, 310.0, 520.0, 90.0), R=3e-3, mu=0.45, F_min=4.0, F_max=50.0)
BALANCE_KEYS = ("grf", "f_world", "iters", "status")
BALANCE_INPUTS = ("root_acc", "R", "Rz", "foot", "contact")
BALANCE_MOVE_N = 100 * TOL_FORCE_BALANCE_N      # what a variant below must move the oracle's forces by, on at least half of a batch


# the batches tests/test_gpu_balance_constants.py solves (balance_batch(scen, n, seed)); tests/test_balance_constants_host.py runs the yardstick alone on each of them
BATCH_MAIN, BATCH_SMALL, BATCH_EDGES = (256, 4242), (9, 4243), (257, 4244)


def balance_settings_cases():
    """the settings the H = 1 kernel is held at: gpu_common.SETTINGS_CASES and one Ruiz pass"""
    from gpu_common import SETTINGS_CASES
    return SETTINGS_CASES + [dict(scaling=1)]


def _with_q(i, j):
    q = list(GENERIC_BALANCE["Q"]); q[i], q[j] = q[j], q[i]
    return dict(GENERIC_BALANCE, Q=tuple(q))


def balance_variants():
    """{name: GENERIC_BALANCE with ONE property put back to the structure of the defaults, or two weights exchanged}: what a kernel or an argument fill computes that swaps
    weights inside a triple, takes the force weights for the torque weights, or reads R, mu, F_min or F_max from somewhere else.  F_max: 50 -> 60 (180 would bind on too few QPs)"""
    G = GENERIC_BALANCE
    return {"Q[0] <-> Q[1]": _with_q(0, 1), "Q[1] <-> Q[2]": _with_q(1, 2), "Q[3] <-> Q[4]": _with_q(3, 4), "Q[4] <-> Q[5]": _with_q(4, 5),
            "force and torque triples exchanged": dict(G, Q=G["Q"][3:] + G["Q"][:3]), "R -> 1e-3": dict(G, R=1e-3), "mu -> 0.7": dict(G, mu=0.7), "F_min -> 0": dict(G, F_min=0.0),
            "F_max 50 -> 60": dict(G, F_max=60.0)}


# constants at the edge of what the library accepts (invalid_balance_config refuses only negative, non-finite and F_min > F_max): the generic set with one field at its edge
BALANCE_EDGE_CONSTANTS = {"mu = 0": dict(GENERIC_BALANCE, mu=0.0), "F_min = F_max = 30": dict(GENERIC_BALANCE, F_min=30.0, F_max=30.0), "R = 0": dict(GENERIC_BALANCE, R=0.0),
                          "Q[1] = Q[4] = 0": dict(GENERIC_BALANCE, Q=(2.0, 0.0, 0.7, 310.0, 0.0, 90.0)), "Q = 0": dict(GENERIC_BALANCE, Q=(0.0,) * 6)}


def balance_config(E, qp):
    """a constants dict as the engine's a1mpc_balance_config (E: the package or its engine module), every field written"""
    c = E.BalanceConfig()
    c.Q[:] = [float(v) for v in qp["Q"]]; c.R, c.mu, c.F_min, c.F_max = float(qp["R"]), float(qp["mu"]), float(qp["F_min"]), float(qp["F_max"])
    return c


def oracle_qp(oracle, qp):
    """a constants dict as the oracle's orc_qp_params"""
    p = oracle.QpParams()
    p.Qw[:] = [float(v) for v in qp["Q"]]; p.R, p.mu, p.F_min, p.F_max = float(qp["R"]), float(qp["mu"]), float(qp["F_min"]), float(qp["F_max"])
    return p


def balance_batch(scen, n, seed):
    """scenarios.balance_random(n, seed) with the contacts of its second half replaced by the pattern b % 16 of robot b: every one of the sixteen patterns, all-swing among them
    (balance_random itself draws 1 .. 15 and is left as it is)"""
    sc = scen.balance_random(n, seed=seed)
    b = np.arange(n // 2, n)
    sc["contact"][n // 2:] = (((b % 16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    if n >= 32:
        assert len({tuple(c) for c in sc["contact"]}) == 16
    return sc


def balance_rows(sc, lo, hi):
    """rows lo .. hi - 1 of a balance batch, as contiguous arrays"""
    return dict(sc, **{k: np.ascontiguousarray(sc[k][lo:hi]) for k in BALANCE_INPUTS})


def oracle_balance(oracle, qp, st, sc):
    """every QP of a balance batch through oracle.balance_solve with the constants dict qp -> dict(grf, f_world, iters, status)"""
    n = len(sc["root_acc"]); q = oracle_qp(oracle, qp)
    ref = dict(grf=np.zeros((n, 12)), f_world=np.zeros((n, 12)), iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    for b in range(n):
        r = oracle.balance_solve(q, st, sc["root_acc"][b], sc["R"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
        ref["grf"][b], ref["f_world"][b], ref["iters"][b], ref["status"][b] = r["grf"], r["f_world"], r["info"].iters, r["info"].status
    return ref


def x87_balance(qp, osqp, sc):
    """-> x87_solve(j): QP j of the batch on the oracle's extended-precision build, constants dict qp, OSQP settings overrides osqp"""
    import x87
    q = x87.qp_params(qp); st = x87.settings(**osqp)
    return lambda j: x87.balance_solve(q, st, sc["root_acc"][j], sc["R"][j], sc["Rz"][j], sc["foot"][j], sc["contact"][j])


def _force_distance(a, b):
    k = len(a["grf"])
    return np.maximum(np.abs(a["grf"] - b["grf"]).reshape(k, -1).max(1), np.abs(a["f_world"] - b["f_world"]).reshape(k, -1).max(1))


def balance_held_to_oracle(out, ref, x87_solve, case, label=""):
    """gpu_common.held_to_oracle for the balance QP.  out / ref: dict(grf, f_world, iters, status) of the same k QPs (engine, oracle).
    1. every QP stops at the oracle's iteration with the oracle's status;
    2. grf and f_world within helpers.TOL_FORCE_BALANCE_N -- or, for fewer than X87_PCT per cent of the QPs (at most X87_PCT_NOISY per cent on NOISY_CASES), settled by the
       extended-precision build of the oracle: x87_solve(j) -> dict(grf, f_world, iters) stops at the same iteration, and the engine is no further from it than 5 x the
       double-precision oracle's own distance + TOL_FORCE_BALANCE_N.
    The caps are conditions: tests/test_balance_constants_host.py shows the oracle and x87 by themselves never part by more than the bar on the batches the GPU file solves.
    Every figure is printed before anything is asserted.  -> dict(resolved, worst (N, engine vs oracle), worst_ratio)"""
    from gpu_common import NOISY_CASES, X87_PCT, X87_PCT_NOISY, case_id
    from helpers import TOL_FORCE_BALANCE_N
    k = len(out["iters"])
    off = np.flatnonzero((out["iters"] != ref["iters"]) | (out["status"] != ref["status"]))
    d = _force_distance(out, ref)
    cand = np.flatnonzero(~(d <= TOL_FORCE_BALANCE_N))       # (a NaN is a candidate, and fails below)
    allowed = (X87_PCT_NOISY * k) // 100 if case in NOISY_CASES else (X87_PCT * k - 1) // 100
    print(f"{label} {case_id(case) or 'default'}: {k} QPs, {len(off)} with another iteration count or status, worst engine-vs-oracle {np.nanmax(d) if k else 0.0:.2e} N, "
          f"{len(cand)} above the bar ({allowed} may be), statuses {dict(zip(*np.unique(ref['status'], return_counts=True)))}")
    rows = []
    for j in cand[np.argsort(-np.nan_to_num(d[cand], nan=np.inf))][:allowed + 4]:
        xr = x87_solve(int(j))
        full = lambda r: np.concatenate([np.ravel(r["grf"][j]), np.ravel(r["f_world"][j])])
        xe = np.concatenate([np.ravel(xr["grf"]), np.ravel(xr["f_world"])])
        rows.append((int(j), float(d[j]), float(np.abs(full(out) - xe).max()), float(np.abs(full(ref) - xe).max()), int(xr["iters"]), int(out["iters"][j])))
    if rows:
        print(f"{label} {case_id(case) or 'default'}: (qp, engine-vs-oracle, engine-vs-x87, oracle-vs-x87, x87 iterations, engine iterations): {rows}")
    assert len(off) == 0, (label, case, [(int(j), int(out["iters"][j]), int(ref["iters"][j]), int(out["status"][j]), int(ref["status"][j])) for j in off[:8]])
    assert len(cand) <= allowed, (label, case, len(cand), k, rows)
    for j, dj, d_e, d_o, it_x, it_e in rows:
        assert it_x == it_e, (label, case, rows)
        assert d_e <= 5.0 * d_o + TOL_FORCE_BALANCE_N, (label, case, rows)
    worst_ratio = max([r[2] / max(r[3], 1e-300) for r in rows], default=0.0)
    return dict(resolved=int(len(cand)), worst=float(d.max()) if k else 0.0, worst_ratio=float(worst_ratio))


def balance_yardstick_alone(label, ref, x87_solve, case):
    """the oracle (ref: dict(grf, f_world, iters, status) of k QPs) against its extended-precision build ALONE: the same iteration count and status on every QP and NO QP
    further than TOL_FORCE_BALANCE_N apart -- balance_held_to_oracle's caps are never needed by the yardstick itself.  -> the worst distance"""
    from gpu_common import case_id
    from helpers import TOL_FORCE_BALANCE_N
    k = len(ref["iters"])
    xs = [x87_solve(j) for j in range(k)]
    x = dict(grf=np.array([v["grf"] for v in xs]), f_world=np.array([v["f_world"] for v in xs]), iters=np.array([v["iters"] for v in xs]), status=np.array([v["status"] for v in xs]))
    d = _force_distance(ref, x)
    off = np.flatnonzero((x["iters"] != ref["iters"]) | (x["status"] != ref["status"]))
    print(f"{label} {case_id(case) or 'default'}: {k} QPs, {len(off)} with another iteration count or status than x87, worst oracle-vs-x87 {d.max():.2e} N, "
          f"{int((~(d <= TOL_FORCE_BALANCE_N)).sum())} above the bar, statuses {dict(zip(*np.unique(ref['status'], return_counts=True)))}")
    assert len(off) == 0, (label, case, off[:8])
    assert (d <= TOL_FORCE_BALANCE_N).all(), (label, case, float(d.max()))
    return float(d.max())


_VARIANTS_SEEN = {}


def assert_balance_variants_move(oracle, sc, settings=None, label="", names=None):
    """The sensitivity precondition, on the ORACLE alone, before any engine output is read: every balance_variants() entry moves the oracle's grf of the batch sc (solved at
    GENERIC_BALANCE under `settings`) by more than 100 x TOL_FORCE_BALANCE_N on at least half of its QPs -- or a pass on that batch could not tell the generic set from the
    variant.  A (batch, settings) pair is solved once per session; names: only these variants are asserted (all are printed).  -> {name: (share, median move)}"""
    from gpu_common import assert_variants_move
    st = oracle.default_settings() if settings is None else settings
    key = (hash(b"".join(np.ascontiguousarray(sc[k]).tobytes() for k in BALANCE_INPUTS)), bytes(st))
    if key not in _VARIANTS_SEEN:
        full = oracle_balance(oracle, GENERIC_BALANCE, st, sc)["grf"]
        _VARIANTS_SEEN[key] = (full, {name: oracle_balance(oracle, var, st, sc)["grf"] for name, var in balance_variants().items()})
    full, var = _VARIANTS_SEEN[key]
    label = f"{label} balance QP x {len(full)}".strip()
    if names is not None:
        assert_variants_move(label + " (not asserted)", full, {k: v for k, v in var.items() if k not in names}, move=BALANCE_MOVE_N, share=0.0)
        var = {k: var[k] for k in names}
    return assert_variants_move(label, full, var, move=BALANCE_MOVE_N, share=0.5)
