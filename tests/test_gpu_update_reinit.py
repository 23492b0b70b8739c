"""GPU, through the C ABI: warm_start = 2 when the zero pattern of the dense Hessian changes between two ticks -- osqp-eigen clears the solver, sets it up again (fresh
scaling, rho back to the settings' rho) and warm-starts it from the previous solve's SCALED iterates (RowSolver::setup "pattern change"; oracle/a1mpc_oracle.c `reinit`)
-- on every kernel family that has an update-path instantiation, on both paths, across path switches, under zero weights, and next to the other things a handle does.

Yardstick: oracle.mpc_solve_update with one carry per followed robot (foot_stride = 12 on the ticks that ran the general path).  On every followed robot on every tick:
the oracle's iteration count and status, |dGRF| <= TOL_FORCE_N, and the handle reports warm-start mode 2.  Before any kernel output is looked at, the oracle's
info.reinit must equal the PLAN of the fleet (tests/update_reinit_common.py: which class of robot changes which foot coordinate to exactly 0.0 on which tick; the
classes interleave by index % 4, so every main / twin pair, quad and CU-wide workgroup holds re-initialising and updating robots on the same tick).

Constants: the `hardware` set.  On it the oracle's own two linear-system back ends stay within 1e-9 N of each other over each of these sequences
(tests/test_update_reinit_host.py asserts that), so the distance to the oracle measures the kernel and not the conditioning of the doubly scaled warm start.

Families are reached by batch size, with a1mpc_last_stage_ms telling the split pipeline (it alone has a set-up stage of its own) from the others."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import _engine
from helpers import TOL_FORCE_N, oracle_params
from update_reinit_common import FAMILIES, INTERPLAY, SETTINGS, SWITCH_PATHS, SWITCHES, ZERO_WEIGHTS, followed, oracle_tick

pytestmark = pytest.mark.gpu


def _solve(eng, q):
    if q["foot_stride"]:
        return eng.solve_strided(q["x0"], q["xref"], q["R"], q["foot"], 12, q["contact"], 0)
    return eng.solve(q["x0"], q["xref"], q["R"], q["foot"], q["contact"])


def _held(oracle, pr, st, q, out, idx, carries, want, what):
    """one tick: the oracle's re-initialisations equal the plan `want` (input side), then the engine's output equals the oracle's on every followed robot"""
    res = [oracle_tick(oracle, pr, st, q, int(b), carries[int(b)]) for b in idx]
    got = np.array([bool(o["info"].reinit) for o in res])
    assert np.array_equal(got, np.asarray(want)[idx]), (what, "the oracle's re-initialisations are not the planned ones", got.astype(int), np.asarray(want)[idx].astype(int))
    worst = 0.0
    for b, o in zip(idx, res):
        d = float(np.abs(out["grf"][b] - o["grf"]).max())
        worst = max(worst, d)
        assert out["iters"][b] == o["info"].iters and out["status"][b] == o["info"].status, (what, int(b), int(out["iters"][b]), o["info"].iters, int(out["status"][b]),
                                                                                             o["info"].status, "reinit", int(o["info"].reinit))
        assert d <= TOL_FORCE_N, (what, int(b), d)
    return worst, res


def _chain(pkg, oracle, scen, seq):
    """the sequence's fleet on one handle and, its followed robots, on the oracle"""
    fl = seq.fleet(scen); paths = seq.paths; what = seq.name
    sc = dict(horizon=fl.h, params=fl.p)
    pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1, **seq.settings)
    idx = followed(fl.n, fl.classes)
    carries = {int(b): oracle.update_carry(fl.h) for b in idx}
    want = seq.plan(fl.classes)
    assert want[:, idx].any() and fl.n < 4 or all((fl.classes[idx] == c).any() for c in range(4)), (what, "a class without a followed robot")
    worst, seen = 0.0, []
    with _engine(pkg, sc, fl.n, warm_start=2, **seq.settings) as eng:
        for t, path in enumerate(paths):
            q = fl.tick(t, general=path == "G")
            out = _solve(eng, q)
            assert eng.last_warm_start_mode() == 2, (what, t)
            seen.append(eng.last_stage_ms()[0] > 0.0)
            w, _ = _held(oracle, pr, st, q, out, idx, carries, want[t], (what, "tick", t, path))
            worst = max(worst, w)
    print(f"{what}: {fl.n} x h{fl.h}, {len(idx)} robots followed over {len(paths)} ticks ({paths}), {int(want[:, idx].sum())} re-initialisations, "
          f"worst |dGRF| {worst:.2e} N, set-up stage of its own per tick {[int(s) for s in seen]}")
    if isinstance(seq.staged, tuple):
        assert tuple(seen) == seq.staged, (what, seen)
    elif seq.staged is not None:
        assert all(s == seq.staged for s in seen[1:]), (what, seen)
    return worst


_ids = lambda seqs: [q.name for q in seqs]


@pytest.mark.parametrize("seq", FAMILIES, ids=_ids(FAMILIES))
def test_update_path_reinitialisation_on_every_kernel_family(pkg, oracle, scen, seq):
    """the four classes of the fleet (never | tick 2 | ticks 2 and 4 with a leg-to-leg move of the zero | every tick through a cycle of four patterns) interleaved in one
    batch with an odd count, on the kernel family the batch size selects"""
    _chain(pkg, oracle, scen, seq)


@pytest.mark.parametrize("seq", SWITCHES, ids=_ids(SWITCHES))
def test_reinitialisation_across_path_switches(pkg, oracle, scen, seq):
    """a handle that alternates between the fast and the general path (SWITCH_PATHS): the pattern is compared across the switch -- a switch without a change stays on
    the update path, a change that comes with a switch (either direction) or on the tick after one re-initialises"""
    want = seq.plan(seq.fleet(scen).classes)
    sw = [t for t in range(1, len(SWITCH_PATHS)) if SWITCH_PATHS[t] != SWITCH_PATHS[t - 1]]
    if seq.n >= 4:
        for a, b in (("F", "G"), ("G", "F")):
            at = [t for t in sw if SWITCH_PATHS[t - 1] == a and SWITCH_PATHS[t] == b]
            assert any(want[t].any() for t in at) and any((~want[t]).any() for t in at), (a, b)
        assert any(want[t + 1, 1:3].any() for t in sw if t + 1 < len(SWITCH_PATHS))
    else:
        assert want.any()
    _chain(pkg, oracle, scen, seq)


@pytest.mark.parametrize("seq", ZERO_WEIGHTS, ids=_ids(ZERO_WEIGHTS))
def test_reinitialisation_follows_the_weighted_pattern(pkg, oracle, scen, seq):
    """a flag of B~ that changes under a zero weight changes no stored entry of the Hessian.  `unweighted`: roll, pitch and their rates carry no weight, a foot's z
    toggled to 0.0 is no pattern change (classes 1 and 3), a foot's y is (class 2); `test_mpc`: roll and pitch are weighted, every toggle is a change.  Where the
    oracle does not re-initialise the kernel must not either."""
    cls = seq.fleet(scen).classes; want = seq.plan(cls)
    if seq.weights == "unweighted":
        assert not want[:, cls == 1].any() and not want[:, cls == 3].any() and want[:, cls == 2].any()
    _chain(pkg, oracle, scen, seq)


@pytest.mark.parametrize("seq", SETTINGS, ids=_ids(SETTINGS))
def test_reinitialisation_under_non_default_settings(pkg, oracle, scen, seq):
    """gpu_common.SETTINGS_CASES that make "rho back to the settings' rho" (a non-default rho; no adaptation, so nothing else ever moves it) and "fresh scaling" (none at
    all) visible"""
    from gpu_common import SETTINGS_CASES
    assert seq.settings in SETTINGS_CASES
    _chain(pkg, oracle, scen, seq)


# --------------------------------------------------------------------------------------------------------------------------------- interplay
def test_a_change_after_a_failed_tick_still_compares_the_patterns(pkg, oracle, scen):
    """tick 2 fails on every third robot (a NaN in x0: zeros out, NON_CVX).  OSQP's workspace survives a failed solve with cold iterates (store_solution -> cold_start; the
    scalings, the data and the pattern stay), so on tick 3 the pattern is still compared against tick 2's: the failed robots whose pattern changes re-initialise -- from
    zero iterates --, the others follow the update path"""
    n, h = 41, 10
    fl = INTERPLAY["failed"].fleet(scen)
    sc = dict(horizon=h, params=fl.p); pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1)
    idx = np.arange(n); carries = {b: oracle.update_carry(h) for b in range(n)}
    want = fl.plan(6); bad = np.arange(n) % 3 == 0
    assert want[3, bad].any() and not want[3, bad].all() and want[3, ~bad].any()
    with _engine(pkg, sc, n, warm_start=2) as eng:
        for t in range(6):
            q = fl.tick(t)
            if t == 2:
                q["x0"][bad, 4] = np.nan
            out = _solve(eng, q)
            assert eng.last_warm_start_mode() == 2
            _, res = _held(oracle, pr, st, q, out, idx, carries, want[t], ("failed tick", t))
            if t == 2:
                assert all(res[b]["info"].status == -7 for b in np.flatnonzero(bad)) and not out["grf"][bad].any()


def test_a_change_after_an_injected_warm_start(pkg, oracle, scen):
    """a1mpc_warm_start on the update path replaces the iterates and keeps the previous tick's workspace (scalings, data, pattern); a pattern change on the next tick
    re-initialises from the INJECTED iterates, scaled by the previous tick's equilibration.  The oracle starts from exactly that workspace (carry_from_workspace)."""
    n, h = 24, 10
    fl = INTERPLAY["injected"].fleet(scen)
    sc = dict(horizon=h, params=fl.p); pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1); mu = fl.p["mu"]
    rng = np.random.default_rng(85)
    want = fl.plan(5)
    assert want[4].any() and not want[4].all()
    with _engine(pkg, sc, n, warm_start=2) as eng:
        lead = {b: oracle.update_carry(h) for b in range(n)}
        for t in range(4):
            q3 = fl.tick(t); o3 = _solve(eng, q3)
            assert eng.last_warm_start_mode() == 2, t
            _held(oracle, pr, st, q3, o3, np.arange(n), lead, want[t], ("lead-in tick", t))
        x, y, rho = eng.get_warm_start(n); D, E, c = eng.get_workspace_scaling(n)
        xi = x * (1.0 + rng.normal(0, 0.02, x.shape)); yi = y * (1.0 + rng.normal(0, 0.02, y.shape)); ri = rho * 1.5
        eng.set_warm_start(xi, yi, ri)
        q = fl.tick(4)
        out = _solve(eng, q)
        assert eng.last_warm_start_mode() == 2
    f = xi.reshape(n, h, 4, 3)
    zA = np.stack([f[..., 0] + mu * f[..., 2], f[..., 0] - mu * f[..., 2], f[..., 1] + mu * f[..., 2], f[..., 1] - mu * f[..., 2], f[..., 2]], axis=-1).reshape(n, 20 * h)
    carries = {}
    for b in range(n):
        P, g, _, l, u, _ = oracle.mpc_form(pr, q3["x0"][b], q3["xref"][b], q3["R"][b], q3["foot"][b], q3["contact"][b])
        carries[b] = oracle.carry_from_workspace(h, xi[b], yi[b], zA[b], ri[b], D[b], E[b], c[b], P, g, l, u)
    worst, _ = _held(oracle, pr, st, q, out, np.arange(n), carries, want[4], "tick after a1mpc_warm_start")
    print(f"a pattern change after an injected warm start: {int(want[4].sum())} of {n} robots re-initialise, worst |dGRF| {worst:.2e} N")


def test_a_change_after_reset_warm_start(pkg, oracle, scen):
    """a1mpc_reset_warm_start drops the workspace: the next tick is a first tick (no re-initialisation, whatever the pattern did), the one after compares against it"""
    n, h = 41, 10
    fl = INTERPLAY["reset"].fleet(scen)
    sc = dict(horizon=h, params=fl.p); pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1)
    idx = np.arange(n); carries = {b: oracle.update_carry(h) for b in range(n)}
    want = fl.plan(6)
    assert want[3].any() and want[4].any()
    want[3] = False                                         # the reset comes before tick 3
    with _engine(pkg, sc, n, warm_start=2) as eng:
        for t in range(6):
            if t == 3:
                eng.reset_warm_start()
                carries = {b: oracle.update_carry(h) for b in range(n)}
            q = fl.tick(t)
            out = _solve(eng, q)
            assert eng.last_warm_start_mode() == 2, t
            _held(oracle, pr, st, q, out, idx, carries, want[t], ("reset", t))


def test_pipeline_slots_reinitialise_on_their_own_ticks(pkg, oracle, scen):
    """two fleets on the two slots of a pipeline, their classes one apart: robot b re-initialises on other ticks in slot 0 than in slot 1.  Each slot carries its own
    workspace, pattern included"""
    n, h, ticks = 41, 10, 6
    fleets = [INTERPLAY[f"slot{s}"].fleet(scen) for s in range(2)]
    sc = dict(horizon=h, params=fleets[0].p); pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1)
    want = [f.plan(ticks) for f in fleets]
    assert (want[0] != want[1]).any(axis=1)[2:].all()
    carries = [{b: oracle.update_carry(h) for b in range(n)} for _ in range(2)]
    cfg = pkg.make_config(fleets[0].p, h, warm_start=2)
    with pkg.Pipeline(cfg, n, 0, depth=2) as pipe:
        for t in range(ticks):
            qs = [f.tick(t) for f in fleets]
            outs = [dict(grf=np.zeros((n, 12)), iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32)) for _ in range(2)]
            for s in range(2):
                assert pipe.submit(qs[s]["x0"], qs[s]["xref"], qs[s]["R"], qs[s]["foot"], qs[s]["contact"], outs[s], slot=s, fresh=False) == s
            pipe.wait()
            for s in range(2):
                mode = C.c_int32(-9)
                assert pipe.lib.a1mpc_last_warm_start_mode(pipe.handle(s), C.byref(mode)) == 0 and mode.value == 2, (s, t, mode.value)
                _held(oracle, pr, st, qs[s], outs[s], np.arange(n), carries[s], want[s][t], ("pipeline slot", s, "tick", t))


def test_both_paths_reinitialise_on_the_same_ticks_of_a_step_invariant_sequence(pkg, oracle, scen):
    """the same QP sequence through a1mpc_solve_batch and through a1mpc_solve_batch_strided with the feet repeated over the horizon (foot_stride = 12): the same
    pattern, the same re-initialisation ticks, the same iteration counts, both held to the oracle"""
    n, h, ticks = 41, 10, 6
    fl = INTERPLAY["both-paths"].fleet(scen)
    sc = dict(horizon=h, params=fl.p); pr = oracle_params(oracle, sc); st = oracle.default_settings(warm_start=1)
    want = fl.plan(ticks); idx = np.arange(n)
    carries = [{b: oracle.update_carry(h) for b in range(n)} for _ in range(2)]
    with _engine(pkg, sc, n, warm_start=2) as fast, _engine(pkg, sc, n, warm_start=2) as gen:
        for t in range(ticks):
            q = fl.tick(t)
            qg = dict(q, foot=np.ascontiguousarray(np.tile(q["foot"], (1, h))), foot_stride=12)
            a = _solve(fast, q); b = _solve(gen, qg)
            assert fast.last_warm_start_mode() == 2 and gen.last_warm_start_mode() == 2
            _held(oracle, pr, st, q, a, idx, carries[0], want[t], ("fast", t))
            _held(oracle, pr, st, qg, b, idx, carries[1], want[t], ("general", t))
            assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"]), t
            assert np.abs(a["grf"] - b["grf"]).max() <= TOL_FORCE_N, t
