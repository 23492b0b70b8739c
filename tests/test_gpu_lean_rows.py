"""GPU, through the C ABI: the Riccati factor pass without the gain work of step 0 (RowSolver::factorize computes S_0^-1 alone at t = 0: K_0 is never used, there is no
P_0) on every kernel family that instantiates it, on inputs that make exact zeros and first products of either sign, vs the oracle: same iteration count and status on every
QP, forces within the parity tolerance of the suite (helpers.TOL_FORCE_N, TOL_FORCE_BALANCE_N for the balance QP).

Families are reached the way tests/test_gpu_settings_kernel_families.py reaches them -- by batch size, with a1mpc_last_stage_ms telling the split pipeline (it alone has a
set-up stage of its own) from the others: the few special QPs run alone (latency kernel) and again as the first AND the last rows of a fused-size and of a split-size
batch of random QPs with an odd count (so the last wavefront holds a lone QP, and it is one of the special ones).  The pipelines agree bit for bit on the rows they share
(DESIGN "Parity", tests/test_gpu_extended_horizons.py), which is asserted here too.

The special rows:  0  every leg in swing (every bound 0: the forces are 0 to the solver's tolerance);  1  a foot with zero coordinates, contacts 1001;  2  x0 equal to every reference state,
contacts 0111;  further rows: random states with mixed contact patterns (scenarios.config5_divergent: all 15 patterns)."""
import numpy as np
import pytest

from gpu_common import _engine
from helpers import TOL_FORCE_BALANCE_N, TOL_FORCE_N, compare, oracle_batch, oracle_params

pytestmark = pytest.mark.gpu

KEYS = ("u", "grf", "iters", "status")
FIELDS = ("x0", "xref", "R", "foot", "contact")


def _special(scen, h, n, seed):
    """n >= 3 QPs at horizon h: rows 0-2 as in the module docstring, the others random with mixed contact patterns"""
    sc = scen.config5_divergent(nb=n, seed=seed, horizon=h)
    sc["contact"][0] = 0
    sc["contact"][1] = [1, 0, 0, 1]; sc["foot"][1, 0] = 0.0; sc["foot"][1, 1] = 0.0; sc["foot"][1, 10] = 0.0
    sc["contact"][2] = [0, 1, 1, 1]; sc["xref"][2] = np.tile(sc["x0"][2], h)
    return sc


def _framed(scen, sp, n):
    """a batch of n QPs: the special rows `sp` first and last, random flat-terrain QPs in between"""
    k = len(sp["x0"]); h = sp["horizon"]
    sc = scen.config3_random_flat(nb=n, seed=7300 + h + n, horizon=h)
    for f in FIELDS:
        sc[f][:k] = sp[f]; sc[f][n - k:] = sp[f]
    return sc


def _solve(eng, sc, **kw):
    return eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True, **kw)


def _rows(out, idx):
    return {k: out[k][idx] for k in KEYS}


def _held(out, ref, what):
    r = compare(out, {k: ref[k] for k in KEYS}, tol=TOL_FORCE_N, min_same=1.0)
    print(what, r, "iterations", out["iters"].tolist()[:8])
    return r


def _families(pkg, oracle, scen, h, k, n_fused, n_split, seed):
    """the k special QPs alone, framing a fused-size batch and framing a split-size batch: each held to the oracle, the shared rows bit for bit"""
    sp = _special(scen, h, k, seed)
    ref = oracle_batch(oracle, sp)
    assert (ref["status"] == 1).all(), ref["status"]
    # every leg in swing: every force is held between bounds of 0, so it is the primal residual of its row -- below eps_abs = 1e-3 where OSQP stops (observed: 3e-6)
    assert np.abs(ref["grf"][0]).max() < 1e-3 and np.abs(ref["u"][0]).max() < 1e-3
    sizes = [n for n in (n_split, n_fused) if n is not None]
    outs = {}
    with _engine(pkg, sp, max(sizes), warm_start=0) as eng:
        outs[k] = _solve(eng, sp)
        assert eng.last_stage_ms()[0] == 0.0
        for n in sizes:
            sc = _framed(scen, sp, n)
            outs[n] = _solve(eng, sc)
            form_ms = eng.last_stage_ms()[0]
            assert (form_ms > 0.0) if n == n_split else (form_ms == 0.0), (h, n, form_ms)
            # the random rows in between: a sample against the oracle
            mid = dict(sc); idx = np.arange(k, min(n - k, k + 24))
            for f in FIELDS:
                mid[f] = sc[f][idx]
            _held(_rows(outs[n], idx), oracle_batch(oracle, mid), f"h{h} x {n}: rows {idx[0]}..{idx[-1]}")
    _held(outs[k], ref, f"h{h} x {k} (latency kernel)")
    assert np.abs(outs[k]["grf"][0]).max() < 1e-3 and np.abs(outs[k]["u"][0]).max() < 1e-3
    for n in sizes:
        for a, b in ((slice(0, k), "first"), (slice(n - k, n), "last")):
            got = _rows(outs[n], a)
            _held(got, ref, f"h{h} x {n} ({'split' if n == n_split else 'fused'}), {b} rows")
            for key in KEYS:
                assert np.array_equal(got[key], outs[k][key]), (h, n, b, key)


def test_three_qps_h10_on_every_kernel_family(pkg, oracle, scen):
    """n = 3 at h = 10 (one wavefront with a pair and a lone QP) on the latency kernel, and the same three QPs framing 1501 (fused kernel) and 3001 (set-up kernel +
    persistent rows) QPs"""
    _families(pkg, oracle, scen, 10, 3, 1501, 3001, 7110)


@pytest.mark.parametrize("h,n_fused,n_split", [(4, 601, 3001), (16, 701, 1501), (20, 301, 1301)], ids=lambda v: str(v))
def test_five_qps_at_the_smallest_horizon_the_cu_wide_kernel_and_the_quads(pkg, oracle, scen, h, n_fused, n_split):
    """n = 5 at h = 4 (the smallest horizon: step 0 is a quarter of the factor pass), h = 16 (fused quads; the CU-wide persistent workgroup at 1501) and h = 20 (the quads
    of rows at 1301)"""
    _families(pkg, oracle, scen, h, 5, n_fused, n_split, 7100 + h)


@pytest.mark.parametrize("n_frame", [None, 1501, 3001], ids=["latency", "fused", "split"])
def test_a_nan_input_returns_zeros_and_the_error_status_h10(pkg, scen, n_frame):
    """one QP of the three with a NaN in x0: NON_CVX (-7) and zero GRFs for it, every other row bit for bit what the batch gives without the NaN"""
    sp = _special(scen, 10, 3, 7110)
    sc = sp if n_frame is None else _framed(scen, sp, n_frame)
    n = len(sc["x0"])
    bad = dict(sc); bad["x0"] = sc["x0"].copy(); bad["x0"][1, 4] = np.nan; bad["x0"][n - 1, 7] = np.nan
    isbad = np.zeros(n, bool); isbad[[1, n - 1]] = True
    with _engine(pkg, sc, n, warm_start=0) as eng:
        a = _solve(eng, bad)
        clean = _solve(eng, sc)
    assert (a["status"][isbad] == -7).all() and not a["grf"][isbad].any(), (a["status"][isbad], a["grf"][isbad])
    assert (clean["status"] == 1).all()
    for k in KEYS:
        assert np.array_equal(a[k][~isbad], clean[k][~isbad]), k


def test_four_balance_qps(pkg, oracle, scen):
    """H = 1, where step 0 is the only step of the factor pass: four contacts, a mixed pattern, a foot with zero coordinates, and a NaN root_acc (NON_CVX, zero GRFs)"""
    n = 4
    sc = scen.balance_random(n, seed=7400)
    sc["contact"][0] = 1; sc["contact"][1] = [1, 0, 1, 1]; sc["contact"][2] = 1
    sc["foot"][2, 0] = 0.0; sc["foot"][2, 4] = 0.0
    acc = sc["root_acc"].copy(); acc[3, 2] = np.nan
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, 10)
    with pkg.Engine(cfg, 64, 0) as eng:
        out = eng.balance_solve(acc, sc["R"], sc["Rz"], sc["foot"], sc["contact"])
    qp, st = oracle.default_qp_params(), oracle.default_settings()
    assert out["status"][3] == -7 and not out["grf"][3].any(), out["status"][3]
    for b in range(3):
        r = oracle.balance_solve(qp, st, sc["root_acc"][b], sc["R"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
        d = max(np.abs(out["f_world"][b] - r["f_world"]).max(), np.abs(out["grf"][b] - r["grf"]).max())
        print("balance QP", b, "iterations", out["iters"][b], r["info"].iters, "distance", d)
        assert out["iters"][b] == r["info"].iters and out["status"][b] == r["info"].status, b
        assert d < TOL_FORCE_BALANCE_N, (b, d)


def test_a_warm_started_second_tick_h10(pkg, oracle, scen):
    """warm_start = 1, two ticks of the three special QPs (the second from slightly moved states: its first factor pass starts from the carried rho): every QP of either tick
    stops where the oracle's chained solver stops, with its status and forces"""
    h, n = 10, 3
    sp = _special(scen, h, n, 7110)
    pr = oracle_params(oracle, sp); st = oracle.default_settings(warm_start=1)
    wx = [np.zeros(12 * h) for _ in range(n)]; wy = [np.zeros(20 * h) for _ in range(n)]; rho = [None] * n
    rng = np.random.default_rng(7500)
    with _engine(pkg, sp, n, warm_start=1) as eng:
        for t in range(2):
            if t > 0:
                sp["x0"][:, :12] += rng.normal(0, 2e-3, (n, 12))
            out = _solve(eng, sp)
            for b in range(n):
                o = oracle.mpc_solve(pr, st, sp["x0"][b], sp["xref"][b], sp["R"][b], sp["foot"][b], sp["contact"][b], warm_x=wx[b], warm_y=wy[b], warm_rho=rho[b])
                wx[b], wy[b], rho[b] = o["warm_x"], o["warm_y"], o["rho"]
                d = max(np.abs(out["u"][b] - o["u"]).max(), np.abs(out["grf"][b] - o["grf"]).max())
                print("tick", t, "QP", b, "iterations", out["iters"][b], o["info"].iters, "distance", d)
                assert out["iters"][b] == o["info"].iters and out["status"][b] == o["info"].status, (t, b)
                assert d <= TOL_FORCE_N, (t, b, d)
