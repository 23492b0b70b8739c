"""GPU: a1mpc_horizon_states_batch(_device) / a1mpc_horizon_states_ticks_batch(_device) -- the predicted states of a force plan over the horizon and its cost.
Yardsticks (tests/horizon_states_ref.py; the kernel is never compared with itself): the reference's own A_qp / B_qp / hessian / gradient (S/ConvexMpc.cpp compiled verbatim,
oracle/_ref), the oracle, and the recurrence restated in numpy.longdouble, which tests/test_horizon_states_abi.py pins to the reference at h = 10 / 16 / 20.
Bars, both 1e-12 and both relative to the sum of the absolute values of the accumulated terms (cancellation does not enter):
  states  |x_pred - X| <= 1e-12 S componentwise, S = |A_qp||x0| + |B_qp||u| (the same sum accumulated step by step for the recurrence yardstick)
  cost    |cost[0](u) + cost[1](u) - cost[0](0) - (1/2 u'Pu + g'u)| <= 1e-12 (cost[0](u) + cost[0](0) + cost[1](u) + 1/2 |u|'|P||u| + |g|'|u|)
The yardsticks themselves agree within 3.5e-16 S (states) and 2.9e-16 of the scale (cost identity on the reference's P, g): more than three orders inside the bars; a
wrong index, sign, step offset or leg order misses them by ten orders or more."""
import ctypes as C

import numpy as np
import pytest

import horizon_states_ref as HS
from gpu_common import _engine, _strided_inputs
from helpers import MIN_SAME_ITERS, TOL_FORCE_N, compare, oracle_batch, oracle_params

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _forces(rng, n, h):
    return rng.uniform(-60.0, 180.0, (n, 12 * h))   # not a solution: every block of B_qp carries weight


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.mark.parametrize("h", [10, 16, 20])
def test_states_equal_the_reference_A_qp_x0_plus_B_qp_u(pkg, scen, h):
    """48 QPs, foot_stride 0 and 12, yaw_A None and a per-QP yaw different from x0[2], forces uniform in [-60, 180] N: within the states bar of A_qp x0 + B_qp u on the
    A_qp / B_qp of REF.convex_mpc_form; x_pred[..., 12] == x0[12] exactly."""
    import ref as REF
    if not REF.build():
        pytest.skip("oracle/_ref not available")
    n = 48
    rng = np.random.default_rng(4100 + h)
    sc, feet, fs, _, _ = _strided_inputs(scen, rng, h, n, True, False)
    u = _forces(rng, n, h); yaw = sc["x0"][:, 2] + rng.uniform(0.1, 0.6, n) * rng.choice([-1.0, 1.0], n)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        for foot, stride in ((sc["foot"], 0), (feet, fs)):
            for ya in (None, yaw):
                out = eng.horizon_states(sc["x0"], sc["R"], foot, u=u, foot_stride=stride, yaw_A=ya)
                ref = HS.reference_states(REF, sc["params"], h, sc["x0"], sc["xref"], sc["R"], foot, stride, sc["contact"], u, ya)
                ratio = HS.states_ratio(out["x_pred"], ref["X"], ref["S"])
                print(f"h {h} foot_stride {stride} yaw_A {'own' if ya is not None else 'x0[2]'}: worst |x_pred - (A_qp x0 + B_qp u)| / S = {ratio:.2e}")
                assert out["cost"] is None
                assert ratio <= HS.BAR, (h, stride, ya is not None, ratio)
                assert np.array_equal(out["x_pred"][..., 12], np.broadcast_to(sc["x0"][:, 12:13], (n, h)))


_ENGINES = {}


@pytest.fixture(scope="module")
def big_engine(pkg, scen):
    """one handle per horizon for the ragged sizes (max_batch 5000)"""
    def get(h):
        if h not in _ENGINES:
            _ENGINES[h] = _engine(pkg, scen.config3_random_flat(nb=1, horizon=h), 5000, warm_start=0)
        return _ENGINES[h]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


@pytest.mark.parametrize("h", [4, 10, 14, 20])
@pytest.mark.parametrize("n", [1, 67, 5000])
def test_every_qp_at_ragged_sizes(pkg, scen, big_engine, n, h):
    """n = 1 (a lone QP), 67 (a partly filled last wavefront), 5000 (many workgroups and a ragged tail) at four horizons (one, two and a half, three and a half and five
    chunks of steps), per-step feet, a yaw of its own, both outputs: every QP within the states bar of the longdouble recurrence and its cost within 1e-12 of the recurrence's
    (relative to the abs-sum of the squares' terms).  The outputs are device arrays of n + 64 rows poisoned with NaN: no NaN inside n, nothing written beyond n."""
    import torch
    rng = np.random.default_rng(100 * h + n)
    sc, feet, fs, _, _ = _strided_inputs(scen, rng, h, n, True, False)
    u = _forces(rng, n, h); yaw = sc["x0"][:, 2] + rng.uniform(-0.5, 0.5, n)
    eng = big_engine(h)
    xp = torch.full((n + 64, h * 13), float("nan"), dtype=torch.float64, device=_dev()); cost = torch.full((n + 64, 2), float("nan"), dtype=torch.float64, device=_dev())
    eng.horizon_states_device(n, _t(sc["x0"]), _t(sc["xref"]), _t(sc["R"]), _t(feet), fs, _t(u), xp, cost, d_yaw_A=_t(yaw))
    torch.cuda.synchronize()
    xp, cost = xp.cpu().numpy(), cost.cpu().numpy()
    assert np.isnan(xp[n:]).all() and np.isnan(cost[n:]).all(), "written beyond n"
    assert not np.isnan(xp[:n]).any() and not np.isnan(cost[:n]).any()
    X, S = HS.rollout(sc["params"], h, sc["x0"], sc["R"], feet, fs, u, yaw)
    ratio = HS.states_ratio(xp[:n].reshape(n, h, 13), X, S)
    # the cost against the yardstick trajectory's: a sum of squares q (x - x_ref)^2, whose accumulated terms are bounded by q (|x| + |x_ref|)^2 -- S bounds |x|
    cy = HS.costs(sc["params"], h, X, sc["xref"], u)
    q = np.asarray(sc["params"]["q"], np.float64)[:12]
    scale0 = (q * (S[..., :12] + np.abs(sc["xref"].reshape(n, h, 13)[..., :12])) ** 2).sum((1, 2))
    r0 = float((np.abs(cost[:n, 0] - cy[:, 0]) / scale0).max()); r1 = float((np.abs(cost[:n, 1] - cy[:, 1]) / cy[:, 1]).max())
    print(f"n {n} h {h}: worst |x_pred - X| / S = {ratio:.2e}; cost[0] {r0:.2e} of its abs-sum, cost[1] {r1:.2e} relative")
    assert ratio <= HS.BAR and r0 <= HS.BAR and r1 <= HS.BAR, (n, h, ratio, r0, r1)
    assert np.array_equal(xp[:n].reshape(n, h, 13)[..., 12], np.broadcast_to(sc["x0"][:, 12:13], (n, h)))


def _perturbations(rng, sc, u, h, fz_max, k=8):
    """k feasible neighbours of every plan: each stance force of a random half of the (step, leg) pairs pulled 1 % towards (0, 0, fz_max / 2) -- a convex combination of the
    plan with a point strictly inside pyramid and box, so it stays inside both; swing legs keep their zero force"""
    n = len(u)
    stance = np.broadcast_to(sc["contact"].reshape(n, 1, 4, 1).astype(bool), (n, h, 4, 3))
    centre = np.array([0.0, 0.0, fz_max / 2.0])
    out = []
    for _ in range(k):
        pick = rng.random((n, h, 4, 1)) < 0.5
        pick[:, 0] = True                                # (never empty)
        uu = u.reshape(n, h, 4, 3)
        out.append(np.where(stance & pick, uu + 0.01 * (centre - uu), uu).reshape(n, 12 * h))
    return out


@pytest.mark.parametrize("h", [4, 10, 16, 20])
def test_cost_identity_and_the_solved_plan_is_cheapest(pkg, oracle, scen, h):
    """16 QPs.  cost[0](u) + cost[1](u) - cost[0](0) = 1/2 u'Pu + g'u within the cost bar, on the reference's hessian / gradient (h = 10, 16, 20) or the oracle's (h = 4),
    at the engine's own solution and at random forces.  u_full = None: cost[1] == 0 exactly and x_pred is the free response A_qp x0 within the states bar."""
    n = 16
    rng = np.random.default_rng(4300 + h)
    sc = scen.config3_random_flat(nb=n, horizon=h, seed=4300 + h)
    p = sc["params"]
    if h == 4:
        pr = oracle_params(oracle, sc)
        forms = [oracle.mpc_form(pr, sc["x0"][b], sc["xref"][b], sc["R"][b], sc["foot"][b], sc["contact"][b]) for b in range(n)]
        P = np.array([f[0] for f in forms]); g = np.array([f[1] for f in forms])
        X0, S0 = HS.rollout(p, h, sc["x0"], sc["R"], sc["foot"], 0, None)
    else:
        import ref as REF
        if not REF.build():
            pytest.skip("oracle/_ref not available")
        ref = HS.reference_states(REF, p, h, sc["x0"], sc["xref"], sc["R"], sc["foot"], 0, sc["contact"], None)
        P, g, X0, S0 = ref["P"], ref["g"], ref["X"], ref["S"]
    with _engine(pkg, sc, n, warm_start=0) as eng:
        sol = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
        assert (sol["status"] == 1).all()
        free = eng.horizon_states(sc["x0"], sc["R"], sc["foot"], u=None, xref=sc["xref"])
        assert (free["cost"][:, 1] == 0.0).all()
        r_free = HS.states_ratio(free["x_pred"], X0, S0)
        print(f"h {h}: free response, worst |x_pred - A_qp x0| / S = {r_free:.2e}")
        assert r_free <= HS.BAR
        plans = {"solved": sol["u"], "random": _forces(rng, n, h)}
        cost = {k: eng.horizon_states(sc["x0"], sc["R"], sc["foot"], u=v, xref=sc["xref"])["cost"] for k, v in plans.items()}
        near = [eng.horizon_states(sc["x0"], sc["R"], sc["foot"], u=v, xref=sc["xref"])["cost"] for v in _perturbations(rng, sc, sol["u"], h, p["fz_max"])]
        eps_rel = float(eng.cfg.eps_rel)
    for k, v in plans.items():
        gap = HS.cost_gap(cost[k], free["cost"], P, g, v)
        print(f"h {h} {k} plan: worst cost-identity gap {float(gap.max()):.2e} of its scale")
        assert (gap <= HS.BAR).all(), (h, k, float(gap.max()))
    # The solved plan is no dearer than any of its 8 feasible neighbours.  Slack eps_rel x the cost: the solve is converged to OSQP's default tolerance only, so the
    # returned plan may sit that far (relatively) above the optimum that a neighbour can undercut it by
    total = cost["solved"].sum(1)
    worst = max(float(((total - c.sum(1)) / c.sum(1)).max()) for c in near)
    print(f"h {h}: (cost(solved) - cost(neighbour)) / cost(neighbour) at most {worst:.2e} (allowed {eps_rel:.0e})")
    for c in near:
        assert (total <= c.sum(1) * (1.0 + eps_rel)).all(), (h, worst)


@pytest.mark.parametrize("h", [10, 16])
def test_structural_bit_equalities(pkg, oracle, scen, h):
    """n = 300: host entry == device entry; foot_stride 12 with the same feet repeated == foot_stride 0; yaw_A = x0[:, 2] == None; the ticks entry's x_pred == the
    (x0, x_ref) entry's with x0 = [tick[:12], -9.8]; the ticks entry's cost within the cost bar of the cost with oracle.mpc_reference's x_ref; the first 100 rows of a 300-row
    call == a 100-row call."""
    import torch
    n = 300
    rng = np.random.default_rng(4400 + h)
    sc = scen.config3_random_flat(nb=n, horizon=h, seed=4400 + h)
    u = _forces(rng, n, h)
    x0, xref, R, foot, tick = sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["tick"]
    with _engine(pkg, sc, n, warm_start=0) as eng:
        host = eng.horizon_states(x0, R, foot, u=u, xref=xref)
        xp = torch.zeros((n, h * 13), dtype=torch.float64, device=_dev()); co = torch.zeros((n, 2), dtype=torch.float64, device=_dev())
        eng.horizon_states_device(n, _t(x0), _t(xref), _t(R), _t(foot), 0, _t(u), xp, co)
        torch.cuda.synchronize()
        assert np.array_equal(xp.cpu().numpy().reshape(n, h, 13), host["x_pred"]) and np.array_equal(co.cpu().numpy(), host["cost"])
        rep = eng.horizon_states(x0, R, np.tile(foot, (1, h)), u=u, xref=xref, foot_stride=12)
        assert np.array_equal(rep["x_pred"], host["x_pred"]) and np.array_equal(rep["cost"], host["cost"])
        own = eng.horizon_states(x0, R, foot, u=u, xref=xref, yaw_A=x0[:, 2].copy())
        assert np.array_equal(own["x_pred"], host["x_pred"]) and np.array_equal(own["cost"], host["cost"])
        first = eng.horizon_states(x0[:100], R[:100], foot[:100], u=u[:100], xref=xref[:100])
        assert np.array_equal(first["x_pred"], host["x_pred"][:100]) and np.array_equal(first["cost"], host["cost"][:100])
        # tick records: x0 = [tick[:12], -9.8]; x_ref as S/A1RobotControl.cpp:470-488 builds it
        x0t = np.c_[tick[:, :12], np.full(n, -9.8)]
        tk = eng.horizon_states_ticks(tick, R, foot, u=u)
        tk_dev_x = torch.zeros((n, h * 13), dtype=torch.float64, device=_dev()); tk_dev_c = torch.zeros((n, 2), dtype=torch.float64, device=_dev())
        eng.horizon_states_ticks_device(n, _t(tick), _t(R), _t(foot), 0, _t(u), tk_dev_x, tk_dev_c)
        torch.cuda.synchronize()
        assert np.array_equal(tk_dev_x.cpu().numpy().reshape(n, h, 13), tk["x_pred"]) and np.array_equal(tk_dev_c.cpu().numpy(), tk["cost"])
        assert eng.horizon_states_ticks(tick, R, foot, u=u, want_cost=False)["cost"] is None
        xr_o = np.array([oracle.mpc_reference(h, sc["params"]["dt"], tick[b, 0:3], tick[b, 3:6], R[b], tick[b, 12:15], tick[b, 15:18], tick[b, 18:21], tick[b, 21]) for b in range(n)])
        ex = eng.horizon_states(x0t, R, foot, u=u, xref=xr_o)
        # refusals that need a live handle (A1MPC_ERR_INVALID_ARGUMENT = 1, the argument named)
        L, H_, dp = eng.lib, eng._h, lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        o13, o2 = np.zeros((n, h * 13)), np.zeros((n, 2))
        for args, word in (((n + 1, dp(x0), dp(xref), dp(R), dp(foot), 0, None, dp(u), dp(o13), dp(o2)), b"max_batch"),
                           ((n, dp(x0), dp(xref), dp(R), dp(foot), 0, None, dp(u), None, None), b"both null"),
                           ((n, dp(x0), None, dp(R), dp(foot), 0, None, dp(u), dp(o13), dp(o2)), b"x_ref"),
                           ((n, None, dp(xref), dp(R), dp(foot), 0, None, dp(u), dp(o13), dp(o2)), b"x0"),
                           ((n, dp(x0), dp(xref), None, dp(foot), 0, None, dp(u), dp(o13), dp(o2)), b"R_world"),
                           ((n, dp(x0), dp(xref), dp(R), None, 0, None, dp(u), dp(o13), dp(o2)), b"foot_abs"),
                           ((n, dp(x0), dp(xref), dp(R), dp(foot), 6, None, dp(u), dp(o13), dp(o2)), b"foot_stride")):
            assert L.a1mpc_horizon_states_batch(H_, *args) == 1 and word in L.a1mpc_last_error(), (word, L.a1mpc_last_error())
        assert L.a1mpc_horizon_states_batch(H_, 0, None, None, None, None, 0, None, None, dp(o13), None) == 1      # (n == 0 does not excuse a null input)
        assert L.a1mpc_horizon_states_batch(H_, 0, dp(x0), dp(xref), dp(R), dp(foot), 0, None, dp(u), dp(o13), dp(o2)) == 0 and not o13.any()
    assert np.array_equal(tk["x_pred"], ex["x_pred"])
    # the two x_ref differ by the rounding of base + (slope dt)(t + 1): the cost is held to the abs-sum of its terms, q (|x| + |x_ref|)^2 summed
    q = np.asarray(sc["params"]["q"], np.float64)[:12]
    scale0 = (q * (np.abs(ex["x_pred"][..., :12]) + np.abs(xr_o.reshape(n, h, 13)[..., :12])) ** 2).sum((1, 2))
    r0 = float((np.abs(tk["cost"][:, 0] - ex["cost"][:, 0]) / scale0).max())
    print(f"h {h}: ticks cost[0] vs the cost with oracle.mpc_reference's x_ref: {r0:.2e} of its abs-sum")
    assert r0 <= HS.BAR and np.array_equal(tk["cost"][:, 1], ex["cost"][:, 1])
    with _engine(pkg, scen.config3_random_flat(nb=1, horizon=1), 4, warm_start=0) as e1:      # a handle of horizon 1 is refused
        z = np.zeros(13 * 4)
        assert e1.lib.a1mpc_horizon_states_batch(e1._h, 1, dp(z), dp(z), dp(z), dp(z), 0, None, None, dp(z), None) == 1 and b"horizon" in e1.lib.a1mpc_last_error()


def test_standing_robot_with_its_weight_on_four_feet_stays_where_it_is(pkg, scen):
    """scenario_stand with u = m 9.8 / 4 on every foot's z at every step: x_pred equals x0 at every step within 1e-15 absolute (a handful of roundings of 9.8 dt; the
    symmetric feet cancel the torque exactly)."""
    sc = scen.scenario_stand()
    h = sc["horizon"]; m = sc["params"]["mass"]
    u = np.tile([0.0, 0.0, m * 9.8 / 4.0], (1, 4 * h))
    with _engine(pkg, sc, 1, warm_start=0) as eng:
        out = eng.horizon_states(sc["x0"], sc["R"], sc["foot"], u=u, xref=sc["xref"])
    d = float(np.abs(out["x_pred"] - sc["x0"][:, None, :]).max())
    print(f"stand: worst |x_pred - x0| = {d:.2e}")
    assert d <= 1e-15


def test_closed_loop_that_never_leaves_the_device(pkg, oracle, scen):
    """64 robots, h = 10, cold starts, 30 ticks on one stream: solve_device -> horizon_states_device -> x0 <- x_pred[:, 0, :] by a device copy, x_ref / R / feet / contacts
    fixed, every tick's x0 and u_full kept in device history tensors, all 30 ticks enqueued before the one synchronisation.  Then, tick by tick: forces, iterations and status
    against the oracle on that tick's x0 (helpers.compare: MIN_SAME_ITERS, TOL_FORCE_N), and the next x0 within the states bar of the longdouble recurrence applied to that
    tick's x0 and the GPU's u.  Input condition, on the yardstick's trajectory: at least half the robots move by >= 1e-3 m (else a kernel returning x0 would pass)."""
    import torch
    n, h, ticks = 64, 10, 30
    sc = scen.config3_random_flat(nb=n, horizon=h, seed=4600)
    dev = _dev()
    xref, R, foot, contact = _t(sc["xref"]), _t(sc["R"]), _t(sc["foot"]), _t(sc["contact"])
    x_hist = torch.zeros((ticks + 1, n, 13), dtype=torch.float64, device=dev); x_hist[0] = _t(sc["x0"])
    u_hist = torch.zeros((ticks, n, 12 * h), dtype=torch.float64, device=dev); grf_hist = torch.zeros((ticks, n, 12), dtype=torch.float64, device=dev)
    it_hist = torch.zeros((ticks, n), dtype=torch.int32, device=dev); st_hist = torch.zeros((ticks, n), dtype=torch.int32, device=dev)
    x_pred = torch.zeros((n, h, 13), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _engine(pkg, sc, n, warm_start=0) as eng:
        for t in range(ticks):
            eng.solve_device(n, x_hist[t], xref, R, foot, contact, grf_hist[t], u_hist[t], it_hist[t], st_hist[t], stream=stream.cuda_stream)
            eng.horizon_states_device(n, x_hist[t], xref, R, foot, 0, u_hist[t], x_pred, stream=stream.cuda_stream)
            with torch.cuda.stream(stream):
                x_hist[t + 1].copy_(x_pred[:, 0, :])
        torch.cuda.synchronize()
    xs, us = x_hist.cpu().numpy(), u_hist.cpu().numpy()
    grf, its, sts = grf_hist.cpu().numpy(), it_hist.cpu().numpy(), st_hist.cpu().numpy()
    yard = sc["x0"].astype(LD); worst = 0.0
    for t in range(ticks):
        sct = dict(sc, x0=np.ascontiguousarray(xs[t]))
        compare(dict(grf=grf[t], u=us[t], iters=its[t], status=sts[t]), oracle_batch(oracle, sct), tol=TOL_FORCE_N, min_same=MIN_SAME_ITERS)
        X, S = HS.rollout(sc["params"], h, xs[t], sc["R"], sc["foot"], 0, us[t], steps=1)
        ratio = HS.states_ratio(xs[t + 1][:, None, :], X, S); worst = max(worst, ratio)
        assert ratio <= HS.BAR, (t, ratio)
        yard = HS.rollout(sc["params"], h, yard.astype(np.float64), sc["R"], sc["foot"], 0, us[t], steps=1)[0][:, 0]
    moved = np.linalg.norm((yard[:, 3:6] - sc["x0"][:, 3:6]).astype(np.float64), axis=1)
    print(f"closed loop: worst |x0(t+1) - yardstick| / S = {worst:.2e}; {int((moved >= 1e-3).sum())} of {n} robots moved >= 1 mm (median {np.median(moved):.3e} m)")
    assert (moved >= 1e-3).sum() >= n // 2
