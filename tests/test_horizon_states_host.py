"""The predicted-horizon-states kernel on the CPU: the product's kernel text compiled for the host (tests/emu/horizon_states_host.py: 64 host threads in lock step are
one wavefront) against the yardsticks of tests/horizon_states_ref.py -- the shipped lane mapping, shuffles, LDS rows, chunks of steps, dead lanes and arithmetic, at the
bars of tests/test_gpu_horizon_states.py, which runs the same comparisons on the GPU (where cos / sin / the division are the device library's)."""
import os, sys
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import horizon_states_host as host
import horizon_states_ref as HS
from gpu_common import _strided_inputs


@pytest.mark.parametrize("h", [4, 10, 14, 20])
@pytest.mark.parametrize("n", [1, 67, 130])
def test_kernel_text_on_the_host_matches_the_longdouble_recurrence(scen, n, h):
    """a lone QP, a partly filled last wavefront, several workgroups; one, two and a half, three and a half and five chunks of steps; per-step feet, a yaw of its own:
    states within 1e-12 S, costs within 1e-12 of the abs-sum of their terms, x[12] copied, NaN-poisoned rows beyond n untouched"""
    rng = np.random.default_rng(100 * h + n)
    sc, feet, fs, _, _ = _strided_inputs(scen, rng, h, n, True, False)
    u = rng.uniform(-60.0, 180.0, (n, 12 * h)); yaw = sc["x0"][:, 2] + rng.uniform(-0.5, 0.5, n)
    xp, cost = host.run(sc["params"], h, sc["R"], feet, x0=sc["x0"], xref=sc["xref"], u=u, foot_stride=fs, yaw_A=yaw, rows=n + 20)
    assert np.isnan(xp[n:]).all() and np.isnan(cost[n:]).all() and not np.isnan(xp[:n]).any() and not np.isnan(cost[:n]).any()
    X, S = HS.rollout(sc["params"], h, sc["x0"], sc["R"], feet, fs, u, yaw)
    ratio = HS.states_ratio(xp[:n], X, S)
    cy = HS.costs(sc["params"], h, X, sc["xref"], u)
    q = np.asarray(sc["params"]["q"], np.float64)[:12]
    scale0 = (q * (S[..., :12] + np.abs(sc["xref"].reshape(n, h, 13)[..., :12])) ** 2).sum((1, 2))
    r0 = float((np.abs(cost[:n, 0] - cy[:, 0]) / scale0).max()); r1 = float((np.abs(cost[:n, 1] - cy[:, 1]) / cy[:, 1]).max())
    print(f"n {n} h {h}: worst |x_pred - X| / S = {ratio:.2e}; cost[0] {r0:.2e} of its abs-sum, cost[1] {r1:.2e} relative")
    assert ratio <= HS.BAR and r0 <= HS.BAR and r1 <= HS.BAR
    assert np.array_equal(xp[:n, :, 12], np.broadcast_to(sc["x0"][:, 12:13], (n, h)))


@pytest.mark.parametrize("h", [10, 16, 20])
def test_kernel_text_on_the_host_matches_the_reference_and_its_cost_identity(scen, h):
    """24 QPs against A_qp x0 + B_qp u and 1/2 u'Pu + g'u on the reference's A_qp / B_qp / hessian / gradient (oracle/_ref): broadcast and per-step feet; zero forces give
    cost[1] == 0 and the free response"""
    import ref as REF
    if not REF.build():
        pytest.skip("oracle/_ref not built and the reference sources are absent")
    n = 24
    rng = np.random.default_rng(900 + h)
    sc, feet, fs, _, _ = _strided_inputs(scen, rng, h, n, True, False)
    u = rng.uniform(-60.0, 180.0, (n, 12 * h))
    for foot, stride in ((sc["foot"], 0), (feet, fs)):
        ref = HS.reference_states(REF, sc["params"], h, sc["x0"], sc["xref"], sc["R"], foot, stride, sc["contact"], u)
        ref0 = HS.reference_states(REF, sc["params"], h, sc["x0"], sc["xref"], sc["R"], foot, stride, sc["contact"], None)
        xp, cost = host.run(sc["params"], h, sc["R"], foot, x0=sc["x0"], xref=sc["xref"], u=u, foot_stride=stride)
        xp0, cost0 = host.run(sc["params"], h, sc["R"], foot, x0=sc["x0"], xref=sc["xref"], u=None, foot_stride=stride)
        assert (cost0[:, 1] == 0.0).all()
        r, r0 = HS.states_ratio(xp, ref["X"], ref["S"]), HS.states_ratio(xp0, ref0["X"], ref0["S"])
        gap = float(HS.cost_gap(cost, cost0, ref["P"], ref["g"], u).max())
        print(f"h {h} foot_stride {stride}: states {r:.2e} (free response {r0:.2e}) of S, cost identity {gap:.2e} of its scale")
        assert r <= HS.BAR and r0 <= HS.BAR and gap <= HS.BAR


def test_kernel_text_structural_bit_equalities(oracle, scen):
    """foot_stride 12 with the same feet repeated == 0; yaw_A = x0[:, 2] == none; the first 40 rows of a 70-row call == a 40-row call; one output alone == both; the tick
    record's x_pred == the (x0, x_ref) form's, its cost within 1e-12 of the abs-sum of its terms of the cost with oracle.mpc_reference's x_ref"""
    n, h = 70, 10
    rng = np.random.default_rng(31)
    sc = scen.config3_random_flat(nb=n, horizon=h, seed=31)
    p, x0, xref, R, foot, tick = sc["params"], sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["tick"]
    u = rng.uniform(-60.0, 180.0, (n, 12 * h))
    xp, cost = host.run(p, h, R, foot, x0=x0, xref=xref, u=u)
    for other in (host.run(p, h, R, np.tile(foot, (1, h)), x0=x0, xref=xref, u=u, foot_stride=12), host.run(p, h, R, foot, x0=x0, xref=xref, u=u, yaw_A=x0[:, 2].copy())):
        assert np.array_equal(other[0], xp) and np.array_equal(other[1], cost)
    first = host.run(p, h, R[:40], foot[:40], x0=x0[:40], xref=xref[:40], u=u[:40])
    assert np.array_equal(first[0], xp[:40]) and np.array_equal(first[1], cost[:40])
    assert np.array_equal(host.run(p, h, R, foot, x0=x0, u=u, want_cost=False)[0], xp) and np.array_equal(host.run(p, h, R, foot, x0=x0, xref=xref, u=u, want_x=False)[1], cost)
    xt, ct = host.run(p, h, R, foot, tick=tick, u=u)
    xr_o = np.array([oracle.mpc_reference(h, p["dt"], tick[b, 0:3], tick[b, 3:6], R[b], tick[b, 12:15], tick[b, 15:18], tick[b, 18:21], tick[b, 21]) for b in range(n)])
    xe, ce = host.run(p, h, R, foot, x0=np.c_[tick[:, :12], np.full(n, -9.8)], xref=xr_o, u=u)
    assert np.array_equal(xt, xe) and np.array_equal(ct[:, 1], ce[:, 1])
    q = np.asarray(p["q"], np.float64)[:12]
    scale0 = (q * (np.abs(xe[..., :12]) + np.abs(xr_o.reshape(n, h, 13)[..., :12])) ** 2).sum((1, 2))
    assert float((np.abs(ct[:, 0] - ce[:, 0]) / scale0).max()) <= HS.BAR


def test_kernel_text_standing_robot_stays_where_it_is(scen):
    sc = scen.scenario_stand()
    h = sc["horizon"]
    u = np.tile([0.0, 0.0, sc["params"]["mass"] * 9.8 / 4.0], (1, 4 * h))
    xp, _ = host.run(sc["params"], h, sc["R"], sc["foot"], x0=sc["x0"], xref=sc["xref"], u=u)
    assert float(np.abs(xp - sc["x0"][:, None, :]).max()) <= 1e-15
