"""CPU: every yardstick and every host-executable kernel text on a GENERIC set of robot constants (gpu_common.GENERIC_CONSTANTS: a full inertia_body, weight on x / y
position, twelve different r) -- the ground tests/test_gpu_generic_constants.py stands on.  All five scenarios.PARAM_SETS have a diagonal inertia, q[3] = q[4] = 0 and r
repeated over lanes, so a kernel that reads a wrong pair of inertia words, swaps or drops q[3] / q[4], indexes r by leg or is handed the diagonal only passes every other
test of the suite.

1. the oracle alone against its 80-bit build (tests/x87.py) on the batches the GPU file solves: same iteration on every QP, and the share of QPs further than TOL_FORCE_N
   apart within the cap gpu_common.held_to_oracle grants the case -- so a QP the GPU file settles by x87 is settled inside a cap the yardstick meets by itself;
2. every generic_variants() entry moves the oracle's forces by more than 100 x TOL_FORCE_N on at least half of a batch;
3. the oracle's formation against the reference's ConvexMpc compiled verbatim (oracle/_ref), the bars of tests/test_ref_pin.py's GPU counterpart;
4. the solver text on host fibers (tests/emu) against the oracle, bar 1e-8, same iteration, status and factor passes on every QP; the Ruiz sweep's early stop exact;
5. the host-compiled caller-side kernel texts against their numpy restatements, each with the comparison its own host test uses.
The balance QP has weights of its own: tests/test_balance_constants_host.py is this file's counterpart for them."""
import numpy as np
import pytest

import emu
import ground_ref as GR
import horizon_states_host
import horizon_states_ref as HS
import plant_host
import plant_ref as PR
import sensor_synthesis_host
import sensor_synthesis_ref as SR
import walk_ref as WR
import walk_step_ground_host
import walk_step_host
from gpu_common import (GENERIC_CONSTANTS, GENERIC_FAST_CASES, assert_batch_is_sensitive, assert_sensitive, generic_case_id, generic_params, generic_scenario,
                        generic_strided, generic_variants, generic_warm_ticks, oracle_sample, oracle_strided, oracle_warm_chain, split_case, yardstick_alone)
from helpers import compare, oracle_batch, oracle_params
from test_gpu_settings_kernel_families import FAST_SHAPES, GEN_SHAPES_H10, _x87_cold

GEN_SHAPES = GEN_SHAPES_H10 + [(20, 1700, "split")]
KEYS = ("u", "grf", "iters", "status")


def test_the_set_is_what_its_recipe_says():
    """GENERIC_CONSTANTS' inertia is Rr diag(I_gazebo) Rr' of the recipe (its eigenvalues are the gazebo set's, it is symmetric, no entry is zero), r[k] = 1e-7 (1 + k / 4),
    q[3], q[4] > 0 and different, q[6], q[7], q[8] different; every variant differs from the set in exactly the one property it names"""
    G = GENERIC_CONSTANTS
    v = np.array([-0.2405794275760342, -0.39730769868844346, -0.07450848662857455]); th = np.linalg.norm(v); a = v / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rr = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    I = Rr @ np.diag([0.0158533, 0.0377999, 0.0456542]) @ Rr.T
    Ig = np.array(G["inertia"]).reshape(3, 3)
    assert np.abs(Ig - (I + I.T) / 2).max() <= 1e-17 and np.array_equal(Ig, Ig.T) and (np.abs(Ig) > 1e-4).all()
    assert np.abs(np.linalg.eigvalsh(Ig) - [0.0158533, 0.0377999, 0.0456542]).max() <= 1e-15
    assert np.array_equal(G["r"], 1e-7 * (1 + np.arange(12) / 4)) and len(set(G["r"])) == 12
    assert G["q"][3] > 0 and G["q"][4] > 0 and G["q"][3] != G["q"][4] and len({G["q"][6], G["q"][7], G["q"][8]}) == 3 and G["mass"] == 11.3
    V = generic_variants()
    assert len(V) == 7 and all(len(var) == 1 and not np.array_equal(var[k], G[k]) for var in V.values() for k in var)


# ------------------------------------------------------------------------------------------------ 1. the yardstick alone, on the GPU file's batches
@pytest.mark.parametrize("h,n_fused,n_split", FAST_SHAPES + [(4, None, 96)], ids=lambda v: str(v))
@pytest.mark.parametrize("case", GENERIC_FAST_CASES, ids=generic_case_id)
def test_oracle_and_x87_agree_on_the_fast_path_batches(oracle, scen, case, h, n_fused, n_split):
    """96 QPs spread over the batch test_fast_path_cold solves at this horizon and case (the first and the last among them), and 96 of an h = 4 batch"""
    osqp, par = split_case(case)
    sc = generic_scenario(scen, h, n_split, **par)
    idx = oracle_sample(n_split, 96)
    ref = oracle_strided(oracle, oracle_params(oracle, sc), oracle.default_settings(**osqp), sc, sc["foot"], 0, sc["contact"], 0, idx)
    x = _x87_cold(sc, h, osqp)
    yardstick_alone(f"fast path h{h} x {n_split}", ref, lambda j: x(int(idx[j])), case)


@pytest.mark.parametrize("h,n,kernel", GEN_SHAPES, ids=lambda v: str(v))
def test_oracle_and_x87_agree_on_the_general_path_batches(oracle, scen, h, n, kernel):
    """the 96 QPs test_general_path holds at this shape: per-step feet and a contact schedule"""
    sc, foot, fs, contact, cs = generic_strided(scen, h, n)
    idx = oracle_sample(n, 96)
    ref = oracle_strided(oracle, oracle_params(oracle, sc), oracle.default_settings(), sc, foot, fs, contact, cs, idx)
    x = _x87_cold(sc, h, {}, foot, fs, contact, cs)
    yardstick_alone(f"general path h{h} x {n}", ref, lambda j: x(int(idx[j])), {})


@pytest.mark.parametrize("mode", [1, 2])
def test_oracle_and_x87_agree_on_the_warm_started_ticks(oracle, scen, mode):
    """the four ticks of test_warm_starts, every robot chained through the oracle; x87 starts each tick from the state the oracle's solve started from"""
    import x87
    for t, (ref, x87_solve) in enumerate(oracle_warm_chain(oracle, x87, generic_warm_ticks(scen), mode, 10)):
        yardstick_alone(f"warm_start = {mode}, h10 x 64, tick {t}", ref, x87_solve, {})


# ------------------------------------------------------------------------------------------------ 2. sensitivity
@pytest.mark.parametrize("h", [10, 20])
def test_every_variant_moves_the_oracles_forces(oracle, scen, h):
    """96 QPs of generic_scenario: each of the seven one-property reversions moves the forces by more than 100 x TOL_FORCE_N on at least half of them"""
    sc = generic_scenario(scen, h, 96)
    ref = oracle_batch(oracle, sc)
    assert_batch_is_sensitive(f"h{h} x 96", oracle, sc, np.arange(96), ref["u"])


# ------------------------------------------------------------------------------------------------ 3. the oracle's formation against the reference
@pytest.mark.parametrize("h", [10, 16, 20])
def test_oracle_formation_equals_reference_ConvexMpc(oracle, scen, h):
    """6 QPs, broadcast and per-step feet: P within 1e-12 and g within 1e-10 of S/ConvexMpc.cpp's, relative to the largest entry; l and u equal"""
    import ref as REF
    if not REF.build():
        pytest.skip("oracle/_ref not available")
    nb = 6
    sc, foot, fs, _, _ = generic_strided(scen, h, nb)
    p = sc["params"]; pr = oracle_params(oracle, sc)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    worst = [0.0, 0.0]
    for b in range(nb):
        for f, fstr in ((sc["foot"][b], 0), (foot[b], 12)):
            P, g, A, l, u, _ = oracle.mpc_form(pr, sc["x0"][b], sc["xref"][b], sc["R"][b], f, sc["contact"][b], foot_stride=fstr)
            r = REF.convex_mpc_form(h, p["q"], p["r"], sc["x0"][b][:3], p["mass"], p["inertia"], sc["R"][b], f, sc["contact"][b], sc["x0"][b], sc["xref"][b], p["dt"],
                                    foot_stride=fstr)
            worst = [max(worst[0], rel(P, r["P"])), max(worst[1], rel(g, r["g"]))]
            assert rel(P, r["P"]) <= 1e-12 and rel(g, r["g"]) <= 1e-10, (b, fstr, worst)
            assert np.array_equal(l, r["l"]) and np.array_equal(u, r["u"]) and np.array_equal(A, r["A"])
    print(f"h {h}: oracle vs reference ConvexMpc, P {worst[0]:.1e}, g {worst[1]:.1e} relative")


# ------------------------------------------------------------------------------------------------ 4. the solver text on host fibers
def _held(out, ref):
    assert (out["nfact"] == ref["nfact"]).all(), (out["nfact"], ref["nfact"])
    r = compare(out, ref, tol=1e-8, min_same=1.0)
    assert (ref["status"] == 1).all()
    return max(r["du"], r["dgrf"])


@pytest.mark.parametrize("h,n,rows", [(10, 6, "twin"), (16, 2, "quad"), (20, 2, "quad")])
def test_emulated_fused_path(oracle, scen, h, n, rows):
    """one row per QP against the oracle, and the rows the device runs (main / twin pairs at h = 10, quads at h = 16 / 20) with the single row's bits"""
    sc = generic_scenario(scen, h, 8)
    one = emu.solve(sc, n)
    worst = _held(one, oracle_batch(oracle, sc, n))
    dev = emu.solve(sc, n, **{rows: True})
    for k in KEYS + ("nfact",):
        assert np.array_equal(one[k], dev[k]), (h, rows, k)
    print(f"emulated fused path h{h} x {n}: worst force difference {worst:.1e} N")


@pytest.mark.parametrize("h,n,rows", [(10, 5, 2), (4, 3, 2)])
def test_emulated_split_pipeline(oracle, scen, h, n, rows):
    sc = generic_scenario(scen, h, 8)
    worst = _held(emu.solve(sc, n, split_rows=rows), oracle_batch(oracle, sc, n))
    two = emu.solve(sc, n, split_rows=rows, twin=True)
    assert np.array_equal(two["u"], emu.solve(sc, n)["u"])
    print(f"emulated split pipeline h{h} x {n}: worst force difference {worst:.1e} N")


def test_emulated_general_path(oracle, scen):
    """per-step feet and a contact schedule at h = 10: single row and main / twin pair against the oracle's strided formation"""
    h, nb = 10, 3
    sc, foot, fs, contact, cs = generic_strided(scen, h, nb)
    out = emu.solve_gen(sc, foot, fs, contact, cs)
    ref = oracle_strided(oracle, oracle_params(oracle, sc), oracle.default_settings(), sc, foot, fs, contact, cs, np.arange(nb))
    pr = oracle_params(oracle, sc)
    nfact = [oracle.mpc_solve(pr, oracle.default_settings(), sc["x0"][b], sc["xref"][b], sc["R"][b], foot[b], contact[b], foot_stride=fs, contact_stride=cs)["info"].nfact
             for b in range(nb)]
    assert np.array_equal(out["nfact"], nfact)
    compare(out, ref, tol=1e-8, min_same=1.0)
    two = emu.solve_gen(sc, foot, fs, contact, cs, twin=True)
    assert all(np.array_equal(two[k], out[k]) for k in KEYS)


def test_emulated_update_path(oracle, scen):
    """warm_start = 2 over four ticks at h = 10 on the fused main / twin pair: the oracle's iteration, status and forces every tick"""
    h = 10
    seq = scen.config2_trot_sequence(8, horizon=h)
    seq["params"] = generic_params(seq["params"])
    pr = oracle_params(oracle, seq); st = oracle.default_settings(warm_start=1)
    carry_o = oracle.update_carry(h)
    wx = np.zeros((1, 12 * h)); wy = np.zeros((1, 20 * h)); rho = np.zeros(1); carry = emu.carry_buffer(h, 1)
    for k in range(4):
        o = oracle.mpc_solve_update(pr, st, seq["x0"][k], seq["xref"][k], seq["R"][k], seq["foot"][k], seq["contact"][k], carry_o)
        one = {kk: (seq[kk][k:k + 1] if kk in ("x0", "xref", "R", "foot", "contact") else seq[kk]) for kk in seq}
        e = emu.solve(one, n=1, warm=(wx, wy, rho), carry=carry, warm_start=2, twin=True)
        assert e["iters"][0] == o["info"].iters and e["status"][0] == o["info"].status == 1 and e["nfact"][0] == o["info"].nfact, (k, e["iters"], o["info"].iters)
        assert np.abs(e["grf"][0] - o["grf"]).max() < 1e-8 and np.abs(e["u"][0] - o["u"]).max() < 1e-8, k
    assert carry[0, 0] > 0.0


@pytest.mark.parametrize("split", [0, 2])
def test_emulated_ruiz_sweep_early_stop_is_exact_without_the_references_weights(scen, split):
    """RowSolver::setup argues the ties of its early stop from the reference's weights; the claim is exactness, and it must hold without them: a build that visits every
    column (-DA1X_FULL_SWEEP) gives the same bits at h = 10, fused and through the set-up kernel of the split pipeline"""
    sc = generic_scenario(scen, 10, 8)
    fast = emu.solve(sc, 6, split_rows=split, twin=split > 0)
    with emu.using(emu.variant(["-DA1X_FULL_SWEEP"], "fullsweep")):
        full = emu.solve(sc, 6, split_rows=split, twin=split > 0)
    for k in KEYS + ("nfact",):
        assert np.array_equal(fast[k], full[k]), k


# ------------------------------------------------------------------------------------------------ 5. the caller-side kernel texts
N = 67    # a partly filled second wavefront
_BODY = {"mass": dict(mass=12.0), **{k: v for k, v in generic_variants().items() if "inertia" in v}}   # what the plants read: the mass and all nine inertia words


def _step_same(out, ref, n, touch=False):
    """test_plant_host._same / test_walk_host._same_step / test_ground_host._same_step: omega, v, pos, R, the feet (foot_vel_body, touch) bit for bit, the angles within
    plant_ref.ANGLE_BAR; rows beyond n and words [12:stride) stay poisoned"""
    f64 = out[:4]     # state, R, foot (, foot_vel_body)
    assert all(np.isnan(a[n:]).all() for a in f64) and np.isnan(f64[0][:n, 12:]).all()
    assert not np.isnan(f64[0][:n, :12]).any() and not any(np.isnan(a[:n]).any() for a in f64[1:])
    assert PR.bits_equal(f64[0][:n, 3:12], ref[0][:, 3:12])
    for a, r in zip(f64[1:], ref[1:]):
        assert PR.bits_equal(a[:n], r)
    if touch:
        assert (out[4][n:] == 0xFF).all() and np.array_equal(out[4][:n], ref[4])
    worst = float(np.abs(f64[0][:n, :3] - ref[0][:, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


def _walkers(scen, seed):
    rng = np.random.default_rng(seed)
    sc = WR.random_walkers(scen, rng, N)
    sc["params"] = generic_params(sc["params"])
    sc["state"][:, 5] = rng.uniform(0.25, 0.45, N)
    sc["wide"] = np.concatenate([sc["state"], rng.normal(0, 1, (N, 10))], 1)
    sc["ground"] = GR.random_planes(sc, rng, N)
    return sc


@pytest.mark.parametrize("substeps", [1, 4])
def test_plant_step_kernel_text(scen, substeps):
    sc = _walkers(scen, 9501)
    a = (sc["wide"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"], 0.0025, substeps)
    ref = PR.step(sc["params"], *a)
    assert_sensitive(f"plant step, {substeps} sub-step(s)", (ref[0][:, 3:12], ref[1], ref[2]),
                     {k: (lambda r: (r[0][:, 3:12], r[1], r[2]))(PR.step(dict(sc["params"], **v), *a)) for k, v in _BODY.items()})
    _step_same(plant_host.run(sc["params"], *a, rows=N + 5), ref, N)


@pytest.mark.parametrize("substeps", [1, 4])
def test_walk_step_kernel_text(scen, substeps):
    sc = _walkers(scen, 9502)
    a = (sc["wide"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], sc["ext"])
    for track, flat in ((0.5, 0), (1.0, 1)):
        kw = dict(dt=0.0025, substeps=substeps, swing_track=track, flat_ground=flat, ground_z=0.05)
        ref = WR.step(sc["params"], *a, **kw)
        assert_sensitive(f"walk step, {substeps} sub-step(s)", (ref[0][:, 3:12],) + tuple(ref[1:4]),
                         {k: (lambda r: (r[0][:, 3:12],) + tuple(r[1:4]))(WR.step(dict(sc["params"], **v), *a, **kw)) for k, v in _BODY.items()})
        _step_same(walk_step_host.run(sc["params"], *a, rows=N + 5, **kw), ref, N)


@pytest.mark.parametrize("substeps", [1, 4])
def test_ground_step_kernel_text(scen, substeps):
    sc = _walkers(scen, 9503)
    a = (sc["wide"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], sc["ground"], sc["ext"])
    kw = dict(dt=0.0025, substeps=substeps, swing_track=0.5)
    ref = GR.step(sc["params"], *a, **kw)
    assert_sensitive(f"ground step, {substeps} sub-step(s)", (ref[0][:, 3:12],) + tuple(ref[1:4]),
                     {k: (lambda r: (r[0][:, 3:12],) + tuple(r[1:4]))(GR.step(dict(sc["params"], **v), *a, **kw)) for k, v in _BODY.items()})
    _step_same(walk_step_ground_host.run(sc["params"], *a, rows=N + 5, **kw), ref, N, touch=True)


@pytest.mark.parametrize("with_ext", [False, True])
def test_sensor_synthesis_kernel_text(scen, with_ext):
    """the synthesis reads the mass (accelerometer, foot force): the outputs that are + - * / alone bit for bit, the others within 4 E of the 80-bit evaluation"""
    rng = np.random.default_rng(9504)
    sc = SR.random_robots(scen, rng, N, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
    mass = GENERIC_CONSTANTS["mass"]
    a = (sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"] if with_ext else None)
    r64, r80 = (SR.synthesise(mass, *a, rho_opt=sc["rho_opt"], dtype=dt) for dt in (np.float64, np.longdouble))
    other = SR.synthesise(sc["mass"], *a, rho_opt=sc["rho_opt"])
    assert_sensitive("sensor synthesis", (r64["imu_acc_raw"],), dict(mass=(other["imu_acc_raw"],)))
    out = sensor_synthesis_host.run(mass, *a, rho_opt=sc["rho_opt"], rows=N + 3)
    SR.assert_is_ref(out, r64, r80, N, ("generic", with_ext))
    assert all((v[N:] == 0xFF).all() if k == "reach" else np.isnan(v[N:]).all() for k, v in out.items())


@pytest.mark.parametrize("h", [4, 10, 20])
def test_horizon_states_kernel_text(scen, h):
    """per-step feet, a yaw of its own: states within HS.BAR of the longdouble recurrence, the costs within HS.BAR of the abs-sum of their terms; every variant (and the
    mass) moves the recurrence's states or costs"""
    sc, feet, fs, _, _ = generic_strided(scen, h, N)
    rng = np.random.default_rng(9505 + h)
    u = rng.uniform(-60.0, 180.0, (N, 12 * h)); yaw = sc["x0"][:, 2] + rng.uniform(-0.5, 0.5, N)
    X, S = HS.rollout(sc["params"], h, sc["x0"], sc["R"], feet, fs, u, yaw)
    cy = HS.costs(sc["params"], h, X, sc["xref"], u)

    def yard(var):
        p = dict(sc["params"], **var); Xv, _ = HS.rollout(p, h, sc["x0"], sc["R"], feet, fs, u, yaw)
        return (Xv.astype(np.float64), HS.costs(p, h, Xv, sc["xref"], u).astype(np.float64))
    assert_sensitive(f"horizon states h{h}", (X.astype(np.float64), cy.astype(np.float64)), {k: yard(v) for k, v in dict(generic_variants(), mass=dict(mass=12.0)).items()})
    xp, cost = horizon_states_host.run(sc["params"], h, sc["R"], feet, x0=sc["x0"], xref=sc["xref"], u=u, foot_stride=fs, yaw_A=yaw, rows=N + 20)
    assert np.isnan(xp[N:]).all() and np.isnan(cost[N:]).all() and not np.isnan(xp[:N]).any() and not np.isnan(cost[:N]).any()
    ratio = HS.states_ratio(xp[:N], X, S)
    q = np.asarray(sc["params"]["q"], np.float64)[:12]
    scale0 = (q * (S[..., :12] + np.abs(sc["xref"].reshape(N, h, 13)[..., :12])) ** 2).sum((1, 2))
    r0 = float((np.abs(cost[:N, 0] - cy[:, 0]) / scale0).max()); r1 = float((np.abs(cost[:N, 1] - cy[:, 1]) / cy[:, 1]).max())
    print(f"h {h}: worst |x_pred - X| / S = {ratio:.2e}; cost[0] {r0:.2e} of its abs-sum, cost[1] {r1:.2e} relative")
    assert ratio <= HS.BAR and r0 <= HS.BAR and r1 <= HS.BAR
