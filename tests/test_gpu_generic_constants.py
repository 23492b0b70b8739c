"""GPU, through the C ABI: every kernel that reads the robot constants on a GENERIC set (gpu_common.GENERIC_CONSTANTS) -- a full inertia_body, weight on x / y position,
twelve different r.  Every scenarios.PARAM_SETS entry has a diagonal inertia, q[3] = q[4] = 0 and r repeated over lanes, so on the rest of the suite a kernel may read a
wrong pair of inertia words, swap or drop q[3] / q[4], index r by leg, or be handed the diagonal only by a configuration copy, and pass.

Yardsticks and bars are the ones the suite already holds: the oracle through gpu_common.held_to_oracle (TOL_FORCE_N; the cap on QPs settled by the 80-bit build is shown to
hold for the oracle alone on these very batches by tests/test_generic_constants_host.py), the reference's ConvexMpc at 1e-12 / 1e-10, HS.BAR, and bit for bit where the
existing test of an entry is.  Every solver test first shows, on the yardstick and for its own batch, that each of the seven generic_variants() moves the forces by more than
100 x TOL_FORCE_N on at least half of the QPs looked at: a pass cannot come from inputs that hide the constants.  The balance QP has weights of its own: tests/test_gpu_balance_constants.py
holds it to a generic set of those."""
import ctypes as C

import numpy as np
import pytest

import ground_ref as GR
import horizon_states_ref as HS
import plant_ref as PR
import sensor_synthesis_ref as SR
import walk_ref as WR
from gpu_common import (GENERIC_CONSTANTS, GENERIC_FAST_CASES, TickChain, _engine, assert_batch_is_sensitive, assert_sensitive, assert_worlds_equal, generic_case_id,
                        generic_params, generic_scenario, generic_strided, generic_variants, generic_warm_ticks, held_to_oracle, oracle_sample, oracle_strided,
                        oracle_warm_chain, split_case, tick_buffers, tick_inputs, tick_world)
from helpers import TOL_FORCE_N, oracle_params, take
from test_gpu_settings_kernel_families import FAST_SHAPES, GEN_SHAPES_H10, _x87_cold

pytestmark = pytest.mark.gpu
KEYS = ("u", "grf", "iters", "status")
N_SENS = 48     # QPs of a batch the variant check looks at (spread over it, the first and the last among them)


def _oracle(oracle, sc, idx, osqp=None, foot=None, fs=0, contact=None, cs=0):
    st = oracle.default_settings(**(osqp or {}))
    return oracle_strided(oracle, oracle_params(oracle, sc), st, sc, sc["foot"] if foot is None else foot, fs, sc["contact"] if contact is None else contact, cs, idx)


def _sensitive(label, oracle, sc, n, osqp=None, **strided):
    idx = oracle_sample(n, N_SENS)
    st = oracle.default_settings(**(osqp or {}))
    ref = _oracle(oracle, sc, idx, osqp, **strided)
    assert_batch_is_sensitive(label, oracle, sc, idx, ref["u"], st, **strided)


# ------------------------------------------------------------------------------------------------ formation
@pytest.mark.parametrize("h", [10, 16, 20])
def test_formation(pkg, oracle, scen, h):
    """a1mpc_form_qp_batch, 6 QPs: broadcast feet, per-step feet, per-step feet with a contact schedule, and a yaw_A different from x0[2] -- P within 1e-12 and g within
    1e-10 (relative to the largest entry) of S/ConvexMpc.cpp compiled verbatim and of the oracle, l and u equal: the bars of
    test_gpu_formed_dense_qp_equals_reference_ConvexMpc.  (The reference has no contact schedule: that form is held to the oracle, which
    tests/test_generic_constants_host.py holds to the reference.)"""
    import ref as REF
    if not REF.build():
        pytest.skip("oracle/_ref not available")
    nb = 6
    sc, foot, fs, contact, cs = generic_strided(scen, h, nb)
    p = sc["params"]; pr = oracle_params(oracle, sc)
    yaw = sc["x0"][:, 2] + np.random.default_rng(h).uniform(0.1, 0.6, nb) * np.array([1, -1, 1, -1, 1, -1])
    P0 = np.array([oracle.mpc_form(pr, sc["x0"][b], sc["xref"][b], sc["R"][b], sc["foot"][b], sc["contact"][b])[0] for b in range(nb)])
    assert_sensitive(f"formation h{h}", (P0,), {k: (np.array([oracle.mpc_form(oracle_params(oracle, dict(sc, params=dict(p, **v))), sc["x0"][b], sc["xref"][b], sc["R"][b],
                                                                              sc["foot"][b], sc["contact"][b])[0] for b in range(nb)]),)
                                                for k, v in generic_variants().items()})
    with _engine(pkg, sc, nb, warm_start=0) as eng:
        bc = eng.form_qp(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
        ps = eng.form_qp(sc["x0"], sc["xref"], sc["R"], foot, sc["contact"], foot_stride=12)
        pc = eng.form_qp(sc["x0"], sc["xref"], sc["R"], foot, contact, foot_stride=12, contact_stride=4)
        ya = eng.form_qp(sc["x0"], sc["xref"], sc["R"], foot, sc["contact"], foot_stride=12, yaw_A=yaw)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    worst = [0.0, 0.0]

    def held(out, b, P, g, l, u, what):
        rp, rg = rel(out["P"][b], P), rel(out["g"][b], g)
        worst[0], worst[1] = max(worst[0], rp), max(worst[1], rg)
        assert rp <= 1e-12 and rg <= 1e-10, (h, b, what, rp, rg)
        assert np.array_equal(out["l"][b], l) and np.array_equal(out["u"][b], u), (h, b, what)
    for b in range(nb):
        a = (sc["x0"][b], sc["xref"][b], sc["R"][b])
        for out, f, fstr, eul, what in ((bc, sc["foot"][b], 0, sc["x0"][b][:3], "broadcast"), (ps, foot[b], 12, sc["x0"][b][:3], "per-step feet"),
                                        (ya, foot[b], 12, np.array([sc["x0"][b][0], sc["x0"][b][1], yaw[b]]), "yaw_A")):
            r = REF.convex_mpc_form(h, p["q"], p["r"], eul, p["mass"], p["inertia"], sc["R"][b], f, sc["contact"][b], sc["x0"][b], sc["xref"][b], p["dt"], foot_stride=fstr)
            held(out, b, r["P"], r["g"], r["l"], r["u"], what + " vs the reference")
            P, g, A, l, u, _ = oracle.mpc_form(pr, *a, f, sc["contact"][b], yaw=None if what != "yaw_A" else yaw[b], foot_stride=fstr)
            held(out, b, P, g, l, u, what + " vs the oracle")
        P, g, A, l, u, _ = oracle.mpc_form(pr, *a, foot[b], contact[b], foot_stride=12, contact_stride=4)
        held(pc, b, P, g, l, u, "contact schedule vs the oracle")
        assert rel(ya["P"][b], ps["P"][b]) > 1e-6     # (the yaw of its own does change the QP)
    print(f"formation h{h}: worst P {worst[0]:.1e}, g {worst[1]:.1e} relative")


# ------------------------------------------------------------------------------------------------ the fast path, cold
@pytest.mark.parametrize("h,n_fused,n_split", FAST_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", GENERIC_FAST_CASES, ids=generic_case_id)
def test_fast_path_cold(pkg, oracle, scen, case, h, n_fused, n_split):
    """one generic batch per (case, horizon): all of it through the split pipeline, its first n_fused QPs through the fused kernel, its first 200 through the latency kernel;
    which kernel ran is asserted (only the split pipeline has a set-up stage of its own); the latency kernel's rows equal the split batch's bit for bit; the split and the
    fused batch are held to the oracle on 256 QPs spread over each, the first and the last included"""
    osqp, par = split_case(case)
    sc = generic_scenario(scen, h, n_split, **par)
    _sensitive(f"fast path h{h} x {n_split} {generic_case_id(case)}", oracle, sc, n_split, osqp)
    sizes = [n for n in (n_split, n_fused) if n is not None]
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
        idx = oracle_sample(n, 256)
        assert idx[0] == 0 and idx[-1] == n - 1
        ref = _oracle(oracle, sc, idx, osqp)
        assert (ref["status"] == 1).all()
        held_to_oracle({k: outs[n][k][idx] for k in KEYS}, ref, lambda j: x87_solve(int(idx[j])), case, label=f"generic h{h} x {n} ({'split' if n == n_split else 'fused'})")


# ------------------------------------------------------------------------------------------------ the general path
@pytest.mark.parametrize("h,n,kernel", GEN_SHAPES_H10 + [(20, 1700, "split")], ids=lambda v: str(v))
def test_general_path(pkg, oracle, scen, h, n, kernel):
    """per-step feet and a contact schedule, default settings: the general path's latency kernel, fused kernel and split pipeline at h = 10 and its split pipeline at
    h = 20, vs the oracle's strided formation on 96 QPs that hold the first and the last"""
    sc, foot, fs, contact, cs = generic_strided(scen, h, n)
    strided = dict(foot=foot, fs=fs, contact=contact, cs=cs)
    _sensitive(f"general path h{h} x {n}", oracle, sc, n, **strided)
    idx = oracle_sample(n, 96)
    assert len(idx) >= min(n, 96) and idx[0] == 0 and idx[-1] == n - 1
    ref = _oracle(oracle, sc, idx, **strided)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        out = eng.solve_strided(sc["x0"], sc["xref"], sc["R"], foot, fs, contact, cs, want_u=True)
        form_ms = eng.last_stage_ms()[0]
    assert (form_ms > 0.0) if kernel == "split" else (form_ms == 0.0), (h, n, kernel, form_ms)
    x87_sub = _x87_cold(sc, h, {}, foot, fs, contact, cs)
    held_to_oracle({k: out[k][idx] for k in KEYS}, ref, lambda j: x87_sub(int(idx[j])), {}, label=f"generic general path h{h} x {n} ({kernel})")


# ------------------------------------------------------------------------------------------------ warm starts
@pytest.mark.parametrize("mode", [1, 2])
def test_warm_starts(pkg, oracle, scen, mode):
    """the pattern of test_warm_start_modes_with_non_default_settings at h = 10 x 64: four ticks of slowly moving states, every leg changing role at tick 2, every robot
    chained through the oracle with its own carry -- warm_start = 1 (x, y, rho carried) and 2 (the update path)"""
    import x87
    h, n = 10, 64
    ticks = generic_warm_ticks(scen, h, n)
    _sensitive(f"warm_start = {mode}, h{h} x {n}, tick 0", oracle, ticks[0], n)
    chain = oracle_warm_chain(oracle, x87, ticks, mode, h)
    with _engine(pkg, ticks[0], n, warm_start=mode) as eng:
        for t, (sc, (ref, x87_solve)) in enumerate(zip(ticks, chain)):
            out = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
            held_to_oracle({k: out[k] for k in KEYS}, ref, x87_solve, {}, label=f"generic warm_start = {mode}, h{h} x {n}, tick {t}")
        assert eng.last_warm_start_mode() == mode


# ------------------------------------------------------------------------------------------------ configuration transport
def test_configuration_transport(pkg, oracle, scen):
    """the same 300 QPs through a single handle, a sharded handle with two shards on device 0 and a pipeline handle, each built from the generic configuration: forces,
    iterations and statuses bit-equal -- a copy of the configuration that carried only part of it would part them -- and the single handle held to the oracle"""
    h, n = 10, 300
    sc = generic_scenario(scen, h, n, seed=9410)
    _sensitive(f"configuration transport h{h} x {n}", oracle, sc, n)
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    args = (sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
    with pkg.Engine(cfg, n, 0) as eng:
        one = eng.solve(*args, want_u=True)
    with pkg.ShardedEngine(cfg, n, devices=[0, 0], transport=0) as sh:
        assert sh.info()["n_shards"] == 2
        two = sh.solve(*args)
    piped = dict(grf=np.full((n, 12), np.nan), u=np.full((n, 12 * h), np.nan), iters=np.full(n, -1, np.int32), status=np.full(n, -99, np.int32))
    with pkg.Pipeline(cfg, n, 0, depth=2) as pipe:
        pipe.submit(*args, piped)
        pipe.wait()
    for k in ("grf", "iters", "status"):
        assert np.array_equal(one[k], two[k]), ("sharded", k)
        assert np.array_equal(one[k], piped[k]), ("pipeline", k)
    assert np.array_equal(one["u"], piped["u"])
    idx = oracle_sample(n, 96)
    x87_solve = _x87_cold(sc, h, {})
    held_to_oracle({k: one[k][idx] for k in KEYS}, _oracle(oracle, sc, idx), lambda j: x87_solve(int(idx[j])), {}, label=f"generic single handle h{h} x {n}")


# ------------------------------------------------------------------------------------------------ the control tick
def test_control_tick_matches_the_chain(pkg, oracle, scen):
    """a1mpc_control_tick_device against the seven *_device entries chained by hand (gpu_common.TickChain) on a second handle, n = 300, h = 10, two ticks, both handles built
    from the generic configuration: every output and carried state bit for bit, every status 1.  Both sides are the engine's, so the first tick's MPC stage is also held to
    the ORACLE on the inputs the chain fed it (48 robots: same iteration, status 1, GRFs within TOL_FORCE_N), after the variant check on those inputs."""
    import torch
    n, h = 300, 10
    rng = np.random.default_rng(2025 + n)
    P = generic_params(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS)
    cfg = pkg.make_config(P, h, warm_start=1)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E = pkg.engine
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e7:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        st = torch.cuda.Stream(device=dev)
        chain = TickChain(e7, prm, n, st)
        w1, w7 = tick_world(n, dev, [0.0, 120.0, 120.0, 0.0]), tick_world(n, dev, [0.0, 120.0, 120.0, 0.0])
        for t in range(2):
            inp_np = tick_inputs(scen, rng, n)
            inp = {k: T(v) for k, v in inp_np.items()}
            e1.control_tick_device(prm, tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
            chain.tick(inp, w7)
            st.synchronize()
            assert_worlds_equal(t, w1, w7)
            assert (w1["i32"]["status"].cpu().numpy() == 1).all(), t
            if t == 0:
                s7 = {k: v.cpu().numpy() for k, v in w7["state"].items()}
                tick = scen.pack_tick(inp_np["root_euler"], s7["root_pos"], inp_np["root_ang_vel"], s7["root_lin_vel"], s7["root_euler_d"], inp_np["root_lin_vel_d"],
                                      inp_np["root_ang_vel_d"], inp_np["root_pos_d_z"])
                fed = dict(horizon=h, params=P, x0=np.c_[tick[:, :12], np.full(n, -9.8)], R=inp_np["R_world"], foot=w7["outs"]["foot_pos_abs"].cpu().numpy(),
                           contact=w7["u8"]["contacts"].cpu().numpy(),
                           xref=np.array([oracle.mpc_reference(h, P["dt"], k[0:3], k[3:6], inp_np["R_world"][b], k[12:15], k[15:18], k[18:21], k[21]) for b, k in enumerate(tick)]))
                grf, iters = w7["outs"]["grf"].cpu().numpy(), w7["i32"]["iters"].cpu().numpy()
        _sensitive(f"control tick h{h} x {n}, tick 0", oracle, fed, n)
        idx = oracle_sample(n, N_SENS)
        ref = _oracle(oracle, fed, idx)
        d = float(np.abs(grf[idx] - ref["grf"]).max())
        print(f"control tick h{h} x {n}, tick 0: {len(idx)} robots, worst GRF distance from the oracle {d:.2e} N")
        assert np.array_equal(iters[idx], ref["iters"]) and (ref["status"] == 1).all() and d <= TOL_FORCE_N, d


# ------------------------------------------------------------------------------------------------ predictions
N = 67     # a partly filled second wavefront


@pytest.mark.parametrize("h", [4, 10, 20])
def test_predictions(pkg, scen, h):
    """a1mpc_horizon_states_batch, 67 QPs, per-step feet, a yaw of its own: states within HS.BAR of the longdouble recurrence, the costs within HS.BAR of the abs-sum of
    their terms; at h = 10 also against the reference's A_qp x0 + B_qp u.  Every variant (and the mass) moves the recurrence's states or costs."""
    sc, feet, fs, _, _ = generic_strided(scen, h, N)
    rng = np.random.default_rng(9505 + h)
    u = rng.uniform(-60.0, 180.0, (N, 12 * h)); yaw = sc["x0"][:, 2] + rng.uniform(-0.5, 0.5, N)
    X, S = HS.rollout(sc["params"], h, sc["x0"], sc["R"], feet, fs, u, yaw)
    cy = HS.costs(sc["params"], h, X, sc["xref"], u)

    def yard(var):
        p = dict(sc["params"], **var); Xv, _ = HS.rollout(p, h, sc["x0"], sc["R"], feet, fs, u, yaw)
        return (Xv.astype(np.float64), HS.costs(p, h, Xv, sc["xref"], u).astype(np.float64))
    assert_sensitive(f"horizon states h{h}", (X.astype(np.float64), cy.astype(np.float64)), {k: yard(v) for k, v in dict(generic_variants(), mass=dict(mass=12.0)).items()})
    with _engine(pkg, sc, N, warm_start=0) as eng:
        out = eng.horizon_states(sc["x0"], sc["R"], feet, u=u, xref=sc["xref"], foot_stride=fs, yaw_A=yaw)
    xp, cost = out["x_pred"], out["cost"]
    ratio = HS.states_ratio(xp, X, S)
    q = np.asarray(sc["params"]["q"], np.float64)[:12]
    scale0 = (q * (S[..., :12] + np.abs(sc["xref"].reshape(N, h, 13)[..., :12])) ** 2).sum((1, 2))
    r0 = float((np.abs(cost[:, 0] - cy[:, 0]) / scale0).max()); r1 = float((np.abs(cost[:, 1] - cy[:, 1]) / cy[:, 1]).max())
    print(f"h {h}: worst |x_pred - X| / S = {ratio:.2e}; cost[0] {r0:.2e} of its abs-sum, cost[1] {r1:.2e} relative")
    assert ratio <= HS.BAR and r0 <= HS.BAR and r1 <= HS.BAR, (h, ratio, r0, r1)
    assert np.array_equal(xp[..., 12], np.broadcast_to(sc["x0"][:, 12:13], (N, h)))
    import ref as REF
    if h == 10 and REF.build():     # (oracle/_ref absent: the longdouble recurrence above, which tests/test_horizon_states_abi.py pins to the reference, stands alone)
        r = HS.reference_states(REF, sc["params"], h, sc["x0"], sc["xref"], sc["R"], feet, fs, sc["contact"], u, yaw)
        ratio = HS.states_ratio(xp, r["X"], r["S"])
        print(f"h {h}: worst |x_pred - (A_qp x0 + B_qp u)| / S = {ratio:.2e}")
        assert ratio <= HS.BAR, ratio


# ------------------------------------------------------------------------------------------------ plants and sensors
_BODY = {"mass": dict(mass=12.0), **{k: v for k, v in generic_variants().items() if "inertia" in v}}    # what the plants read: the mass and all nine inertia words


@pytest.fixture(scope="module")
def eng(pkg, scen):
    sc = scen.scenario_stand()
    sc["params"] = generic_params(sc["params"])
    e = _engine(pkg, sc, 512, warm_start=0)
    yield e
    e.close()


def _walkers(scen, seed):
    rng = np.random.default_rng(seed)
    sc = WR.random_walkers(scen, rng, N)
    sc["params"] = generic_params(sc["params"])
    sc["state"][:, 5] = rng.uniform(0.25, 0.45, N)
    sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (N, 10))], 1))
    sc["ground"] = GR.random_planes(sc, rng, N)
    return sc


def _poisoned_tails(out, n):
    return all(np.isnan(a[n:]).all() for a in out[:4]) and np.isnan(out[0][:n, 12:]).all() and not np.isnan(out[0][:n, :12]).any() and \
        not any(np.isnan(a[:n]).any() for a in out[1:4])


@pytest.mark.parametrize("sub", [1, 4])
def test_plant_step(eng, scen, sub):
    """a1mpc_plant_step_batch_device on 67 robots, 1 and 4 sub-steps, a wrench: test_gpu_plant's comparison (pos, R, v, omega and the feet bit for bit, the angles within
    1e-12) with the restatement at the generic mass and inertia; nothing written beyond row n"""
    from test_gpu_plant import _assert_is_ref, _device_step
    sc = _walkers(scen, 9501)
    a = (sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"], 0.0025, sub)
    ref = PR.step(sc["params"], *a)
    assert_sensitive(f"plant step, {sub} sub-step(s)", (ref[0][:, 3:12], ref[1], ref[2]),
                     {k: (lambda r: (r[0][:, 3:12], r[1], r[2]))(PR.step(dict(sc["params"], **v), *a)) for k, v in _BODY.items()})
    out = _device_step(eng, sc, N, sub, True)
    assert _poisoned_tails(out, N)
    _assert_is_ref(out, ref, N, 22)


@pytest.mark.parametrize("sub", [1, 4])
def test_walk_step(eng, scen, sub):
    """a1mpc_walk_step_batch_device: test_gpu_walk's comparison (foot_vel_body among the bits) at swing_track 0.5 without a ground and 1 with the flat ground"""
    from test_gpu_walk import GROUND_Z, _assert_is_ref, _device_step
    sc = _walkers(scen, 9502)
    a = (sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], sc["ext"] if sub == 4 else None)
    for track, flat in ((0.5, 0), (1.0, 1)):
        kw = dict(dt=0.0025, substeps=sub, swing_track=track, flat_ground=flat, ground_z=GROUND_Z)
        ref = WR.step(sc["params"], *a, **kw)
        assert_sensitive(f"walk step, {sub} sub-step(s)", (ref[0][:, 3:12],) + tuple(ref[1:4]),
                         {k: (lambda r: (r[0][:, 3:12],) + tuple(r[1:4]))(WR.step(dict(sc["params"], **v), *a, **kw)) for k, v in _BODY.items()})
        out = _device_step(eng, sc, N, track, flat, sub)
        assert _poisoned_tails(out, N)
        _assert_is_ref(out, ref, N)


@pytest.mark.parametrize("sub", [1, 4])
def test_walk_step_ground(eng, scen, sub):
    """a1mpc_ground_step_batch_device with a plane per robot: test_gpu_ground's comparison (touch among the bits)"""
    import torch
    from test_gpu_ground import _assert_is_ref, _ff, _nan, _t
    sc = _walkers(scen, 9503)
    a = (sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], sc["ground"], sc["ext"])
    kw = dict(dt=0.0025, substeps=sub, swing_track=0.5)
    ref = GR.step(sc["params"], *a, **kw)
    assert_sensitive(f"ground step, {sub} sub-step(s)", (ref[0][:, 3:12],) + tuple(ref[1:4]),
                     {k: (lambda r: (r[0][:, 3:12],) + tuple(r[1:4]))(GR.step(dict(sc["params"], **v), *a, **kw)) for k, v in _BODY.items()})
    so, Ro, fo, vo, to = _nan(N + 3, 22), _nan(N + 3, 9), _nan(N + 3, 12), _nan(N + 3, 12), _ff(N + 3)
    torch.cuda.synchronize()
    eng.walk_step_ground_device(N, _t(sc["tick"]), 22, _t(sc["R"]), _t(sc["foot"]), _t(sc["grf"]), _t(sc["contacts"]), _t(sc["Rz"]), _t(sc["target"]), vo, to, _t(sc["ground"]),
                                _t(sc["ext"]), so, Ro, fo, walk=eng.walk_config(substeps=sub, swing_track=0.5))
    torch.cuda.synchronize()
    out = tuple(x.cpu().numpy() for x in (so, Ro, fo, vo, to))
    assert _poisoned_tails(out, N) and (out[4][N:] == 0xFF).all()
    _assert_is_ref(out, ref, N)


@pytest.mark.parametrize("ext", [False, True])
def test_sensor_synthesis(eng, scen, ext):
    """a1mpc_sensor_synthesis_batch_device reads the mass (accelerometer, foot force): test_gpu_sensor_synthesis's comparison -- the outputs that are + - * / alone bit for
    bit, the others within 4 E of the restatement's 80-bit evaluation"""
    from test_gpu_sensor_synthesis import _device_call, _tail_untouched
    rng = np.random.default_rng(9504)
    sc = SR.random_robots(scen, rng, N, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
    sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (N, 10))], 1))
    mass = GENERIC_CONSTANTS["mass"]
    a = (sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"] if ext else None)
    r64, r80 = (SR.synthesise(mass, *a, rho_opt=sc["rho_opt"], dtype=dt) for dt in (np.float64, np.longdouble))
    other = SR.synthesise(sc["mass"], *a, rho_opt=sc["rho_opt"])
    assert_sensitive("sensor synthesis", (r64["imu_acc_raw"],), dict(mass=(other["imu_acc_raw"],)))
    out = _device_call(eng, sc, N, ext)
    assert _tail_untouched(out, N) and not any(np.isnan(v[:N]).any() for k, v in out.items() if k != "reach")
    SR.assert_is_ref(out, r64, r80, N, ("generic", ext))
