"""GPU, through the C ABI: the caller-side kernels and the one-call control ticks at NON-DEFAULT parameters.  Every caller-side stage takes its constants as arguments
(a1mpc_gait_config, a1mpc_contact_config, a1mpc_tick_params); the rest of the suite runs them at the reference's defaults, where gait.counter_per_swing equals
contact.counter_per_swing, gait.control_dt equals control_dt, and a kernel with 240, 180.0, 0.0025 or 30.0 written into it is indistinguishable from a correct one.  Here
they run at gpu_common.PARAM_SETS: set A (every duplicated quantity different in its two places, nothing at its default) and set B (another period, proportional).
Per-stage tests hold each entry to the oracle (pinned to the reference's compiled sources at these parameters by tests/test_ref_pin.py) at the bars of the existing
per-stage tests, scaled only where a parameter scales the output; the one-call ticks are held to the *_device entries chained by hand, every field, on every tick of a gait
cycle.  Before any kernel output is read, each test shows on the yardstick alone that every parameter it varies changes the compared result (gpu_common.assert_sensitive)
and that the counters land exactly on the set's lift-off mark, early-contact mark and wrap.  Small fleets: 67 robots on a handle of 200."""
import ctypes as C

import numpy as np
import pytest

import gpu_common as G
from gpu_common import PARAM_SETS, PARAM_SPEEDS, TickChain, assert_sensitive, assert_thresholds_are_hit, assert_worlds_equal, tick_buffers, tick_inputs_timetable, tick_world

pytestmark = pytest.mark.gpu

N, CAP = 67, 200     # a partial second wavefront in the robot-per-lane kernels, four lanes per robot in the plan / preview kernels, spare capacity behind the batch
SETS = ["A", "B"]


def _cfg(pkg, scen, h=10, dt=None, **osqp):
    P = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
    if dt is not None:
        P = dict(P, dt=dt)
    return pkg.make_config(P, h, **osqp)


def _fleet(ps, n, ticks, stand=True, check=True):
    """the set's staggered fleet, its movement_mode timetable and (check) the input-side assertion that the marks are hit"""
    gk = G.gait_kw(ps)
    gc0, spd = G.gait_cycle_fleet(n, PARAM_SPEEDS, per_gait=gk["per_gait"], reset=gk["reset"])
    mm_table = G.stand_timetable(n, ticks) if stand else np.ones((ticks, n), np.uint8)
    if check:
        assert_thresholds_are_hit(gc0, spd, mm_table, early_mark=G.early_mark(ps), **gk)
    return gc0, spd, mm_table


# ---------------------------------------------------------------------------------------------------------------- update_plan
def plan_yardstick(oracle, scen, ps, n, ticks, seed):
    """inputs of `ticks` consecutive update_plan calls and the yardstick's outputs: numpy (gpu_common.np_update_plan) held to the oracle bit for bit, and the variants with
    one parameter at its default"""
    rng = np.random.default_rng(seed)
    gc, spd, mm_table = _fleet(ps, n, ticks)
    assert (mm_table == 0).any()
    gp = G.oracle_gait(oracle, ps)
    back = dict(counter_per_gait=dict(counter_per_gait=240.0), counter_per_swing=dict(counter_per_swing=120.0), control_dt=dict(gait_dt=0.0025),
                foot_delta_x_limit=dict(foot_delta_x_limit=0.1), foot_delta_y_limit=dict(foot_delta_y_limit=0.1), default_foot_pos=dict(default_foot_pos=G.DEFAULT_FOOT_POS),
                gait_counter_reset=dict(gait_counter_reset=(0.0, 120.0, 120.0, 0.0)))
    back = {k: v for k, v in back.items() if any(np.any(np.asarray(ps[f]) != np.asarray(x)) for f, x in v.items())}   # (set A's gait.counter_per_swing IS 120)
    steps = []; full = []; var = {k: [] for k in back}; saturated = set()
    dfp = np.asarray(ps["default_foot_pos"]).reshape(4, 3)
    for t in range(ticks):
        inp = G.plan_inputs(scen, rng, n, ps); mm = mm_table[t]
        a = (mm, gc, spd, inp["v"], inp["Rz"], inp["R"], inp["pos"], inp["vd"])
        out = G.np_update_plan(ps, *a)
        for b in range(0, n, 3):   # numpy against the oracle (every third robot: the restatement is vectorised, the oracle is one C call per robot)
            o = oracle.update_plan(gp, mm[b], gc[b], spd[b], inp["v"][b], inp["Rz"][b], inp["R"][b], inp["pos"][b], inp["vd"][b])
            assert all(np.array_equal(x, y[b]) for x, y in zip(o, out)), (t, b)
        for k, over in back.items():
            var[k].append(G.np_update_plan(ps, *a, **over))
        d = out[2].reshape(n, 4, 3)[:, :, :2] - dfp[None, :, :2]
        for ax, lim in ((0, ps["foot_delta_x_limit"]), (1, ps["foot_delta_y_limit"])):
            saturated |= {(ax, s) for s in (1, -1) if np.any(np.abs(d[:, :, ax] - s * lim) <= 1e-16)}
        steps.append((a, out)); full.append(out); gc = out[0]
    assert saturated == {(0, 1), (0, -1), (1, 1), (1, -1)}, saturated
    cat = lambda runs: tuple(np.concatenate([np.asarray(r[j], dtype=np.float64).reshape(n, -1) for r in runs], axis=1) for j in range(5))
    assert_sensitive(f"update_plan, set {ps['name']}", cat(full), {k: cat(v) for k, v in var.items()})
    return steps


@pytest.mark.parametrize("name", SETS)
def test_update_plan_at_other_gaits(pkg, oracle, scen, name):
    """a1mpc_update_plan_batch at the set's a1mpc_gait_config over counter_per_gait / 5 consecutive ticks of the staggered fleet with a stand timetable (the set's
    gait_counter_reset is written), commanded velocities that saturate foot_delta_x_limit and foot_delta_y_limit on both sides (asserted on the yardstick): all five outputs
    bit for bit."""
    ps = PARAM_SETS[name]
    ticks = int(ps["counter_per_gait"] / 5)
    steps = plan_yardstick(oracle, scen, ps, N, ticks, 300 + ord(name))
    gait = G.gait_config(pkg.engine, ps)
    with pkg.Engine(_cfg(pkg, scen), CAP, 0) as eng:
        for t, (a, ref) in enumerate(steps):
            out = eng.update_plan(*a, gait=gait)
            for k, r in zip(("gait_counter", "plan_contacts", "foot_pos_target_rel", "foot_pos_target_abs", "foot_pos_target_world"), ref):
                assert np.array_equal(out[k], r), (t, k, np.argwhere(out[k] != r)[:4])
    print(f"update_plan, set {name}: {ticks} ticks x {N} robots bit for bit (worst distance 0)")


# ---------------------------------------------------------------------------------------------------------------- contacts / terrain
def contact_yardstick(oracle, ps, adapt, n, ticks, seed):
    rng = np.random.default_rng(seed)
    gk = G.gait_kw(ps)
    gc, spd, mm_table = _fleet(ps, n, ticks, stand=False)
    kw = dict(counter_per_swing=ps["contact_per_swing"], foot_force_low=ps["foot_force_low"], use_terrain_adapt=adapt)
    base = np.outer([0.2, 0.2, -0.2, -0.2], [1.0, 0.0, 0.3]).reshape(12) + np.outer([1, -1, 1, -1], [0.0, 0.13, 0.0]).reshape(12) + np.tile([0.0, 0.0, -0.3], 4)
    states = [oracle.contact_state() for _ in range(n)]; alt = [oracle.contact_state() for _ in range(n)]
    pitch0 = np.full(n, 0.0625); pitch = pitch0.copy(); pitch_alt = pitch0.copy()
    early = {k: np.zeros((n, 4), bool) for k in ("full", "counter_per_swing", "foot_force_low")}
    steps = []; cts = {k: [] for k in early}; pit = []; pit_alt = []
    for t in range(ticks):
        gc, plan = G.gait_loop(gc, spd, mm_table[t], **gk)
        ff = rng.choice(G.force_values(ps), size=(n, 4)); foot = base + rng.normal(0, 0.03, (n, 12)); z = np.where(rng.random(n) < 0.9, 0.3, 0.05)
        ref = [oracle.contact_terrain_step(states[b], gc[b], plan[b], ff[b], foot[b], z[b], pitch[b], **kw) for b in range(n)]
        pitch_in = pitch; pitch = np.array([r[3] for r in ref])
        ct = np.array([r[0] for r in ref])
        for k, (cps, low) in dict(full=(ps["contact_per_swing"], ps["foot_force_low"]), counter_per_swing=(120.0, ps["foot_force_low"]),
                                  foot_force_low=(ps["contact_per_swing"], 30.0)).items():
            c, early[k] = G.np_contacts(gc, plan, ff, early[k], cps, low); cts[k].append(c)
        assert np.array_equal(cts["full"][-1], ct), t   # the numpy lines ARE the oracle's contacts
        if adapt == 0:   # the same run with the terrain adaptation on: the pitch must move
            ra = [oracle.contact_terrain_step(alt[b], gc[b], plan[b], ff[b], foot[b], z[b], pitch_alt[b], **dict(kw, use_terrain_adapt=1)) for b in range(n)]
            pitch_alt = np.array([r[3] for r in ra]); pit_alt.append(pitch_alt)
        pit.append(pitch)
        steps.append(((gc, plan, ff, foot, z), pitch_in, dict(contacts=ct, rec=np.array([r[1] for r in ref]), angle=np.array([r[2] for r in ref]), pitch=pitch)))
    st = lambda seq: np.stack(seq, axis=1)
    var = {k: (st(cts[k]),) for k in ("counter_per_swing", "foot_force_low")}
    assert_sensitive(f"contacts, set {ps['name']}", (st(cts["full"]),), var)
    if adapt == 0:
        assert_sensitive(f"terrain pitch, set {ps['name']}", (st(pit),), dict(use_terrain_adapt=(st(pit_alt),)))
        assert np.array_equal(st(pit), np.tile(pitch0[:, None], (1, ticks)))
    return steps


@pytest.mark.parametrize("adapt", [0, 1])
@pytest.mark.parametrize("name", SETS)
def test_contact_terrain_contacts_and_terrain_entries_at_other_configs(pkg, oracle, scen, name, adapt):
    """One cycle of the set's slowest leg (walking fleet, forces ON 45 N and 50 N) through a1mpc_contact_terrain_batch, a1mpc_contacts_batch (a handle of its own) and
    a1mpc_terrain_batch (a third handle, fed the first one's foot_pos_recent_contact) at the set's a1mpc_contact_config, then the threshold scripts at the set's marks
    (150 / 240 and the next double, 45 N and the next double) on a fresh handle: contacts and filtered positions bit for bit against the oracle, terrain angle and pitch
    within 1e-13; with use_terrain_adapt = 0 the pitch comes back bit-unchanged from both entries that take it."""
    ps = PARAM_SETS[name]
    ticks = int(ps["counter_per_gait"] / min(PARAM_SPEEDS))
    steps = contact_yardstick(oracle, ps, adapt, N, ticks, 500 + 2 * ord(name) + adapt)
    ccfg = G.contact_config(pkg.engine, ps, adapt)
    worst = 0.0
    cfg = _cfg(pkg, scen)
    with pkg.Engine(cfg, CAP, 0) as e_ct, pkg.Engine(cfg, CAP, 0) as e_c, pkg.Engine(cfg, CAP, 0) as e_t, pkg.Engine(cfg, CAP, 0) as e_s:
        pitch_t = steps[0][1].copy()
        for t, (a, pitch_in, ref) in enumerate(steps):
            out = e_ct.contact_terrain(*a, pitch_in, cfg=ccfg)       # (fed the yardstick's pitch: 1e-13 differences do not accumulate into the comparison)
            alone = e_c.contacts(*a[:4], cfg=ccfg)
            pitch_t, ang_t = e_t.terrain(out["foot_pos_recent_contact"], a[4], pitch_in, use_terrain_adapt=adapt)
            assert np.array_equal(out["contacts"], ref["contacts"]) and np.array_equal(out["foot_pos_recent_contact"], ref["rec"]), (t, np.argwhere(out["contacts"] != ref["contacts"])[:4])
            assert np.array_equal(alone["contacts"], ref["contacts"]) and np.array_equal(alone["foot_pos_recent_contact"], ref["rec"]), t
            d = max(np.abs(out["terrain_angle"] - ref["angle"]).max(), np.abs(out["root_euler_d_pitch"] - ref["pitch"]).max(),
                    np.abs(ang_t - ref["angle"]).max(), np.abs(pitch_t - ref["pitch"]).max())
            worst = max(worst, d)
            assert d <= 1e-13, (t, d)
            if adapt == 0:
                assert np.array_equal(out["root_euler_d_pitch"], pitch_in) and np.array_equal(pitch_t, pitch_in), t
        scripts = G.contact_scripts(ps["counter_per_swing"], ps["foot_force_low"], ps["contact_per_swing"], ps["counter_per_gait"])
        worst_s = G.contact_threshold_run(lambda *a: e_s.contact_terrain(*a, cfg=ccfg), oracle, N, 1e-13, scripts=scripts, adapt=adapt,
                                          counter_per_swing=ps["contact_per_swing"], foot_force_low=ps["foot_force_low"])
    print(f"contact stage, set {name}, adapt {adapt}: {ticks} ticks, contacts / positions bit for bit, worst angle / pitch distance {worst:.2e} (cycle), {worst_s:.2e} (scripts)")


# ---------------------------------------------------------------------------------------------------------------- swing legs
def swing_inputs(scen, ps, n, ticks, seed, check=True):
    rng = np.random.default_rng(seed)
    gk = G.gait_kw(ps)
    gc, spd, mm_table = _fleet(ps, n, ticks, stand=False, check=check)
    dfp = np.asarray(ps["default_foot_pos"])
    steps = []
    for t in range(ticks):
        gc, _ = G.gait_loop(gc, spd, mm_table[t], **gk)
        yaw = rng.uniform(-3, 3, n); Rz = scen.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)
        steps.append((Rz, dfp + rng.normal(0, 0.03, (n, 12)), gc, dfp + rng.normal(0, 0.05, (n, 12))))
    return steps


def swing_oracle_run(oracle, steps, n, kw, target_last_override=None):
    """-> per tick (cur, kin, start, rel_last, target_last), the state carried by the oracle (target_last re-seeded from target_last_override[t] after each tick)"""
    st = [np.zeros((n, 12)) for _ in range(3)]; out = []
    for t, (Rz, foot, gc, tgt) in enumerate(steps):
        cur = np.zeros((n, 12)); kin = np.zeros((n, 12))
        for b in range(n):
            cur[b], kin[b] = oracle.swing_legs(Rz[b], foot[b], gc[b], tgt[b], st[0][b], st[1][b], st[2][b], **kw)
        out.append((cur, kin, st[0].copy(), st[1].copy(), st[2].copy()))
        if target_last_override is not None:
            st[2][:] = target_last_override[t]
    return out


def swing_kw(ps, **over):
    return dict(dict(kp=ps["kp_foot"], kd=ps["kd_foot"], counter_per_swing=ps["counter_per_swing"], dt=ps["control_dt"]), **over)


@pytest.mark.parametrize("name", SETS)
def test_swing_legs_at_other_gains_period_and_dt(pkg, oracle, scen, name):
    """a1mpc_swing_legs_batch over counter_per_gait / 5 ticks of the set's fleet with the set's kp / kd, the gait's counter_per_swing and the tick's control_dt: the carried
    start / last-position state and foot_pos_cur bit for bit, foot_pos_target_last_time within 1e-15, the foot force within 1e-9 scaled by the gains (gpu_common.force_bar).
    The oracle takes the kernel's foot_pos_target_last_time after every tick, as in test_swing_legs_N4a_sequence."""
    ps = PARAM_SETS[name]
    ticks = int(ps["counter_per_gait"] / 5)
    steps = swing_inputs(scen, ps, N, ticks, 700 + ord(name))
    full_kw = swing_kw(ps)
    back = dict(kp_foot=swing_kw(ps, kp=(300.0, 400.0, 400.0)), kd_foot=swing_kw(ps, kd=(8.0, 8.0, 8.0)), counter_per_swing=swing_kw(ps, counter_per_swing=120.0),
                control_dt=swing_kw(ps, dt=0.0025), the_gaits_control_dt=swing_kw(ps, dt=ps["gait_dt"]), the_contact_stages_counter_per_swing=swing_kw(ps, counter_per_swing=ps["contact_per_swing"]))
    back = {k: v for k, v in back.items() if v != full_kw}
    pack = lambda run: tuple(np.stack([r[j] for r in run], axis=1) for j in range(5))
    assert_sensitive(f"swing legs, set {name}", pack(swing_oracle_run(oracle, steps, N, full_kw)), {k: pack(swing_oracle_run(oracle, steps, N, v)) for k, v in back.items()})
    assert max(g[2].max() for g in steps) > ps["counter_per_swing"] + 0.9 * (ps["counter_per_gait"] - ps["counter_per_swing"])   # the spline time comes close to 1
    kp, kd = np.array(ps["kp_foot"]), np.array(ps["kd_foot"])
    st_g = [np.zeros((N, 12)) for _ in range(3)]; got = []
    with pkg.Engine(_cfg(pkg, scen), CAP, 0) as eng:
        for Rz, foot, gc, tgt in steps:
            cur, kin = eng.swing_legs(Rz, foot, gc, tgt, *st_g, kp=kp, kd=kd, counter_per_swing=ps["counter_per_swing"], dt=ps["control_dt"])
            got.append((cur, kin, st_g[0].copy(), st_g[1].copy(), st_g[2].copy()))
    ref = swing_oracle_run(oracle, steps, N, full_kw, target_last_override=[g[4] for g in got])
    worst = dict(target=0.0, kin=0.0)
    for t, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g[0], r[0]) and np.array_equal(g[2], r[2]) and np.array_equal(g[3], r[3]), t
        worst["target"] = max(worst["target"], np.abs(g[4] - r[4]).max()); worst["kin"] = max(worst["kin"], np.abs(g[1] - r[1]).max())
    print(f"swing legs, set {name}: state / foot_pos_cur bit for bit, worst |d foot_pos_target_last_time| {worst['target']:.2e}, |d foot_forces_kin| {worst['kin']:.2e} N "
          f"(bar {G.force_bar(ps):.3e})")
    assert worst["target"] <= 1e-15 and worst["kin"] <= G.force_bar(ps), worst


# ---------------------------------------------------------------------------------------------------------------- leg state, EKF, joint torques
LEG_BARS = (("foot_pos_rel", 1e-14), ("Jb", 1e-14), ("foot_vel_rel", 1e-13), ("foot_pos_abs", 1e-14), ("foot_vel_abs", 1e-13), ("foot_pos_world", 1e-14), ("foot_vel_world", 1e-13))


def test_leg_state_at_another_geometry(pkg, oracle, scen):
    """a1mpc_leg_state_batch with set A's rho_fix (all five entries different from leg to leg) and rho_opt: the bars of test_leg_state_N4b times the ratio of the largest
    reach |ox| + |oy| + |d| + lt + lc to the A1's (gpu_common.LEG_BAR_SCALE)."""
    ps = PARAM_SETS["A"]
    rng = np.random.default_rng(41)
    q = rng.uniform(-1.2, 1.2, (N, 12)); qd = rng.normal(0, 3, (N, 12))
    eul = rng.uniform(-0.5, 0.5, (N, 3)); eul[:, 2] = rng.uniform(-3, 3, N); R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(N, 9)
    pos = rng.normal(0, 2, (N, 3)); vel = rng.normal(0, 1, (N, 3))
    names = [k for k, _ in LEG_BARS]
    run = lambda **kw: tuple(np.array([oracle.leg_state(q[b], qd[b], R[b], pos[b], vel[b], **kw)[k] for b in range(N)]) for k in names)
    full = run(rho_fix=ps["rho_fix"], rho_opt=ps["rho_opt"])
    assert_sensitive("leg state, set A", full, dict(rho_fix=run(rho_opt=ps["rho_opt"]), rho_opt=run(rho_fix=ps["rho_fix"])))
    with pkg.Engine(_cfg(pkg, scen), CAP, 0) as eng:
        out = eng.leg_state(q, qd, R, pos, vel, rho_fix=ps["rho_fix"], rho_opt=ps["rho_opt"])
    worst = {k: float(np.abs(out[k] - r).max()) for k, r in zip(names, full)}
    print(f"leg state, set A (bars x {G.LEG_BAR_SCALE:.4f}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, tol in LEG_BARS:
        assert worst[k] <= tol * G.LEG_BAR_SCALE, (k, worst[k])


def ekf_inputs(scen, n, ticks, seed):
    rng = np.random.default_rng(seed)
    base = np.array([0.18, 0.13, -0.3, 0.18, -0.13, -0.3, -0.18, 0.13, -0.3, -0.18, -0.13, -0.3])
    steps = []
    for t in range(ticks):
        mm = np.where(rng.random(n) < 0.8, 1, 0).astype(np.uint8) if t > 3 else np.zeros(n, np.uint8)
        yaw = rng.uniform(-3, 3, n); eul = rng.normal(0, 0.05, (n, 2)); R = scen.rot_zyx(eul[:, 0], eul[:, 1], yaw).reshape(n, 9)
        steps.append((mm, rng.choice(np.concatenate([G.FORCE_EKF, rng.uniform(0, 160, 6)]), size=(n, 4)), R, np.array([0.0, 0.0, 9.81]) + rng.normal(0, 0.3, (n, 3)),
                      rng.normal(0, 0.3, (n, 3)), base + rng.normal(0, 0.01, (n, 12)), rng.normal(0, 0.3, (n, 12))))
    return steps


def ekf_oracle_run(oracle, steps, n, dt, flat, device):
    states = [oracle.ekf_state() for _ in range(n)]
    pos = np.zeros((n, len(steps), 3)); vel = np.zeros((n, len(steps), 3)); ec = np.zeros((n, len(steps), 4), np.uint8)
    for t, (mm, ff, R, acc, w, fk, fv) in enumerate(steps):
        for b in range(n):
            pos[b, t], vel[b, t], ec[b, t] = oracle.ekf_step(states[b], dt, mm[b], ff[b], R[b], acc[b], w[b], fk[b], fv[b], assume_flat_ground=flat, device=device)
    return pos, vel, ec


@pytest.mark.parametrize("flat,dt", [(0, 0.002), (0, 0.005), (0, 0.0025), (1, 0.005)])
def test_ekf_without_flat_ground_and_at_other_dt(pkg, oracle, scen, flat, dt):
    """a1mpc_ekf_update_batch at assume_flat_ground = 0 and at the sets' control_dt, 80 ticks (as test_ekf_N4c_sequence): bit for bit against the oracle's device variant,
    within 1e-10 of the pinned variant (which tests/test_ref_pin.py holds to A1BasicEKF(false) and to these dt)."""
    ticks = 80
    steps = ekf_inputs(scen, N, ticks, 51 + int(dt * 1e4) + flat)
    dev = ekf_oracle_run(oracle, steps, N, dt, flat, True)
    back = {}
    if flat != 1:
        back["assume_flat_ground"] = ekf_oracle_run(oracle, steps, N, dt, 1, True)
    if dt != 0.0025:
        back["dt"] = ekf_oracle_run(oracle, steps, N, 0.0025, flat, True)
    assert_sensitive(f"EKF flat {flat} dt {dt}", dev, back)
    pinned = ekf_oracle_run(oracle, steps, N, dt, flat, False)
    worst = 0.0
    with pkg.Engine(_cfg(pkg, scen), CAP, 0) as eng:
        for t, (mm, ff, R, acc, w, fk, fv) in enumerate(steps):
            pos, vel, ec = eng.ekf_update(dt, mm, ff, R, acc, w, fk, fv, assume_flat_ground=flat)
            assert np.array_equal(pos, dev[0][:, t]) and np.array_equal(vel, dev[1][:, t]) and np.array_equal(ec, dev[2][:, t]), (t, np.abs(pos - dev[0][:, t]).max())
            worst = max(worst, np.abs(pos - pinned[0][:, t]).max(), np.abs(vel - pinned[1][:, t]).max())
            assert np.array_equal(ec, pinned[2][:, t]), t
    print(f"EKF flat {flat} dt {dt}: bit for bit against the device variant, worst distance to the pinned variant {worst:.2e}")
    assert worst <= 1e-10, worst


def test_joint_torques_at_another_km(pkg, oracle, scen):
    """a1mpc_joint_torques_batch with set A's km_foot (0.2, 0.05, 0.08): bit for bit, every pivot pattern and a singular block as in test_joint_torques_N3_bit_exact"""
    ps = PARAM_SETS["A"]
    rng = np.random.default_rng(11)
    n = N
    Jb = rng.normal(0, 0.2, (n, 4, 9)); Jb[:, :, [0, 4, 8]] += rng.choice([-0.3, 0.3], size=(n, 4, 3)); Jb[5, 1] = 0.0
    c = (rng.random((n, 4)) < 0.5).astype(np.uint8); act = (rng.random(n) < 0.9).astype(np.uint8); c[5, 1] = 0; act[5] = 1
    grf = rng.normal(0, 40, (n, 12)); fk = rng.normal(0, 20, (n, 12)); tg = rng.normal(0, 1, (n, 12)); prev = rng.normal(0, 5, (n, 12))
    run = lambda km: (np.array([oracle.joint_torques(act[b], c[b], Jb[b].reshape(36), grf[b], fk[b], np.array(km), tg[b], prev[b]) for b in range(n)]),)
    full = run(ps["km_foot"])
    assert_sensitive("joint torques, set A", full, dict(km_foot=run((0.1, 0.1, 0.04))))
    with pkg.Engine(_cfg(pkg, scen), CAP, 0) as eng:
        tau = eng.joint_torques(act, c, Jb.reshape(n, 36), grf, fk, np.array(ps["km_foot"]), tg, prev)
    assert np.array_equal(tau, full[0], equal_nan=True), np.argwhere(tau != full[0])[:4]
    print(f"joint torques, set A: {n} robots bit for bit (worst distance 0)")


# ---------------------------------------------------------------------------------------------------------------- horizon preview
@pytest.mark.parametrize("footholds", [False, True])
@pytest.mark.parametrize("name", SETS)
def test_horizon_preview_at_other_gaits(pkg, oracle, scen, name, footholds):
    """a1mpc_horizon_preview_batch / _footholds_batch at the set's gait on an engine whose MPC dt is 0.004.  The schedule, byte for byte, is the oracle's update_plan run
    forward at the set's gait (tests/test_gpu_horizon_preview.py::_oracle_plan_forward), and >= 40 % of the walking robots switch inside the horizon.  The per-step feet
    are the numpy loop f = f - (v * dt) with the HANDLE's dt, bit for bit (with footholds: the rule of tests/test_gpu_foothold_preview.py).  The three dt of the call all
    differ -- the MPC's 0.004, the tick's control_dt and the gait's control_dt, which for set A is moved to 0.003 in this test only (the preview reads neither of the latter
    two) -- and the numpy feet at either of the other two differ from the expected ones."""
    from test_gpu_foothold_preview import _bits, _command, _rule, _touchdowns
    from test_gpu_horizon_preview import _oracle_plan_forward
    ps = dict(PARAM_SETS[name])
    if ps["gait_dt"] == 0.004:
        ps["gait_dt"] = 0.003
    mpc_dt, h, tps, mode = 0.004, 10, 2, 2
    assert len({mpc_dt, ps["gait_dt"], ps["control_dt"]}) == 3 or name == "B"     # (set B: its two control_dt are equal by design, both differ from the MPC's)
    assert mpc_dt not in (ps["gait_dt"], ps["control_dt"])
    rng = np.random.default_rng(900 + ord(name) + footholds)
    n = N
    gc, spd, _ = _fleet(ps, n, 4, stand=False)
    mm = np.where(np.arange(n) % 6 == 5, 0, 1).astype(np.uint8)
    plan_now = (gc <= ps["counter_per_swing"]).astype(np.uint8)
    contacts = np.where(mm[:, None] == 1, plan_now | (rng.random((n, 4)) < 0.1), 1).astype(np.uint8)
    dfp = np.asarray(ps["default_foot_pos"])
    foot = dfp + rng.normal(0, 0.05, (n, 12)); T = dfp + rng.normal(0, 0.05, (n, 12))
    vd = rng.normal(0, 0.6, (n, 3)); eul = rng.normal(0, 0.2, (n, 3)); eul[:, 2] = rng.uniform(-3, 3, n)
    R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)
    # ---- the yardstick: schedule from the oracle, feet from numpy
    plan = _oracle_plan_forward(oracle, mm, gc, spd, h, tps, gp=G.oracle_gait(oracle, ps))
    plan_back = {f"gait.{k}": _oracle_plan_forward(oracle, mm, gc, spd, h, tps, gp=G.oracle_gait(oracle, ps, **{k: v}))
                 for k, v in (("counter_per_gait", 240.0), ("counter_per_swing", 120.0)) if ps[k] != v}     # (set A's gait.counter_per_swing is 120)
    expect_sched = np.concatenate([contacts[:, None, :], plan], axis=1)
    walking = mm == 1
    seq = np.concatenate([plan_now[:, None, :], plan], axis=1)[walking]
    switched = (seq != seq[:, :1]).any(axis=(1, 2)).mean()
    print(f"preview, set {name}: {switched:.3f} of the walking robots switch inside the horizon")
    assert switched >= 0.4, switched
    td = _touchdowns(expect_sched, n, h) if footholds else np.zeros((n, h, 4), bool)
    feet = lambda dt: _rule(foot, T, _command(R, vd, mode) * dt, td)
    expect_feet = feet(mpc_dt)
    assert_sensitive(f"preview, set {name}", (expect_sched[:, 1:], expect_feet), dict({k: (v, expect_feet) for k, v in plan_back.items()}, mpc_dt_default=(plan, feet(0.0025)),
                                                                                      mpc_dt_taken_from_the_gait=(plan, feet(ps["gait_dt"])),
                                                                                      mpc_dt_taken_from_the_tick=(plan, feet(ps["control_dt"]))))
    if footholds:
        assert td.any(axis=(1, 2))[walking].mean() >= 0.2
    with pkg.Engine(_cfg(pkg, scen, h, dt=mpc_dt), CAP, 0) as eng:
        pv = eng.preview_config(contact_schedule=1, foot_preview=mode, ticks_per_step=tps)
        out = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=pv, gait=G.gait_config(pkg.engine, ps), foot_target_abs=T if footholds else None)
    got_s = out["contact_sched"].reshape(n, h, 4); got_f = out["foot_steps"].reshape(n, h, 4, 3)
    assert np.array_equal(got_s, expect_sched), np.argwhere(got_s != expect_sched)[:5]
    assert np.array_equal(_bits(got_f), _bits(expect_feet)), np.abs(got_f - expect_feet).max()
    print(f"preview, set {name}, footholds {footholds}: schedule byte for byte, feet bit for bit (worst distance 0)")


# ---------------------------------------------------------------------------------------------------------------- the one-call ticks
PITCH0 = 0.0625     # root_euler_d[:, 1] the tick worlds start from: with use_terrain_adapt = 0 it must come back bit-unchanged on every tick
_PRECONDITIONS_SHOWN = set()


def _stage_params(ps, adapt):
    """what each stage of a tick is to receive according to include/a1mpc.h, one entry per (stage, argument)"""
    return dict(rho_fix=np.asarray(ps["rho_fix"]), rho_opt=np.asarray(ps["rho_opt"]), ekf_dt=ps["control_dt"], flat=ps["assume_flat_ground"],
                counter_per_gait=ps["counter_per_gait"], plan_cps=ps["counter_per_swing"], plan_dt=ps["gait_dt"], dx=ps["foot_delta_x_limit"], dy=ps["foot_delta_y_limit"],
                default_foot_pos=np.asarray(ps["default_foot_pos"]), reset=tuple(ps["gait_counter_reset"]), swing_cps=ps["counter_per_swing"], swing_dt=ps["control_dt"],
                kp=tuple(ps["kp_foot"]), kd=tuple(ps["kd_foot"]), contact_cps=ps["contact_per_swing"], low=ps["foot_force_low"], adapt=adapt, km=np.array(ps["km_foot"]))


def _oracle_front_chain(oracle, raws, gc0, robots, P, grf):
    """The stages of a control tick around the MPC on the ORACLE, chained as include/a1mpc.h chains them, for the robots `robots` over the ticks of `raws` (the tick's own
    inputs): leg state -> EKF (device variant) -> update_plan -> swing legs -> contacts / terrain -> joint torques (fed the fixed forces `grf` in the MPC's place: no QP is
    solved here).  -> (len(robots), everything the stages produced, tick after tick)"""
    gp = oracle.gait_params(P["default_foot_pos"], counter_per_gait=P["counter_per_gait"], counter_per_swing=P["plan_cps"], control_dt=P["plan_dt"], dx=P["dx"], dy=P["dy"],
                            reset=P["reset"])
    rows = []
    for j, b in enumerate(robots):
        ekf, cst = oracle.ekf_state(), oracle.contact_state()
        pos, vel, gc, pitch, tau = np.array([0.0, 0.0, 0.3]), np.zeros(3), gc0[b].copy(), PITCH0, np.zeros(12)
        st = [np.zeros(12) for _ in range(3)]; row = []
        for t, r in enumerate(raws):
            leg = oracle.leg_state(r["joint_pos"][b], r["joint_vel"][b], r["R_world"][b], pos, vel, rho_fix=P["rho_fix"], rho_opt=P["rho_opt"])
            pos, vel, ec = oracle.ekf_step(ekf, P["ekf_dt"], r["movement_mode"][b], r["foot_force"][b], r["R_world"][b], r["imu_acc"][b], r["imu_ang_vel"][b],
                                           leg["foot_pos_rel"], leg["foot_vel_rel"], assume_flat_ground=P["flat"], device=True)
            gc, pc, rel, ab, wo = oracle.update_plan(gp, r["movement_mode"][b], gc, r["gait_counter_speed"][b], vel, r["R_z"][b], r["R_world"][b], pos, r["root_lin_vel_d"][b])
            cur, kin = oracle.swing_legs(r["R_z"][b], leg["foot_pos_abs"], gc, rel, st[0], st[1], st[2], kp=P["kp"], kd=P["kd"], counter_per_swing=P["swing_cps"], dt=P["swing_dt"])
            ct, rec, ang, pitch = oracle.contact_terrain_step(cst, gc, pc, r["foot_force"][b], leg["foot_pos_abs"], pos[2], pitch, counter_per_swing=P["contact_cps"],
                                                              foot_force_low=P["low"], use_terrain_adapt=P["adapt"])
            tau = oracle.joint_torques(r["mpc_active"][b], ct, leg["Jb"], grf[j, t], kin, P["km"], r["torques_gravity"][b], tau)
            row += [leg["foot_pos_rel"], leg["Jb"], leg["foot_pos_abs"], pos, vel, ec, gc, pc, rel, ab, wo, cur, kin, st[0], ct, rec, [ang, pitch], tau]
        rows.append(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in row]))
    return (np.array(rows),)


def tick_preconditions(oracle, ps, adapt, raws, gc0, mm_table, label):
    """The sensitivity precondition of the one-call ticks, on the oracle alone and on the tick's OWN inputs (its first ticks, a dozen robots of the blocks that stand):
    the stages chained as above with every field of a1mpc_tick_params put back to its default, one at a time, and with each confusion a tick could make between its
    duplicated fields -- the gait's control_dt for the swing legs or the EKF, the contact stage's counter_per_swing for the swing legs, the gait's for the contact
    logic -- give another result than the field-to-stage mapping of include/a1mpc.h.  With use_terrain_adapt = 0 this includes: at 1 the pitch would have moved.
    Variants that change nothing by construction are left out (set A's gait.counter_per_swing is 120; set B's pairs are equal by design; gait_counter_reset where no robot
    of the sample stands)."""
    key = (label, ps["name"], adapt)
    K = min(len(raws), 30)
    n = len(gc0)
    robots = [b for b in list(range(8)) + list(range(16, 20)) if b < n]
    P = _stage_params(ps, adapt)
    A1 = np.array([[0.1805, 0.047, 0.0838, 0.21, 0.21], [0.1805, -0.047, -0.0838, 0.21, 0.21], [-0.1805, 0.047, 0.0838, 0.21, 0.21], [-0.1805, -0.047, -0.0838, 0.21, 0.21]])
    variants = {
        "gait.counter_per_gait": dict(counter_per_gait=240.0), "gait.counter_per_swing": dict(plan_cps=120.0, swing_cps=120.0), "gait.control_dt": dict(plan_dt=0.0025),
        "gait.foot_delta_x_limit": dict(dx=0.1), "gait.foot_delta_y_limit": dict(dy=0.1), "gait.default_foot_pos": dict(default_foot_pos=G.DEFAULT_FOOT_POS),
        "gait.gait_counter_reset": dict(reset=(0.0, 120.0, 120.0, 0.0)), "contact.counter_per_swing": dict(contact_cps=120.0), "contact.foot_force_low": dict(low=30.0),
        "contact.use_terrain_adapt": dict(adapt=1), "control_dt": dict(ekf_dt=0.0025, swing_dt=0.0025), "assume_flat_ground": dict(flat=1),
        "kp_foot": dict(kp=(300.0, 400.0, 400.0)), "kd_foot": dict(kd=(8.0, 8.0, 8.0)), "km_foot": dict(km=np.array([0.1, 0.1, 0.04])), "rho_fix": dict(rho_fix=A1),
        "rho_opt": dict(rho_opt=np.zeros((4, 3))),
        "swing legs given gait.control_dt": dict(swing_dt=ps["gait_dt"]), "swing legs given contact.counter_per_swing": dict(swing_cps=ps["contact_per_swing"]),
        "contacts given gait.counter_per_swing": dict(contact_cps=ps["counter_per_swing"]), "EKF given gait.control_dt": dict(ekf_dt=ps["gait_dt"])}
    same = lambda over: all(np.array_equal(np.asarray(P[k]), np.asarray(v)) for k, v in over.items())
    variants = {k: v for k, v in variants.items() if not same(v)}
    if not (mm_table[:K][:, robots] == 0).any():
        variants.pop("gait.gait_counter_reset")
    if key in _PRECONDITIONS_SHOWN:     # (same inputs as a case before: the inputs depend on the set, the batch and the timetable alone)
        return
    grf = np.random.default_rng(3).normal(0, 40, (len(robots), K, 12))
    full = _oracle_front_chain(oracle, raws[:K], gc0, robots, P, grf)
    assert_sensitive(f"tick, {label}, set {ps['name']}, adapt {adapt}", full, {k: _oracle_front_chain(oracle, raws[:K], gc0, robots, dict(P, **v), grf) for k, v in variants.items()})
    _PRECONDITIONS_SHOWN.add(key)


# entry -> (contact_schedule, foot_preview, ticks_per_step, footholds) of the preview entries; None: no preview config
ENTRIES = dict(plain=None, preview=(1, 0, 1, False), footholds=(1, 1, 2, True), balance=None, sensors=None)
# (entry, set, n, warm_start, ticks; None = one cycle of the slowest leg, contact.use_terrain_adapt).  n = 67: the latency kernel, torques in its output stage from the first
# tick on; n = 2100: the first tick goes through the split pipeline (torques by a launch of their own), the warm ticks through the cost-ordered fused kernel.
# use_terrain_adapt = 0 (set A; set B alternates): the tick's contact stage reads and writes root_euler_d[1] in place, and has to leave it alone
TICK_CASES = ([(e, s, N, w, None, a) for e in ENTRIES for s, w, a in (("A", 1, 1), ("B", 2, 0 if e in ("preview", "sensors") else 1))]
              + [(e, "A", N, 1, None, 0) for e in ("plain", "preview", "footholds")] + [("plain", "A", 2100, 1, 8, 1), ("preview", "A", 2100, 1, 8, 0)])


def _run_one_call(e1, entry, prm, pv, bf, n, st, extra):
    if entry == "plain":
        e1.control_tick_device(prm, bf, n, stream=st.cuda_stream)
    elif entry == "preview":
        e1.control_tick_preview_device(prm, pv, bf, n, stream=st.cuda_stream)
    elif entry == "footholds":
        e1.control_tick_preview_footholds_device(prm, pv, bf, n, stream=st.cuda_stream)
    elif entry == "balance":
        e1.control_tick_balance_device(prm, extra["bt"], bf, n, stream=st.cuda_stream)
    else:
        e1.control_tick_sensors_device(prm, extra["ts"], bf, n, stream=st.cuda_stream)


@pytest.mark.parametrize("entry,name,n,warm,ticks,adapt", TICK_CASES)
def test_one_call_ticks_equal_the_chain_at_other_parameters(pkg, oracle, scen, entry, name, n, warm, ticks, adapt):
    """The five one-call ticks -- a1mpc_control_tick_device, _preview_device, _preview_footholds_device, _balance_device, _sensors_device -- with the set's
    a1mpc_tick_params against the *_device entries chained by hand on a second handle (gpu_common.TickChain, the balance chain of tests/test_gpu_balance_tick.py, the
    sensor and command entries in front of TickChain), which follow the field-to-stage mapping of include/a1mpc.h: every field of a1mpc_tick_buffers, the carried state,
    iters and status equal (NaN-aware) on every tick of one cycle of the slowest leg, staggered fleet, stand timetable, forces on the 45 N / 50 N thresholds.  The counters
    and planned contacts are numpy's loop at the set's gait.  torques_fused is asserted per regime.  root_euler_d[:, 1] starts at 0.0625 in both worlds; with
    contact.use_terrain_adapt = 0 it comes back bit-unchanged on every tick (the sensors entry excepted, whose command stage integrates the pitch rate into it), after
    the oracle has shown on the same inputs that at use_terrain_adapt = 1 it would have moved (tick_preconditions)."""
    import torch
    from test_gpu_balance_tick import _chain_tick
    import test_gpu_sensor_frontend as SF
    ps = PARAM_SETS[name]
    gk = G.gait_kw(ps)
    ticks = int(ps["counter_per_gait"] / min(PARAM_SPEEDS)) if ticks is None else ticks
    stand = entry != "sensors"                        # (the sensors entry makes movement_mode itself: every robot walks from the first tick on)
    rng = np.random.default_rng(8000 + n + ord(name) + stand)
    E = pkg.engine; h = 10
    cfg = _cfg(pkg, scen, h, warm_start=warm)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gc0, spd, mm_table = _fleet(ps, n, ticks, stand=stand)
    raws = [tick_inputs_timetable(scen, rng, n, mm_table[t], spd, forces=G.force_values(ps)) for t in range(ticks)]
    tick_preconditions(oracle, ps, adapt, raws, gc0, mm_table, f"n {n}, {ticks} ticks, {'stand timetable' if stand else 'walking'}")
    cap = max(n, CAP)
    with pkg.Engine(cfg, cap, 0) as e1, pkg.Engine(cfg, cap, 0) as e7:
        prm = G.tick_params(E, ps, adapt)
        st = torch.cuda.Stream(device=dev); sp = C.c_void_p(st.cuda_stream)
        pv = None
        if ENTRIES[entry] is not None:
            sched, feet, tps, footholds = ENTRIES[entry]
            pv = e1.preview_config(contact_schedule=sched, foot_preview=feet, ticks_per_step=tps)
        chain = TickChain(e7, prm, n, st, preview=pv, footholds=entry == "footholds")
        w1, w7 = tick_world(n, dev, gc0), tick_world(n, dev, gc0)
        for w in (w1, w7):
            w["state"]["root_euler_d"][:, 1] = PITCH0
        x1, x7 = {}, {}
        if entry == "balance":
            pos_d = T(np.array([0.0, 0.0, 0.3]) + rng.normal(0, 0.02, (n, 3)))
            for x in (x1, x7):
                x.update(root_pos_d=pos_d, root_acc=torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev),
                         f_world=torch.full((n, 12), float("nan"), dtype=torch.float64, device=dev))
            x1["bt"] = e1.balance_tick(pos_d, x1["root_acc"], x1["f_world"]); x7["bt"] = e7.balance_tick(pos_d)
        if entry == "sensors":
            fronts = [SF._front_world(torch, dev, n) for _ in range(2)]
        gc_np = gc0.copy(); fused_seen = []
        for t in range(ticks):
            mm = mm_table[t]
            raw = raws[t]
            inp = {k: T(v) for k, v in raw.items()}
            if entry == "sensors":
                cmd = np.c_[rng.uniform(-0.4, 0.4, (n, 2)), rng.normal(0, 0.02, n), rng.normal(0, 0.05, (n, 2)), rng.uniform(-0.4, 0.4, n)]
                toggle = np.full(n, 1 if t == 0 else 0, np.uint8)
                d = dict(quat=T(SF._quat_of_euler(raw["root_euler"])), imu_acc_raw=T(raw["imu_acc"]), imu_gyro_raw=T(raw["imu_ang_vel"]), cmd=T(cmd), mode_toggle=T(toggle))
                inp = {k: inp[k] for k in SF.RAW_KEYS}
                (f1, c1), (f7, c7) = fronts
                x1["ts"] = e1.tick_sensors(**d, **c1)
                inp1, inp7 = {**inp, **f1}, {**inp, **f7}
            else:
                inp1 = inp7 = inp
            torch.cuda.synchronize()
            # ---- one call
            _run_one_call(e1, entry, prm, pv, tick_buffers(E, inp1, w1), n, st, x1)
            fused_seen.append(e1.last_control_tick_ms()[1])
            # ---- the chain
            if entry == "balance":
                _chain_tick(e7, prm, x7["bt"], n, sp, inp7, w7, x7)
            else:
                if entry == "sensors":
                    e7.sensor_frontend_device(n, d["quat"], d["imu_acc_raw"], d["imu_gyro_raw"], f7["R_world"], f7["R_z"], f7["root_euler"], f7["imu_acc"], f7["imu_ang_vel"],
                                              f7["root_ang_vel"], stream=st.cuda_stream)
                    e7.command_device(n, d["cmd"], d["mode_toggle"], w7["state"]["root_pos"], prm.control_dt, c7["body_height"], c7["ctrl_state"], w7["state"]["root_euler_d"],
                                      c7["root_pos_d"], c7["kp_linear_xy"], c7["mpc_init_counter"], f7["root_lin_vel_d"], f7["root_ang_vel_d"], f7["movement_mode"],
                                      f7["mpc_active"], f7["root_pos_d_z"], stream=st.cuda_stream)
                chain.tick(inp7, w7)
            st.synchronize(); torch.cuda.synchronize()
            assert_worlds_equal(t, w1, w7)
            if entry == "balance":
                for k in ("root_acc", "f_world"):
                    assert np.array_equal(x1[k].cpu().numpy(), x7[k].cpu().numpy(), equal_nan=True), (t, k)
            if entry == "sensors":
                for k in list(f1) + list(c1):
                    a, b = f1.get(k, c1.get(k)).cpu().numpy(), f7.get(k, c7.get(k)).cpu().numpy()
                    assert np.array_equal(a, b, equal_nan=True), (t, k)
                assert (f1["movement_mode"].cpu().numpy() == 1).all(), t
            if adapt == 0 and entry != "sensors":
                assert (w1["state"]["root_euler_d"][:, 1].cpu().numpy() == PITCH0).all(), t
            # ---- the anchor: counters and planned contacts are numpy's loop at the set's gait
            gc_np, pc_np = G.gait_loop(gc_np, spd, mm, **gk)
            assert np.array_equal(w1["state"]["gait_counter"].cpu().numpy(), gc_np) and np.array_equal(w1["u8"]["plan_contacts"].cpu().numpy(), pc_np), t
        assert np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1
        if entry in ("footholds", "balance"):
            assert fused_seen == [False] * ticks, fused_seen       # per-step feet solve on the general kernels, the balance QP has no output stage: a launch of their own
        else:
            assert fused_seen == ([True] * ticks if n <= 2048 else [False] + [True] * (ticks - 1)), fused_seen
    print(f"{entry}, set {name}, n {n}, warm {warm}, use_terrain_adapt {adapt}: {ticks} ticks, every field equal to the chain (worst distance 0); torques_fused {fused_seen[0]} then {fused_seen[-1]}")


@pytest.mark.parametrize("entry", ["plain", "preview"])
def test_km_foot_changed_between_warm_ticks_reaches_the_fused_output_stage(pkg, oracle, scen, entry):
    """The one-call tick uploads km_foot once and again when it changes; its fused output stage reads the device copy.  Set A, 67 robots, 14 ticks: km_foot goes to other
    values at tick 5 and back at tick 9 (use_terrain_adapt 1 on the plain tick, 0 on the preview tick); the one-call tick equals the chain (whose torque entry takes km_foot as a host array on every call) on every tick across both
    switches, and torques_fused is 1 on every tick: the cached copy is the one being read.  On the oracle first: the two km_foot give different torques."""
    import torch
    ps = PARAM_SETS["A"]
    n, ticks, h = N, 14, 10
    km_a, km_b = np.array(ps["km_foot"]), np.array([0.07, 0.3, 0.11])
    rng = np.random.default_rng(77)
    Jb = rng.normal(0, 0.2, (n, 36)); Jb[:, [0, 4, 8, 9, 13, 17, 18, 22, 26, 27, 31, 35]] += 0.3
    grf = rng.normal(0, 40, (n, 12)); fk = rng.normal(0, 20, (n, 12)); ct = (rng.random((n, 4)) < 0.5).astype(np.uint8)
    run = lambda km: (np.array([oracle.joint_torques(1, ct[b], Jb[b], grf[b], fk[b], km, np.zeros(12), np.zeros(12)) for b in range(n)]),)
    assert_sensitive("km_foot switch", run(km_a), dict(km_foot_other=run(km_b), km_foot_default=run(np.array([0.1, 0.1, 0.04]))))
    E = pkg.engine
    cfg = _cfg(pkg, scen, h, warm_start=1)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gc0, spd, mm_table = _fleet(ps, n, ticks, stand=False)
    with pkg.Engine(cfg, CAP, 0) as e1, pkg.Engine(cfg, CAP, 0) as e7:
        prm = G.tick_params(E, ps, adapt=0 if entry == "preview" else 1)
        st = torch.cuda.Stream(device=dev)
        pv = e1.preview_config(contact_schedule=1, foot_preview=0, ticks_per_step=1) if entry == "preview" else None
        chain = TickChain(e7, prm, n, st, preview=pv)
        w1, w7 = tick_world(n, dev, gc0), tick_world(n, dev, gc0)
        fused_seen = []; swing_seen = 0
        for t in range(ticks):
            prm.km_foot[:] = list(km_b if 5 <= t < 9 else km_a)
            inp = {k: T(v) for k, v in tick_inputs_timetable(scen, rng, n, mm_table[t], spd, forces=G.force_values(ps)).items()}
            torch.cuda.synchronize()
            if pv is None:
                e1.control_tick_device(prm, tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
            else:
                e1.control_tick_preview_device(prm, pv, tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
            fused_seen.append(e1.last_control_tick_ms()[1])
            chain.tick(inp, w7)
            st.synchronize()
            assert_worlds_equal(t, w1, w7)
            active = inp["mpc_active"].cpu().numpy()[:, None] == 1
            swing_seen += int(((w1["u8"]["contacts"].cpu().numpy() == 0) & active).sum())     # km_foot acts on the swing legs of the active robots
        assert fused_seen == [True] * ticks, fused_seen
        assert swing_seen >= ticks * n // 4, swing_seen
    print(f"km_foot switch, {entry}: {ticks} ticks equal to the chain across both switches (worst distance 0), torques_fused on every tick, {swing_seen} swing legs")
