"""GPU, through the C ABI: the foot preview that lands swing legs on their planned footholds -- a1mpc_horizon_preview_footholds_batch(_device),
a1mpc_control_tick_preview_footholds_device and a1mpc_pipeline_submit_ticks_strided_device.  The rule: f_0 = foot_pos_abs; at a touchdown of the schedule (contact bit t set,
bit t - 1 clear, t >= 1) f_t is the words of this tick's foot_pos_target_abs (update_plan's Raibert foothold, S/A1RobotControl.cpp:166-199); otherwise f_t = f_(t-1) - v * dt
(S/test/test_mpc.cpp:112-115).  The yardsticks are the numpy loop of that rule driven by the EXISTING entry's schedule (which test_schedule_is_update_plan_run_forward holds
to the oracle), the oracle's solves and the entries that existed before -- never the new code against itself."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import TICK_OUT_F64, TICK_STATE, _engine, tick_inputs
from helpers import TOL_FORCE_N

pytestmark = pytest.mark.gpu

DEFAULT_FOOT_POS = [0.17, 0.15, -0.35, 0.17, -0.15, -0.35, -0.17, 0.15, -0.35, -0.17, -0.15, -0.35]
PER_GAIT, PER_SWING = 240.0, 120.0   # counter_per_gait / counter_per_swing, S/A1CtrlStates.h:24-25


def _gait_inputs(rng, n, h, tps):
    """the gait inputs of the horizon-preview tests (counters uniform in [0, 240) with the reset pattern and a 239.0 wrap case, per-leg speeds from {1, 1.5, 2, 3}, 80 % of the
    robots walking, every third robot with leg 0 close to a switch), and in addition: on every second robot leg 0 starts at mod(240 - u (h - 1) tps speed, 240) with u in
    (0.05, 0.95), so it crosses 240 -- a touchdown -- inside the horizon.  A step advances at most 16 * 3 = 48 counts, so a sampled step cannot jump over the 120-count stance
    window: the sample before the crossing is in swing, the one after it in stance.  Returns (movement_mode, gait_counter, speed, contacts); contacts are planned or early
    contact (S/A1RobotControl.cpp:271), and exactly the plan on leg 0 of those second robots."""
    mm = (rng.random(n) < 0.8).astype(np.uint8)
    gc = rng.uniform(0, PER_GAIT, (n, 4)); gc[::7] = [0, 120, 120, 0]; gc[::11, 0] = 239.0
    spd = rng.choice([1.0, 1.5, 2.0, 3.0], size=(n, 4))
    k = np.arange(0, n, 3)
    edge = rng.choice([PER_SWING, PER_GAIT], size=len(k))
    gc[k, 0] = np.mod(edge - rng.uniform(0, 1, len(k)) * (h - 1) * tps * spd[k, 0], PER_GAIT)
    j = np.arange(0, n, 2)
    gc[j, 0] = np.mod(PER_GAIT - rng.uniform(0.05, 0.95, len(j)) * (h - 1) * tps * spd[j, 0], PER_GAIT)
    plan_now = (gc <= PER_SWING).astype(np.uint8)
    early = rng.random((n, 4)) < 0.1; early[j, 0] = False
    contacts = np.where(mm[:, None] == 1, plan_now | early, 1).astype(np.uint8)
    return mm, gc, spd, contacts


def _touchdowns(sched, n, h):
    """(n, h, 4) bool: contact at step t and none at step t - 1 (never at step 0)"""
    c = sched.reshape(n, h, 4)
    td = np.zeros((n, h, 4), bool)
    td[:, 1:] = (c[:, 1:] == 1) & (c[:, :-1] == 0)
    return td


def _command(R, vd, mode):
    """the velocity of the recurrence: the body-frame command (1) or R_world * command summed left to right (2, S/A1RobotControl.cpp:470)"""
    return vd if mode == 1 else np.stack([R[:, 3 * r] * vd[:, 0] + R[:, 3 * r + 1] * vd[:, 1] + R[:, 3 * r + 2] * vd[:, 2] for r in range(3)], axis=1)


def _rule(foot, T, s, td):
    """the rule as a plain float64 loop: one rounded product s = v * dt (the caller's), one subtraction per step, T copied at a touchdown"""
    n, h = td.shape[:2]
    f = foot.reshape(n, 4, 3).copy(); Tl = T.reshape(n, 4, 3)
    out = np.zeros((n, h, 4, 3)); out[:, 0] = f
    for t in range(1, h):
        f = np.where(td[:, t, :, None], Tl, f - s[:, None, :])
        out[:, t] = f
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _share(td, mm, n, h, tps):
    share = td.any(axis=(1, 2))[mm == 1].mean()
    print(f"n {n} h {h} tps {tps}: {share:.3f} of the walking robots have a touchdown inside the horizon (reference schedule)")
    return share


def _kinematics(scen, rng, n):
    foot = np.tile(DEFAULT_FOOT_POS, (n, 1)) + rng.normal(0, 0.05, (n, 12))
    T = np.tile(DEFAULT_FOOT_POS, (n, 1)) + rng.normal(0, 0.05, (n, 12))   # far from the feet and independent of them
    vd = rng.normal(0, 0.6, (n, 3)); vd[::5] *= 1000.0; vd[::7, 2] = 0.0
    eul = rng.normal(0, 0.2, (n, 3)); eul[:, 2] = rng.uniform(-3, 3, n)
    return foot, T, vd, scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)


@pytest.mark.parametrize("tps", [1, 3, 16])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("h", [4, 10, 20])
@pytest.mark.parametrize("n", [5000, 1, 67])
def test_feet_are_the_rule_bit_for_bit(pkg, scen, n, h, mode, tps):
    """1. All n x 12 h doubles against the numpy loop of the rule, driven by the EXISTING entry's schedule; the touchdown steps hold the exact words of T and the step after a
    touchdown is T - s.  The feet are the same whether or not the schedule is an output (the lane computes its contact bits for the feet alone), and the schedule that comes
    with them is the existing entry's.  For n >= 67 the reference schedule must show a touchdown at a step >= 1 on >= 40 % of the walking robots, or today's recurrence
    would pass."""
    rng = np.random.default_rng(1200 + 100 * h + 10 * tps + mode)
    mm, gc, spd, contacts = _gait_inputs(rng, n, h, tps)
    foot, T, vd, R = _kinematics(scen, rng, n)
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h)
    with pkg.Engine(cfg, n, 0) as eng:
        pv = eng.preview_config(contact_schedule=1, foot_preview=mode, ticks_per_step=tps)
        ref = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=pv)
        out = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=pv, foot_target_abs=T)
        alone = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=pv, want_schedule=False, foot_target_abs=T)
    td = _touchdowns(ref["contact_sched"], n, h)
    if n >= 67:
        assert _share(td, mm, n, h, tps) >= 0.4
    assert np.array_equal(out["contact_sched"], ref["contact_sched"])
    s = _command(R, vd, mode) * float(cfg.dt)
    expect = _rule(foot, T, s, td)
    got = out["foot_steps"].reshape(n, h, 4, 3)
    assert np.array_equal(_bits(got), _bits(expect)), np.abs(got - expect).max()
    assert alone["contact_sched"] is None and np.array_equal(_bits(alone["foot_steps"]), _bits(out["foot_steps"]))
    Tl = np.broadcast_to(T.reshape(n, 1, 4, 3), (n, h, 4, 3))
    assert np.array_equal(_bits(got[td]), _bits(Tl[td]))   # the words of T, copied
    after = np.zeros_like(td); after[:, 1:] = td[:, :-1]   # (no touchdown follows a touchdown: the leg is in contact)
    assert not (after & td).any()
    Ts = np.broadcast_to((T.reshape(n, 4, 3) - s[:, None, :])[:, None], (n, h, 4, 3))
    assert np.array_equal(_bits(got[after]), _bits(Ts[after]))
    if td.any():
        assert not np.array_equal(got, ref["foot_steps"].reshape(n, h, 4, 3))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("h", [4, 10, 20])
@pytest.mark.parametrize("n", [5000, 1, 67])
def test_where_nothing_lands_nothing_changes(pkg, scen, n, h, mode):
    """1b. Robots without a touchdown in the reference schedule have feet array_equal to a1mpc_horizon_preview_batch's; with contact_schedule 0 (no touchdown can exist)
    that holds for every robot; the schedule output is the existing entry's in both cases."""
    tps = 3
    rng = np.random.default_rng(2200 + 100 * h + mode)
    mm, gc, spd, contacts = _gait_inputs(rng, n, h, tps)
    foot, T, vd, R = _kinematics(scen, rng, n)
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h)
    with pkg.Engine(cfg, n, 0) as eng:
        for sched in (1, 0):
            pv = eng.preview_config(contact_schedule=sched, foot_preview=mode, ticks_per_step=tps)
            ref = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=pv)
            out = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=pv, foot_target_abs=T)
            assert np.array_equal(out["contact_sched"], ref["contact_sched"])
            quiet = ~_touchdowns(ref["contact_sched"], n, h).any(axis=(1, 2))
            if sched == 0:
                assert quiet.all() and np.array_equal(ref["contact_sched"], np.tile(contacts, (1, h)))
            elif n >= 67:
                assert quiet.any() and not quiet.all()
            assert np.array_equal(_bits(out["foot_steps"][quiet]), _bits(ref["foot_steps"][quiet]))


@pytest.mark.parametrize("h,n", [(10, 300), (16, 96), (20, 64), (6, 5)])
def test_solve_parity_on_foothold_feet(pkg, oracle, scen, h, n):
    """2. a1mpc_solve_batch_ticks_strided on the foothold feet + schedule against the oracle's strided formation (every third QP): same iteration count and status on every
    sampled QP, forces within TOL_FORCE_N."""
    tps = 3
    rng = np.random.default_rng(5200 + h)
    sc = scen.config3_random_flat(nb=n, horizon=h)
    mm, gc, spd, contacts = _gait_inputs(rng, n, h, tps)
    T = np.tile(DEFAULT_FOOT_POS, (n, 1)) + rng.normal(0, 0.05, (n, 12))
    with _engine(pkg, sc, n, warm_start=0) as eng:
        pv = eng.preview_config(contact_schedule=1, foot_preview=2, ticks_per_step=tps)
        ref = eng.horizon_preview(mm, gc, spd, contacts, sc["foot"], sc["R"], sc["tick"][:, 15:18], preview=pv)
        p = eng.horizon_preview(mm, gc, spd, contacts, sc["foot"], sc["R"], sc["tick"][:, 15:18], preview=pv, foot_target_abs=T)
        foot, contact = np.ascontiguousarray(p["foot_steps"]), np.ascontiguousarray(p["contact_sched"])
        out = eng.solve_ticks_strided(sc["tick"], sc["R"], foot, 12, contact, 4, want_u=True)
    td = _touchdowns(ref["contact_sched"], n, h)
    assert np.array_equal(contact, ref["contact_sched"])
    if n >= 64:
        assert _share(td, mm, n, h, tps) >= 0.4
    landed = td.any(axis=(1, 2))
    assert (np.abs(foot - ref["foot_steps"]).max(axis=1)[landed] > 1e-3).all()   # the QPs that are solved do stand on other feet than today's
    pr = oracle.mpc_params(h, **{k: sc["params"][k] for k in ("dt", "mu", "fz_min", "fz_max", "q", "r", "mass", "inertia")}); st = oracle.default_settings()
    worst = 0.0
    for b in range(0, n, 3):
        r = oracle.mpc_solve(pr, st, sc["x0"][b], sc["xref"][b], sc["R"][b], foot[b], contact[b], foot_stride=12, contact_stride=4)
        assert out["iters"][b] == r["info"].iters and out["status"][b] == r["info"].status, (b, out["iters"][b], r["info"].iters)
        worst = max(worst, np.abs(out["u"][b] - r["u"]).max(), np.abs(out["grf"][b] - r["grf"]).max())
    print(f"h{h} x {n}: |du| vs the oracle {worst:.2e} N")
    assert worst <= TOL_FORCE_N, worst


def test_the_footholds_matter_and_are_physical(pkg, oracle, scen):
    """3. 256 robots, h = 10, a forward command; T = the oracle's update_plan on the same state.  Legs 1 and 2 of every other robot are in swing and land at one of the steps
    1 .. 9.  Solved once on the foothold feet and once on the existing entry's feet, both with the same schedule: the robots without a touchdown get array_equal outputs
    (the same kernel on the same input words), every robot with one gets another u_full somewhere from its touchdown step on.  No amount is asked of the step-0 GRF (a
    late change moves it by less than the solver's tolerance); the per-step maxima are printed."""
    n, h, tps = 256, 10, 4
    sc = scen.config3_random_flat(nb=n, horizon=h)
    tick = sc["tick"].copy(); tick[:, 15:18] = [0.5, 0.0, 0.0]   # the command, forward
    mm = np.ones(n, np.uint8); spd = np.full((n, 4), 2.0)
    gc = np.tile([0.0, 40.0, 40.0, 0.0], (n, 1))   # nobody switches within 9 * 4 * 2 = 72 counts ...
    step = 1 + np.arange(n // 2) % 9
    gc[::2, 1:3] = (PER_GAIT - 2.0 * tps * step)[:, None]   # ... but legs 1 and 2 of every other robot reach 240 at each of the steps 1 .. 9
    contacts = (gc <= PER_SWING).astype(np.uint8)
    gp = oracle.gait_params(DEFAULT_FOOT_POS)
    Rz = scen.rot_zyx(0 * tick[:, 2], 0 * tick[:, 2], tick[:, 2]).reshape(n, 9)
    T = np.zeros((n, 12))
    for b in range(n):   # this tick's update_plan: the counters above are the ones it leaves behind
        g, _, _, T[b], _ = oracle.update_plan(gp, 1, gc[b] - spd[b], spd[b], tick[b, 9:12], Rz[b], sc["R"][b], tick[b, 3:6], tick[b, 15:18])
        assert np.array_equal(g, gc[b])
    with _engine(pkg, sc, n, warm_start=0) as eng:
        pv = eng.preview_config(contact_schedule=1, foot_preview=2, ticks_per_step=tps)
        ref = eng.horizon_preview(mm, gc, spd, contacts, sc["foot"], sc["R"], tick[:, 15:18], preview=pv)
        new = eng.horizon_preview(mm, gc, spd, contacts, sc["foot"], sc["R"], tick[:, 15:18], preview=pv, foot_target_abs=T)
        assert np.array_equal(new["contact_sched"], ref["contact_sched"])
        a = eng.solve_ticks_strided(tick, sc["R"], new["foot_steps"], 12, ref["contact_sched"], 4, want_u=True)
        b_ = eng.solve_ticks_strided(tick, sc["R"], ref["foot_steps"], 12, ref["contact_sched"], 4, want_u=True)
    td = _touchdowns(ref["contact_sched"], n, h)
    lands = td.any(axis=(1, 2))
    first = np.where(lands, td.any(axis=2).argmax(axis=1), h)
    assert np.array_equal(lands, np.arange(n) % 2 == 0) and set(first[lands]) == set(range(1, h)) and np.array_equal(first[::2], step)
    assert (a["status"] == 1).all() and (b_["status"] == 1).all()
    for k in ("grf", "u", "iters", "status"):
        assert np.array_equal(a[k][~lands], b_[k][~lands]), k
    du = np.abs(a["u"] - b_["u"]).reshape(n, h, 12).max(axis=2)   # (n, h)
    for t in range(1, h):
        print(f"touchdown at step {t}: max |du| per horizon step " + " ".join(f"{v:.1e}" for v in du[first == t].max(axis=0)))
    from_td = np.arange(h)[None, :] >= first[:, None]
    assert ((du > 0) & from_td).any(axis=1)[lands].all()
    ua = a["u"].reshape(n, h, 4, 3)
    assert np.abs(ua[ref["contact_sched"].reshape(n, h, 4) == 0]).max() < 1.0   # swing steps carry no force, wherever their feet are


def _tick_world(pkg, n, dev, counters):
    """the device arrays of one handle's control ticks (state carried from tick to tick, outputs)"""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    init = dict(gait_counter=np.tile(counters, (n, 1)), root_pos=np.tile([0.0, 0.0, 0.3], (n, 1)))
    return dict(state={k: T(init.get(k, np.zeros((n, m)))) for k, m in TICK_STATE.items()},
                outs={k: torch.zeros((n, m) if m > 1 else (n,), dtype=torch.float64, device=dev) for k, m in TICK_OUT_F64.items()},
                u8={k: torch.zeros((n, 4), dtype=torch.uint8, device=dev) for k in ("estimated_contacts", "plan_contacts", "contacts")},
                i32={k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("iters", "status")})


def _tick_buffers(E, inp, w):
    bf = E.TickBuffers()
    for k in E.TICK_BUFFER_FIELDS:
        src = inp if k in inp else next(g for g in (w["state"], w["outs"], w["u8"], w["i32"]) if k in g)
        setattr(bf, k, src[k].data_ptr())
    return bf


def _assert_worlds_equal(t, w1, w2):
    for grp in ("state", "outs", "u8", "i32"):
        for k in w1[grp]:
            a, b = w1[grp][k].cpu().numpy(), w2[grp][k].cpu().numpy()
            assert np.array_equal(a, b, equal_nan=True), (t, k, np.abs(a.astype(float) - b.astype(float)).max())


# legs 1 / 2 are in swing and reach 240 inside the horizon on each of the six ticks (speed 2: 224 .. 234 after update_plan; the shortest horizon below spans 18 counts)
LANDING_COUNTERS = [102.0, 222.0, 222.0, 102.0]


@pytest.mark.parametrize("n,warm,h,feet,tps", [(300, 1, 10, 1, 2), (64, 2, 10, 2, 1), (64, 1, 16, 2, 1)])
def test_control_tick_footholds_one_call_matches_the_chain(pkg, scen, n, warm, h, feet, tps):
    """4. a1mpc_control_tick_preview_footholds_device on one handle against the *_device entries chained by hand on a second one, with
    a1mpc_horizon_preview_footholds_batch_device reading the chain's own foot_pos_target_abs: every output and every carried state bit for bit, six ticks; legs 1 / 2 land
    inside the horizon on every tick, and the chain's feet do hold the chain's targets there.  Per-step feet solve on the general kernels: torques_fused = 0."""
    import torch
    rng = np.random.default_rng(877 + n + h)
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h, warm_start=warm)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    E = pkg.engine
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e7:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        pv = e1.preview_config(contact_schedule=1, foot_preview=feet, ticks_per_step=tps)
        kp = np.array(prm.kp_foot); kd = np.array(prm.kd_foot); km = np.array(prm.km_foot); fix = np.array(prm.rho_fix); opt = np.array(prm.rho_opt)
        st = torch.cuda.Stream(device=dev); sp = C.c_void_p(st.cuda_stream)
        w1, w7 = _tick_world(pkg, n, dev, LANDING_COUNTERS), _tick_world(pkg, n, dev, LANDING_COUNTERS)
        sched_d = torch.zeros((n, 4 * h), dtype=torch.uint8, device=dev)
        feet_d = torch.zeros((n, 12 * h), dtype=torch.float64, device=dev)
        fused_seen = []
        for t in range(6):
            inp = {k: T(v) for k, v in tick_inputs(scen, rng, n).items()}
            # ---- one call
            e1.control_tick_preview_footholds_device(prm, pv, _tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
            fused_seen.append(e1.last_control_tick_ms()[1])
            assert e1.last_warm_start_mode() == warm
            # ---- the chain
            s7, o7, b7, j7, L, H_ = w7["state"], w7["outs"], w7["u8"], w7["i32"], e7.lib, e7._h
            rcs = [L.a1mpc_leg_state_batch_device(H_, n, ptr(inp["joint_pos"]), ptr(inp["joint_vel"]), ptr(inp["R_world"]), ptr(s7["root_pos"]), ptr(s7["root_lin_vel"]), dp_(fix),
                                                  dp_(opt), ptr(o7["foot_pos_rel"]), ptr(o7["j_foot_blocks"]), ptr(o7["foot_vel_rel"]), ptr(o7["foot_pos_abs"]),
                                                  ptr(o7["foot_vel_abs"]), ptr(o7["foot_pos_world"]), ptr(o7["foot_vel_world"]), sp),
                   L.a1mpc_ekf_update_batch_device(H_, n, prm.control_dt, 1, ptr(inp["movement_mode"]), ptr(inp["foot_force"]), ptr(inp["R_world"]), ptr(inp["imu_acc"]),
                                                   ptr(inp["imu_ang_vel"]), ptr(o7["foot_pos_rel"]), ptr(o7["foot_vel_rel"]), ptr(s7["root_pos"]), ptr(s7["root_lin_vel"]),
                                                   ptr(b7["estimated_contacts"]), sp),
                   L.a1mpc_update_plan_batch_device(H_, C.byref(prm.gait), n, ptr(inp["movement_mode"]), ptr(s7["gait_counter"]), ptr(inp["gait_counter_speed"]),
                                                    ptr(s7["root_lin_vel"]), ptr(inp["R_z"]), ptr(inp["R_world"]), ptr(s7["root_pos"]), ptr(inp["root_lin_vel_d"]),
                                                    ptr(b7["plan_contacts"]), ptr(o7["foot_pos_target_rel"]), ptr(o7["foot_pos_target_abs"]), ptr(o7["foot_pos_target_world"]), sp),
                   L.a1mpc_swing_legs_batch_device(H_, n, prm.gait.counter_per_swing, prm.control_dt, ptr(inp["R_z"]), ptr(o7["foot_pos_abs"]), ptr(s7["gait_counter"]),
                                                   ptr(o7["foot_pos_target_rel"]), dp_(kp), dp_(kd), ptr(s7["foot_pos_start"]), ptr(s7["foot_pos_rel_last_time"]),
                                                   ptr(s7["foot_pos_target_last_time"]), ptr(o7["foot_pos_cur"]), ptr(o7["foot_forces_kin"]), sp)]
            with torch.cuda.stream(st):
                pz = s7["root_pos"][:, 2].contiguous(); pitch = s7["root_euler_d"][:, 1].contiguous()
            rcs.append(L.a1mpc_contact_terrain_batch_device(H_, C.byref(prm.contact), n, ptr(s7["gait_counter"]), ptr(b7["plan_contacts"]), ptr(inp["foot_force"]),
                                                            ptr(o7["foot_pos_abs"]), ptr(pz), ptr(pitch), ptr(b7["contacts"]), ptr(o7["foot_pos_recent_contact"]),
                                                            ptr(o7["terrain_angle"]), sp))
            with torch.cuda.stream(st):
                s7["root_euler_d"][:, 1] = pitch
                tick = torch.cat([inp["root_euler"], s7["root_pos"], inp["root_ang_vel"], s7["root_lin_vel"], s7["root_euler_d"], inp["root_lin_vel_d"], inp["root_ang_vel_d"],
                                  inp["root_pos_d_z"].reshape(n, 1)], 1).contiguous()
            rcs.append(L.a1mpc_horizon_preview_footholds_batch_device(H_, C.byref(pv), C.byref(prm.gait), n, ptr(inp["movement_mode"]), ptr(s7["gait_counter"]),
                                                                      ptr(inp["gait_counter_speed"]), ptr(b7["contacts"]), ptr(o7["foot_pos_abs"]), ptr(inp["R_world"]),
                                                                      ptr(inp["root_lin_vel_d"]), ptr(o7["foot_pos_target_abs"]), ptr(sched_d), ptr(feet_d), sp))
            rcs.append(L.a1mpc_solve_batch_ticks_strided_device(H_, n, ptr(tick), ptr(inp["R_world"]), ptr(feet_d), 12, ptr(sched_d), 4, None, ptr(o7["grf"]), None, ptr(j7["iters"]),
                                                                ptr(j7["status"]), sp))
            rcs.append(L.a1mpc_joint_torques_batch_device(H_, n, ptr(inp["mpc_active"]), ptr(b7["contacts"]), ptr(o7["j_foot_blocks"]), ptr(o7["grf"]), ptr(o7["foot_forces_kin"]),
                                                          dp_(km), ptr(inp["torques_gravity"]), ptr(s7["joint_torques"]), sp))
            assert not any(rcs), (rcs, L.a1mpc_last_error())
            st.synchronize()
            assert e7.last_warm_start_mode() == warm
            _assert_worlds_equal(t, w1, w7)
            assert (w1["i32"]["status"].cpu().numpy() == 1).all() and np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1
            sd = sched_d.cpu().numpy()
            assert np.array_equal(sd.reshape(n, h, 4)[:, 0], w7["u8"]["contacts"].cpu().numpy())
            td = _touchdowns(sd, n, h)
            assert td[:, :, 1].any(axis=1).all() and td[:, :, 2].any(axis=1).all(), t   # legs 1 and 2 of every robot land inside the horizon
            fd = feet_d.cpu().numpy().reshape(n, h, 4, 3)
            tg = np.broadcast_to(o7["foot_pos_target_abs"].cpu().numpy().reshape(n, 1, 4, 3), (n, h, 4, 3))
            assert np.array_equal(_bits(fd[td]), _bits(tg[td]))
        assert fused_seen == [False] * 6, fused_seen


@pytest.mark.parametrize("n", [300, 4096])
def test_control_tick_footholds_switched_off_is_the_existing_tick(pkg, scen, n):
    """4b. With foot_preview = 0 the new control-tick entry is a1mpc_control_tick_preview_device: every output and carried state bit for bit over six ticks, the same
    torques_fused."""
    import torch
    rng = np.random.default_rng(199 + n)
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, 10, warm_start=1)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E = pkg.engine
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e2:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        pv = e1.preview_config(contact_schedule=1, foot_preview=0, ticks_per_step=1)
        st = torch.cuda.Stream(device=dev)
        w1, w2 = _tick_world(pkg, n, dev, LANDING_COUNTERS), _tick_world(pkg, n, dev, LANDING_COUNTERS)
        for t in range(6):
            inp = {k: T(v) for k, v in tick_inputs(scen, rng, n).items()}
            e1.control_tick_preview_footholds_device(prm, pv, _tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
            e2.control_tick_preview_device(prm, pv, _tick_buffers(E, inp, w2), n, stream=st.cuda_stream)
            st.synchronize()
            assert e1.last_control_tick_ms()[1] == e2.last_control_tick_ms()[1] and e1.last_warm_start_mode() == e2.last_warm_start_mode() == 1
            _assert_worlds_equal(t, w1, w2)
            assert (w1["i32"]["status"].cpu().numpy() == 1).all() and np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1


@pytest.mark.parametrize("h,n", [(10, 1536), (16, 96)])
def test_pipelined_tick_records_with_strides_are_the_lone_handle(pkg, scen, h, n):
    """5. Four distinct batches of foothold feet + schedule, round-robin through a depth-2 pipeline's submit_ticks_strided_device, against a lone handle's
    a1mpc_solve_batch_ticks_strided_device: array_equal grf, u, iters, status.  (0, 0, NULL) is submit_ticks_device."""
    import torch
    NB, tps = 4, 3
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(6200 + h)
    t_ = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    scs = [scen.config3_random_flat(nb=n, horizon=h, seed=1300 + 10 * h + k) for k in range(NB)]
    cfg = pkg.make_config(scs[0]["params"], h, warm_start=0)
    new_outs = lambda: (torch.zeros(n, 12, dtype=torch.float64, device=dev), torch.zeros(n, 12 * h, dtype=torch.float64, device=dev),
                        torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    ins, ref = [], []
    with pkg.Engine(cfg, n, 0) as eng:
        pv = eng.preview_config(contact_schedule=1, foot_preview=2, ticks_per_step=tps)
        for sc in scs:
            mm, gc, spd, contacts = _gait_inputs(rng, n, h, tps)
            T = np.tile(DEFAULT_FOOT_POS, (n, 1)) + rng.normal(0, 0.05, (n, 12))
            p = eng.horizon_preview(mm, gc, spd, contacts, sc["foot"], sc["R"], sc["tick"][:, 15:18], preview=pv, foot_target_abs=T)
            assert _touchdowns(p["contact_sched"], n, h).any(axis=(1, 2)).mean() > 0.3
            ins.append([t_(sc["tick"]), t_(sc["R"]), t_(p["foot_steps"]), t_(p["contact_sched"], torch.uint8)])
        for tk, R, ft, ct in ins:
            o = new_outs()
            eng.set_schedule(True)
            rc = eng.lib.a1mpc_solve_batch_ticks_strided_device(eng._h, n, ptr(tk), ptr(R), ptr(ft), 12, ptr(ct), 4, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None)
            assert rc == 0, eng.lib.a1mpc_last_error()
            torch.cuda.synchronize()
            ref.append([x.cpu().numpy() for x in o])
            assert (ref[-1][3] == 1).all()
    with pkg.Pipeline(cfg, n, 0, depth=2) as pipe:
        outs = [new_outs() for _ in range(NB)]
        slots = [pipe.submit_ticks_strided_device(n, tk, R, ft, 12, ct, 4, o[0], o[1], o[2], o[3]) for (tk, R, ft, ct), o in zip(ins, outs)]
        assert slots == [0, 1, 0, 1]
        pipe.wait()
        for k in range(NB):
            for got, exp, name in zip(outs[k], ref[k], ("grf", "u", "iters", "status")):
                assert np.array_equal(got.cpu().numpy(), exp), (k, name)
        # (0, 0, NULL) is the tick-record submit
        sc = scs[0]; tk, R = ins[0][:2]; ft, ct = t_(sc["foot"]), t_(sc["contact"], torch.uint8)
        a, b = new_outs(), new_outs()
        pipe.submit_ticks_device(n, tk, R, ft, ct, a[0], a[1], a[2], a[3]); pipe.wait()
        pipe.submit_ticks_strided_device(n, tk, R, ft, 0, ct, 0, b[0], b[1], b[2], b[3]); pipe.wait()
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert (a[3].cpu().numpy() == 1).all()


def test_refusals_leave_the_handle_usable(pkg, oracle, scen):
    """6. A null target with foot_steps_out, a null schedule input with contact_schedule 1 and only feet asked for, a null buffers->foot_pos_target_abs in the control tick
    with foot_preview != 0 and foot_stride 7 in the pipeline submit are A1MPC_ERR_INVALID_ARGUMENT with a message naming the argument; foot_preview 3 stays refused by the
    new entries; the handle solves correctly afterwards."""
    import torch
    n, h = 8, 10
    sc = scen.config3_random_flat(nb=n)
    E = pkg.engine
    mm = np.ones(n, np.uint8); gc = np.zeros((n, 4)); spd = np.ones((n, 4)); ct = np.ones((n, 4), np.uint8)
    foot = np.ascontiguousarray(sc["foot"]); R = np.ascontiguousarray(sc["R"]); vd = np.ascontiguousarray(sc["tick"][:, 15:18]); T = foot + 0.01
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8)); dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    with _engine(pkg, sc, n, warm_start=0) as eng:
        L = eng.lib
        gait = E.GaitConfig(); L.a1mpc_default_gait_config(C.byref(gait))
        sched = np.zeros((n, 4 * h), np.uint8); feet = np.zeros((n, 12 * h))
        ok = E.PreviewConfig(1, 2, 1)

        def call(pv=ok, mm_=mm, gc_=gc, spd_=spd, ct_=ct, T_=T, sched_=None, feet_=feet):
            return L.a1mpc_horizon_preview_footholds_batch(eng._h, C.byref(pv), C.byref(gait), n, u8(mm_), dp(gc_), dp(spd_), u8(ct_), dp(foot), dp(R), dp(vd), dp(T_), u8(sched_),
                                                           dp(feet_))
        assert call(T_=None) == 1 and b"foot_pos_target_abs" in L.a1mpc_last_error(), L.a1mpc_last_error()
        for kw, word in ((dict(mm_=None), b"movement_mode"), (dict(gc_=None), b"gait_counter"), (dict(spd_=None), b"gait_counter_speed"), (dict(ct_=None), b"contacts")):
            assert call(**kw) == 1 and word in L.a1mpc_last_error(), (kw, L.a1mpc_last_error())   # only feet asked for: the footholds read the schedule
        assert call(pv=E.PreviewConfig(1, 3, 1)) == 1 and b"foot_preview" in L.a1mpc_last_error()
        dz = torch.zeros(n * 12 * h, dtype=torch.float64, device="cuda:0"); dpz = C.c_void_p(dz.data_ptr())
        dev_call = lambda pv, tg, mmp: L.a1mpc_horizon_preview_footholds_batch_device(eng._h, C.byref(pv), C.byref(gait), n, mmp, dpz, dpz, dpz, dpz, dpz, dpz, tg, None, dpz, None)
        assert dev_call(ok, None, dpz) == 1 and b"foot_pos_target_abs" in L.a1mpc_last_error()
        assert dev_call(ok, dpz, None) == 1 and b"movement_mode" in L.a1mpc_last_error()
        assert dev_call(E.PreviewConfig(1, 3, 1), dpz, dpz) == 1 and b"foot_preview" in L.a1mpc_last_error()
        # the control tick: every mandatory buffer present, the target missing
        prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm)); bf = E.TickBuffers()
        for k in E.TICK_BUFFER_FIELDS:
            setattr(bf, k, dz.data_ptr())
        bf.foot_pos_target_abs = None
        assert L.a1mpc_control_tick_preview_footholds_device(eng._h, C.byref(prm), C.byref(ok), C.byref(bf), n, None) == 1 and b"foot_pos_target_abs" in L.a1mpc_last_error()
        assert L.a1mpc_control_tick_preview_footholds_device(eng._h, C.byref(prm), C.byref(E.PreviewConfig(1, 3, 1)), C.byref(bf), n, None) == 1
        assert b"foot_preview" in L.a1mpc_last_error()
        with pkg.Pipeline(eng.cfg, n, 0, depth=2) as pipe:
            with pytest.raises(pkg.A1MpcError, match="foot_stride"):
                pipe.submit_ticks_strided_device(n, dz, dz, dz, 7, dz, 4, dz)
        # ... and the handle works: no touchdown in this schedule (all feet down, counters at 0), so the feet are today's and the solve is the oracle's
        assert call(sched_=sched) == 0 and (sched == 1).all()
        ref = eng.horizon_preview(mm, gc, spd, ct, foot, R, vd, preview=ok)
        assert np.array_equal(feet, ref["foot_steps"])
        out = eng.solve_ticks_strided(sc["tick"], sc["R"], feet, 12, sched, 4, want_u=True)
    pr = oracle.mpc_params(h, **{k: sc["params"][k] for k in ("dt", "mu", "fz_min", "fz_max", "q", "r", "mass", "inertia")}); st = oracle.default_settings()
    for b in range(n):
        r = oracle.mpc_solve(pr, st, sc["x0"][b], sc["xref"][b], sc["R"][b], feet[b], sched[b], foot_stride=12, contact_stride=4)
        assert out["iters"][b] == r["info"].iters and out["status"][b] == r["info"].status
        assert max(np.abs(out["u"][b] - r["u"]).max(), np.abs(out["grf"][b] - r["grf"]).max()) <= TOL_FORCE_N
