"""GPU, through the C ABI: the gait-aware horizon -- a1mpc_horizon_preview_batch(_device) (contact schedule = update_plan's counter rule run forward, S/A1RobotControl.cpp:156-164;
per-step feet = the recurrence of S/test/test_mpc.cpp:112-115), a1mpc_solve_batch_ticks_strided(_device) (tick records joined with the strides of the general interface) and
a1mpc_control_tick_preview_device (the control tick that uses both).  The yardsticks are the oracle and the entries that existed before, never the new code itself."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import TICK_OUT_F64, TICK_STATE, _engine, tick_inputs
from helpers import TOL_FORCE_N

pytestmark = pytest.mark.gpu

DEFAULT_FOOT_POS = [0.17, 0.15, -0.35, 0.17, -0.15, -0.35, -0.17, 0.15, -0.35, -0.17, -0.15, -0.35]
PER_GAIT, PER_SWING = 240.0, 120.0   # counter_per_gait / counter_per_swing, S/A1CtrlStates.h:24-25


def _gait_inputs(rng, n, h, tps):
    """the inputs of test_update_plan_N2a_bit_exact (counters uniform in [0, 240) with the reset pattern and a 239.0 wrap case, per-leg speeds from {1, 1.5, 2, 3}, 80 % of the
    robots walking); in addition every third robot has leg 0 within (h - 1) * tps * speed counts before 120 or 240, i.e. a switch of that leg inside the horizon"""
    mm = (rng.random(n) < 0.8).astype(np.uint8)
    gc = rng.uniform(0, PER_GAIT, (n, 4)); gc[::7] = [0, 120, 120, 0]; gc[::11, 0] = 239.0
    spd = rng.choice([1.0, 1.5, 2.0, 3.0], size=(n, 4))
    k = np.arange(0, n, 3)
    edge = rng.choice([PER_SWING, PER_GAIT], size=len(k))
    gc[k, 0] = np.mod(edge - rng.uniform(0, 1, len(k)) * (h - 1) * tps * spd[k, 0], PER_GAIT)
    return mm, gc, spd


def _oracle_plan_forward(oracle, mm, gc, spd, h, tps, gp=None):
    """plan_contacts of the next (h - 1) * tps calls of the oracle's update_plan (orc_update_plan, the restatement oracle/_ref pins to the reference's sources) at constant
    speed, every tps-th one kept: (n, h - 1, 4).  One C call per robot and tick, on the robot's own words of the arrays below (the Python wrapper oracle.update_plan
    makes the same call; it allocates nine arrays per call, which 4.6 M calls cannot afford).  gp: oracle.gait_params of another gait (default: the reference's)."""
    n = len(mm)
    gp = oracle.gait_params(DEFAULT_FOOT_POS) if gp is None else gp
    fn = oracle.lib().orc_update_plan
    g = np.array(gc, dtype=np.float64); s = np.ascontiguousarray(spd, dtype=np.float64)
    z3 = np.zeros(3); eye = np.eye(3).reshape(9).copy(); pc = np.zeros(4, np.uint8); rel = np.zeros(12); ab = np.zeros(12); wo = np.zeros(12)
    vp = C.c_void_p
    fixed = [vp(a.ctypes.data) for a in (z3, eye, eye, z3, z3)]
    outs = [vp(a.ctypes.data) for a in (pc, rel, ab, wo)]
    gpr = C.byref(gp)
    plan = np.zeros((n, h - 1, 4), np.uint8)
    for b in range(n):
        gb, sb, mode = vp(g.ctypes.data + 32 * b), vp(s.ctypes.data + 32 * b), C.c_int(int(mm[b]))
        for t in range(1, h):
            for _ in range(tps):
                fn(gpr, mode, gb, sb, *fixed, *outs)
            plan[b, t - 1] = pc
    return plan


@pytest.mark.parametrize("tps", [1, 3, 16])
@pytest.mark.parametrize("h", [4, 10, 16, 20])
@pytest.mark.parametrize("n", [5000, 1, 67])
def test_schedule_is_update_plan_run_forward(pkg, oracle, scen, n, h, tps):
    """1. Step 0 is the contacts input; step t >= 1 is, byte for byte, the plan_contacts that the oracle's update_plan produces t * ticks_per_step ticks later when it is
    called again and again on the same counters (iterated fmod, not a closed form).  Every byte of every robot.  The ORACLE's schedule must show a switch inside the
    horizon on >= 40 % of the walking robots, or a constant schedule would pass."""
    rng = np.random.default_rng(31 + 1000 * h + tps)
    mm, gc, spd = _gait_inputs(rng, n, h, tps)
    plan_now = (gc <= PER_SWING).astype(np.uint8)
    contacts = np.where(mm[:, None] == 1, plan_now | (rng.random((n, 4)) < 0.1), 1).astype(np.uint8)   # planned or early contact (S/A1RobotControl.cpp:271); standing: all feet down
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h)
    with pkg.Engine(cfg, n, 0) as eng:
        out = eng.horizon_preview(mm, gc, spd, contacts, preview=eng.preview_config(ticks_per_step=tps))
    assert out["foot_steps"] is None
    plan = _oracle_plan_forward(oracle, mm, gc, spd, h, tps)
    expect = np.concatenate([contacts[:, None, :], plan], axis=1)
    walking = mm == 1
    if n >= 67:
        seq = np.concatenate([plan_now[:, None, :], plan], axis=1)[walking]
        switched = (seq != seq[:, :1]).any(axis=(1, 2)).mean()
        print(f"n {n} h {h} tps {tps}: {switched:.3f} of the walking robots switch inside the horizon")
        assert switched >= 0.4, switched
    assert (plan[~walking] == 1).all()
    got = out["contact_sched"].reshape(n, h, 4)
    assert got.dtype == np.uint8 and np.array_equal(got, expect), np.argwhere(got != expect)[:5]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,h", [(5000, 10), (67, 20), (1, 4)])
def test_feet_are_the_reference_loop(pkg, scen, n, h, mode):
    """2. foot_preview 1 / 2 against the plain float64 loop f = f - vd * dt (S/test/test_mpc.cpp:112-115; mode 2: vd rotated by R_world as at S/A1RobotControl.cpp:470, summed left
    to right), one rounded product and one subtraction per step: all n x 12 h values bit for bit.  A fifth of the commands are large enough that consecutive steps differ in
    many bits."""
    rng = np.random.default_rng(5 + h + mode)
    P = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
    cfg = pkg.make_config(P, h)
    foot = np.tile(DEFAULT_FOOT_POS, (n, 1)) + rng.normal(0, 0.05, (n, 12))
    vd = rng.normal(0, 0.6, (n, 3)); vd[::5] *= 1000.0; vd[::7, 2] = 0.0
    eul = rng.normal(0, 0.2, (n, 3)); eul[:, 2] = rng.uniform(-3, 3, n)
    R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)
    contacts = np.ones((n, 4), np.uint8); mm = np.ones(n, np.uint8); gc = np.zeros((n, 4)); spd = np.ones((n, 4))
    with pkg.Engine(cfg, n, 0) as eng:
        out = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=eng.preview_config(contact_schedule=0, foot_preview=mode), want_schedule=False)
        both = eng.horizon_preview(mm, gc, spd, contacts, foot, R, vd, preview=eng.preview_config(contact_schedule=0, foot_preview=mode))
    assert out["contact_sched"] is None and np.array_equal(both["foot_steps"], out["foot_steps"])
    assert np.array_equal(both["contact_sched"], np.tile(contacts, (1, h)))   # contact_schedule 0: the reference's broadcast, written out
    v = vd if mode == 1 else np.stack([R[:, 3 * r] * vd[:, 0] + R[:, 3 * r + 1] * vd[:, 1] + R[:, 3 * r + 2] * vd[:, 2] for r in range(3)], axis=1)
    dt = float(cfg.dt)
    f = foot.reshape(n, 4, 3).copy(); expect = np.zeros((n, h, 4, 3))
    for t in range(h):
        expect[:, t] = f
        f = f - (v * dt)[:, None, :]
    got = out["foot_steps"].reshape(n, h, 4, 3)
    assert np.array_equal(got, expect), np.abs(got - expect).max()
    assert (np.abs(got[:, 1] - got[:, 0]).max(axis=(1, 2)) > 1e-3).mean() > 0.15   # the large commands are there


def _preview_of_scenario(eng, rng, sc, feet, sched, tps=4):
    """feet / schedule for the QPs of a random-flat scenario, from the preview entry itself: step 0 = the scenario's contacts and feet, the command = the tick record's"""
    n = len(sc["x0"]); h = sc["horizon"]
    mm, gc, spd = _gait_inputs(rng, n, h, tps)
    pv = eng.preview_config(contact_schedule=1 if sched else 0, foot_preview=feet, ticks_per_step=tps)
    out = eng.horizon_preview(mm, gc, spd, sc["contact"], sc["foot"], sc["R"], sc["tick"][:, 15:18], preview=pv, want_schedule=bool(sched))
    foot, fs = (out["foot_steps"], 12) if feet else (sc["foot"], 0)
    contact, cs = (out["contact_sched"], 4) if sched else (sc["contact"], 0)
    return np.ascontiguousarray(foot), fs, np.ascontiguousarray(contact), cs


@pytest.mark.parametrize("feet,sched", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("h,n", [(10, 300), (16, 96), (20, 64), (6, 5), (10, 4000)])
def test_tick_records_with_strides_vs_the_oracle(pkg, oracle, scen, h, n, feet, sched):
    """3. a1mpc_solve_batch_ticks_strided on the tick records with the preview entry's own outputs as per-step inputs, against the oracle's strided formation on the x0 / x_ref
    the reference would build (every third QP, like test_per_step_feet_and_contact_schedules): same iteration count and status on every sampled QP (MIN_SAME_ITERS = 1.0),
    forces within TOL_FORCE_N; and against a1mpc_solve_batch_strided on the explicit x0 / x_ref: same iterations, forces within TOL_FORCE_N (the bar test_tick_records_N1 sets
    for the unstrided pair).  (0, 0, NULL) is a1mpc_solve_batch_ticks, bit for bit."""
    rng = np.random.default_rng(4000 + h + 2 * feet + sched)
    sc = scen.config3_random_flat(nb=n, horizon=h)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        foot, fs, contact, cs = _preview_of_scenario(eng, rng, sc, feet, sched)
        out = eng.solve_ticks_strided(sc["tick"], sc["R"], foot, fs, contact, cs, want_u=True)
        exp = eng.solve_strided(sc["x0"], sc["xref"], sc["R"], foot, fs, contact, cs, want_u=True)
        plain = eng.solve_ticks_strided(sc["tick"], sc["R"], sc["foot"], 0, sc["contact"], 0, want_u=True)
        ticks = eng.solve_ticks(sc["tick"], sc["R"], sc["foot"], sc["contact"], want_u=True)
    for k in ("grf", "u", "iters", "status"):
        assert np.array_equal(plain[k], ticks[k]), k
    if sched and n >= 64:
        assert (contact.reshape(n, h, 4)[:, 1:] != contact.reshape(n, h, 4)[:, 1:2]).any(axis=(1, 2)).mean() > 0.3   # the schedules do change inside the horizon
    assert np.array_equal(out["iters"], exp["iters"]) and np.array_equal(out["status"], exp["status"])
    d_exp = max(np.abs(out["u"] - exp["u"]).max(), np.abs(out["grf"] - exp["grf"]).max())
    pr = oracle.mpc_params(h, **{k: sc["params"][k] for k in ("dt", "mu", "fz_min", "fz_max", "q", "r", "mass", "inertia")}); st = oracle.default_settings()
    worst = 0.0
    for b in range(0, n, 3):
        r = oracle.mpc_solve(pr, st, sc["x0"][b], sc["xref"][b], sc["R"][b], foot[b], contact[b], foot_stride=fs, contact_stride=cs)
        assert out["iters"][b] == r["info"].iters and out["status"][b] == r["info"].status, (b, out["iters"][b], r["info"].iters)
        worst = max(worst, np.abs(out["u"][b] - r["u"]).max(), np.abs(out["grf"][b] - r["grf"]).max())
    print(f"h{h} x {n} feet {feet} sched {sched}: |du| vs the oracle {worst:.2e} N, vs solve_strided on x0 / x_ref {d_exp:.2e} N")
    assert worst <= TOL_FORCE_N and d_exp <= TOL_FORCE_N, (worst, d_exp)


def _tick_world(pkg, n, dev):
    """the device arrays of one handle's control ticks (state carried from tick to tick, outputs)"""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    init = dict(gait_counter=np.tile([108.0, 228.0, 228.0, 108.0], (n, 1)), root_pos=np.tile([0.0, 0.0, 0.3], (n, 1)))   # six counts (three ticks at speed 2) before the switch
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


@pytest.mark.parametrize("n,warm,h,sched,feet,tps", [(300, 1, 10, 1, 0, 1), (64, 2, 10, 1, 0, 3), (4096, 1, 10, 1, 0, 1), (300, 2, 10, 1, 1, 2), (64, 1, 16, 0, 2, 1)])
def test_control_tick_preview_one_call_matches_the_chain(pkg, scen, n, warm, h, sched, feet, tps):
    """4. a1mpc_control_tick_preview_device on one handle against the *_device entries chained by hand on a second one, with a1mpc_horizon_preview_batch_device +
    a1mpc_solve_batch_ticks_strided_device + a1mpc_joint_torques_batch_device in the place of the ticks solve: every output and every carried state bit for bit, six ticks.
    The gait counters start three ticks before a switch, so the schedule changes while the ticks run.  A schedule alone keeps N3 in the MPC kernel's output stage wherever
    the plain tick has it (torques_fused as a1mpc_control_tick_device reports it); per-step feet solve on the general kernels: torques_fused = 0."""
    import torch
    rng = np.random.default_rng(777 + n + h)
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h, warm_start=warm)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    E = pkg.engine
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e7:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        pv = e1.preview_config(contact_schedule=sched, foot_preview=feet, ticks_per_step=tps)
        kp = np.array(prm.kp_foot); kd = np.array(prm.kd_foot); km = np.array(prm.km_foot); fix = np.array(prm.rho_fix); opt = np.array(prm.rho_opt)
        st = torch.cuda.Stream(device=dev); sp = C.c_void_p(st.cuda_stream)
        w1, w7 = _tick_world(pkg, n, dev), _tick_world(pkg, n, dev)
        sched_d = torch.zeros((n, 4 * h), dtype=torch.uint8, device=dev) if sched else None
        feet_d = torch.zeros((n, 12 * h), dtype=torch.float64, device=dev) if feet else None
        fused_seen, sched_seen = [], []
        for t in range(6):
            inp = {k: T(v) for k, v in tick_inputs(scen, rng, n).items()}
            # ---- one call
            e1.control_tick_preview_device(prm, pv, _tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
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
            rcs.append(L.a1mpc_horizon_preview_batch_device(H_, C.byref(pv), C.byref(prm.gait), n, ptr(inp["movement_mode"]), ptr(s7["gait_counter"]), ptr(inp["gait_counter_speed"]),
                                                            ptr(b7["contacts"]), ptr(o7["foot_pos_abs"]), ptr(inp["R_world"]), ptr(inp["root_lin_vel_d"]), ptr(sched_d), ptr(feet_d), sp))
            rcs.append(L.a1mpc_solve_batch_ticks_strided_device(H_, n, ptr(tick), ptr(inp["R_world"]), ptr(feet_d if feet else o7["foot_pos_abs"]), 12 if feet else 0,
                                                                ptr(sched_d if sched else b7["contacts"]), 4 if sched else 0, None, ptr(o7["grf"]), None, ptr(j7["iters"]),
                                                                ptr(j7["status"]), sp))
            rcs.append(L.a1mpc_joint_torques_batch_device(H_, n, ptr(inp["mpc_active"]), ptr(b7["contacts"]), ptr(o7["j_foot_blocks"]), ptr(o7["grf"]), ptr(o7["foot_forces_kin"]),
                                                          dp_(km), ptr(inp["torques_gravity"]), ptr(s7["joint_torques"]), sp))
            assert not any(rcs), (rcs, L.a1mpc_last_error())
            st.synchronize()
            assert e7.last_warm_start_mode() == warm
            _assert_worlds_equal(t, w1, w7)
            assert (w1["i32"]["status"].cpu().numpy() == 1).all() and np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1
            if sched:
                sd = sched_d.cpu().numpy().reshape(n, h, 4)
                assert np.array_equal(sd[:, 0], w7["u8"]["contacts"].cpu().numpy())
                sched_seen.append(sd[0].copy())
        if feet:
            assert fused_seen == [False] * 6, fused_seen
        else:
            assert fused_seen == ([True] * 6 if n <= 2048 else [False] + [True] * 5), fused_seen
        if sched:   # the schedule saw the switch coming, and it changed from tick to tick
            assert any((s != s[:1]).any() for s in sched_seen) and any(not np.array_equal(sched_seen[0], s) for s in sched_seen[1:])


@pytest.mark.parametrize("n,warm", [(300, 1), (4096, 2)])
def test_control_tick_preview_switched_off_is_the_control_tick(pkg, scen, n, warm):
    """4 (last case). preview {0, 0, 1} against a1mpc_control_tick_device itself: every output and carried state bit for bit over six ticks, the same torques_fused."""
    import torch
    rng = np.random.default_rng(99 + n)
    cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, 10, warm_start=warm)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E = pkg.engine
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e2:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        off = e1.preview_config(contact_schedule=0, foot_preview=0, ticks_per_step=1)
        st = torch.cuda.Stream(device=dev)
        w1, w2 = _tick_world(pkg, n, dev), _tick_world(pkg, n, dev)
        for t in range(6):
            inp = {k: T(v) for k, v in tick_inputs(scen, rng, n).items()}
            e1.control_tick_preview_device(prm, off, _tick_buffers(E, inp, w1), n, stream=st.cuda_stream)
            e2.control_tick_device(prm, _tick_buffers(E, inp, w2), n, stream=st.cuda_stream)
            st.synchronize()
            assert e1.last_control_tick_ms()[1] == e2.last_control_tick_ms()[1] and e1.last_warm_start_mode() == e2.last_warm_start_mode() == warm
            _assert_worlds_equal(t, w1, w2)
            assert (w1["i32"]["status"].cpu().numpy() == 1).all() and np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1


def test_the_schedule_matters_and_is_physical(pkg, scen):
    """5. One batch in which legs 1 and 2 of every other robot lift inside the horizon (all four feet down now).  The scheduled solve puts |f| < 1 N on every (step, leg) the
    schedule marks as swing (the check of test_per_step_feet_and_contact_schedules), and its step-0 GRFs differ from the broadcast solve's on exactly those robots."""
    n, h, tps = 256, 10, 4
    sc = scen.config3_random_flat(nb=n, horizon=h)
    mm = np.ones(n, np.uint8); spd = np.full((n, 4), 2.0)
    gc = np.tile([0.0, 40.0, 40.0, 0.0], (n, 1))   # nobody lifts within 9 * 4 * 2 = 72 counts ...
    gc[::2, 1:3] = 120.0 - 2.0 * tps * np.arange(1, 1 + n // 2)[:, None] % 72   # ... but legs 1 and 2 of every other robot do, at each of the steps 1 .. 9
    contacts = np.ones((n, 4), np.uint8)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        pv = eng.horizon_preview(mm, gc, spd, contacts, preview=eng.preview_config(ticks_per_step=tps))
        sched = pv["contact_sched"]
        out = eng.solve_ticks_strided(sc["tick"], sc["R"], sc["foot"], 0, sched, 4, want_u=True)
        bc = eng.solve_ticks(sc["tick"], sc["R"], sc["foot"], contacts, want_u=True)
    c = sched.reshape(n, h, 4)
    lifts = (c == 0).any(axis=(1, 2))
    assert np.array_equal(lifts, np.arange(n) % 2 == 0) and (c[:, 0] == 1).all() and (out["status"] == 1).all() and (bc["status"] == 1).all()
    u = out["u"].reshape(n, h, 4, 3)
    assert np.abs(u[c == 0]).max() < 1.0
    assert np.abs(u[:, 0][c[:, 0] == 1]).max() > 10.0   # ... and the stance legs carry the robot
    d = np.abs(out["grf"] - bc["grf"]).max(axis=1)
    first = np.where(lifts, (c == 0).any(axis=2).argmax(axis=1), h)   # the first step with a leg in the air
    for t in range(1, h):
        if (first == t).any():
            print(f"first lift at step {t}: step-0 GRF scheduled vs broadcast min {d[first == t].min():.3e} N, median {np.median(d[first == t]):.3e} N")
    # Every robot with a lift gets other forces NOW (the issue's "differ"); the robots without one get the broadcast solve's, to the parity bar.  How much a lift at step t
    # moves step 0 decays with t (a lift at the last steps changes the iterates by less than OSQP's stopping tolerance resolves: 6e-8 N has been observed for a lift at step 7), so an amount is
    # asked only where the lift is imminent, steps 1-2, and there it is the solver's own resolution, eps_abs = 1e-3.
    assert set(first[lifts]) == set(range(1, h)) and (d[lifts] > 0).all() and (d[first <= 2] > 1e-3).all()
    assert d[~lifts].max() <= TOL_FORCE_N and np.array_equal(out["iters"][~lifts], bc["iters"][~lifts])


def test_refusals_leave_the_handle_usable(pkg, oracle, scen):
    """6. ticks_per_step 0 and 65, foot_preview 3, a null config, counter_per_gait <= 0 and horizon 1 are A1MPC_ERR_INVALID_ARGUMENT with a message naming the field, on every
    entry that takes the config; the handle solves correctly afterwards."""
    import torch
    n = 8
    sc = scen.config3_random_flat(nb=n)
    E = pkg.engine
    mm = np.ones(n, np.uint8); gc = np.zeros((n, 4)); spd = np.ones((n, 4)); ct = np.ones((n, 4), np.uint8)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        L = eng.lib
        gait = E.GaitConfig(); L.a1mpc_default_gait_config(C.byref(gait))
        sched = np.zeros((n, 40), np.uint8)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)); dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        call = lambda pv, g=gait: L.a1mpc_horizon_preview_batch(eng._h, pv, C.byref(g), n, u8(mm), dp(gc), dp(spd), u8(ct), None, None, None, u8(sched), None)
        for fields, word in ((dict(ticks_per_step=0), b"ticks_per_step"), (dict(ticks_per_step=65), b"ticks_per_step"), (dict(foot_preview=3), b"foot_preview"),
                             (dict(foot_preview=-1), b"foot_preview")):
            pv = E.PreviewConfig(1, 0, 1)
            for k, v in fields.items():
                setattr(pv, k, v)
            assert call(C.byref(pv)) == 1 and word in L.a1mpc_last_error(), (fields, L.a1mpc_last_error())
            prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm)); bf = E.TickBuffers()
            assert L.a1mpc_control_tick_preview_device(eng._h, C.byref(prm), C.byref(pv), C.byref(bf), n, None) == 1 and word in L.a1mpc_last_error()
            dz = torch.zeros(64, dtype=torch.uint8, device="cuda:0"); dpz = C.c_void_p(dz.data_ptr())
            assert L.a1mpc_horizon_preview_batch_device(eng._h, C.byref(pv), C.byref(gait), n, dpz, dpz, dpz, dpz, None, None, None, dpz, None, None) == 1
        assert call(None) == 1 and b"a1mpc_preview_config" in L.a1mpc_last_error()
        ok = E.PreviewConfig(1, 0, 1)
        bad_gait = E.GaitConfig(); L.a1mpc_default_gait_config(C.byref(bad_gait)); bad_gait.counter_per_gait = 0.0
        assert call(C.byref(ok), bad_gait) == 1 and b"counter_per_gait" in L.a1mpc_last_error()
        assert L.a1mpc_solve_batch_ticks_strided(eng._h, n, dp(sc["tick"]), dp(sc["R"]), dp(sc["foot"]), 7, u8(sc["contact"]), 0, None, dp(np.zeros((n, 12))), None, None, None) == 1
        assert call(C.byref(ok)) == 0 and (sched == 1).all()
        out = eng.solve_ticks_strided(sc["tick"], sc["R"], sc["foot"], 0, sched, 4)
    ref = oracle.mpc_solve_batch(oracle.mpc_params(10, **{k: sc["params"][k] for k in ("dt", "mu", "fz_min", "fz_max", "q", "r", "mass", "inertia")}), oracle.default_settings(),
                                 sc["x0"], sc["xref"], sc["R"], sc["foot"], np.ones((n, 4), np.uint8))
    assert np.array_equal(out["iters"], ref["iters"]) and np.array_equal(out["status"], ref["status"]) and np.abs(out["grf"] - ref["grf"]).max() <= TOL_FORCE_N
    with pkg.Engine(pkg.make_config(sc["params"], 1), n, 0) as e1:   # horizon 1 (the balance-QP analogue) has no horizon to preview
        pv = E.PreviewConfig(1, 0, 1)
        assert e1.lib.a1mpc_horizon_preview_batch(e1._h, C.byref(pv), C.byref(gait), n, u8(mm), dp(gc), dp(spd), u8(ct), None, None, None, u8(sched), None) == 1
        assert b"horizon" in e1.lib.a1mpc_last_error()
