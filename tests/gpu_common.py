"""Shared helpers of the GPU suite (engine factory, strided inputs of the general path, control-tick inputs): imported by the tests/test_gpu_*.py files."""
import numpy as np


def _engine(pkg, sc, max_batch, **osqp):
    cfg = pkg.make_config(sc["params"], sc["horizon"], **osqp)
    return pkg.Engine(cfg, max_batch=max_batch, device=0)


SETTINGS_CASES = [dict(scaling=0), dict(scaling=3), dict(alpha=1.0), dict(alpha=1.8), dict(rho=1.0), dict(rho=0.01, adaptive_rho=0),
                  dict(check_termination=10), dict(adaptive_rho_interval=50), dict(check_termination=10, adaptive_rho_interval=35),
                  dict(max_iter=30), dict(sigma=1e-4), dict(adaptive_rho_interval=0), dict(adaptive_rho_interval=0, check_termination=10),
                          dict(eps_abs=1e-5, eps_rel=1e-5), dict(adaptive_rho_tolerance=2.0)]


def tick_inputs(scen, rng, n):
    """random sensors / commands of one control tick (what test_device_pointer_tick_matches_host_pointer_tick feeds the chain)"""
    eul = rng.normal(0, 0.05, (n, 3)); eul[:, 2] = rng.uniform(-1, 1, n)
    return dict(joint_pos=np.tile([0.0, 0.8, -1.6], (n, 4)) + rng.normal(0, 0.1, (n, 12)), joint_vel=rng.normal(0, 1, (n, 12)),
                R_world=scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9), R_z=scen.rot_zyx(0 * eul[:, 0], 0 * eul[:, 0], eul[:, 2]).reshape(n, 9),
                root_euler=eul, root_ang_vel=rng.normal(0, 0.2, (n, 3)), imu_acc=np.array([0, 0, 9.81]) + rng.normal(0, 0.2, (n, 3)),
                imu_ang_vel=rng.normal(0, 0.2, (n, 3)), foot_force=rng.uniform(0, 120, (n, 4)), movement_mode=np.ones(n, np.uint8),
                mpc_active=(rng.random(n) < 0.9).astype(np.uint8), root_lin_vel_d=np.c_[rng.uniform(-0.4, 0.4, (n, 2)), np.zeros(n)],
                root_ang_vel_d=np.c_[np.zeros((n, 2)), rng.uniform(-0.4, 0.4, n)], root_pos_d_z=np.full(n, 0.3), gait_counter_speed=np.full((n, 4), 2.0),
                torques_gravity=rng.normal(0, 0.5, (n, 12)))


TICK_STATE = dict(gait_counter=4, foot_pos_start=12, foot_pos_rel_last_time=12, foot_pos_target_last_time=12, root_euler_d=3, joint_torques=12, root_pos=3,
                  root_lin_vel=3)
TICK_OUT_F64 = dict(foot_pos_rel=12, j_foot_blocks=36, foot_vel_rel=12, foot_pos_abs=12, foot_vel_abs=12, foot_pos_world=12, foot_vel_world=12, foot_pos_target_rel=12,
                    foot_pos_target_abs=12, foot_pos_target_world=12, foot_pos_cur=12, foot_forces_kin=12, foot_pos_recent_contact=12, terrain_angle=1, grf=12)


def _strided_inputs(scen, rng, h, nb, feet, cont):
    sc = scen.config3_random_flat(nb=nb, horizon=h)
    p = sc["params"]; foot = sc["foot"]; contact = sc["contact"]; fs = cs = 0
    if feet:
        vd = rng.uniform(-0.6, 0.6, (nb, 1, 1, 3))
        foot = (sc["foot"].reshape(nb, 1, 4, 3) - vd * p["dt"] * np.arange(h).reshape(1, h, 1, 1) * 40.0).reshape(nb, h * 12); fs = 12
    if cont:
        sw = rng.integers(0, h + 1, (nb, 4)); first = rng.integers(0, 2, (nb, 4))
        contact = np.where(np.arange(h).reshape(1, h, 1) < sw[:, None, :], first[:, None, :],
                1 - first[:, None, :]).astype(np.uint8).reshape(nb, h * 4); cs = 4
    return sc, np.ascontiguousarray(foot), fs, np.ascontiguousarray(contact), cs


def _oracle_update_ticks(oracle, pr, st, scs, carries):
    """one update-path tick of every robot b (its own carry) on the oracle"""
    n = len(scs["x0"])
    grf = np.zeros((n, 12)); it = np.zeros(n, np.int32); stt = np.zeros(n, np.int32)
    for b in range(n):
        o = oracle.mpc_solve_update(pr, st, scs["x0"][b], scs["xref"][b], scs["R"][b], scs["foot"][b], scs["contact"][b], carries[b])
        grf[b] = o["grf"]; it[b] = o["info"].iters; stt[b] = o["info"].status
    return grf, it, stt


# ---------------------------------------------------------------------------------------------------------------- gait cycles and phase thresholds
# The reference's gait counters are small multiples of the speed: once per cycle and leg they land exactly on counter_per_swing (120), on 1.5 x counter_per_swing (180) and on
# counter_per_gait (240, where fmod gives 0), and every branch of the caller-side kernels compares against one of those values.  The builders below give the tests such counters
# (exactly representable, so every later counter is exact too) and sensor forces that sit on the force thresholds.

PER_GAIT, PER_SWING = 240.0, 120.0                    # counter_per_gait / counter_per_swing, S/A1CtrlStates.h:24-25
GAIT_RESET = np.array([0.0, 120.0, 120.0, 0.0])       # what update_plan writes while the robot stands (S/A1RobotControl.cpp:150-153)
DEFAULT_FOOT_POS = np.array([0.17, 0.15, -0.35, 0.17, -0.15, -0.35, -0.17, 0.15, -0.35, -0.17, -0.15, -0.35])
FORCE_CONTACT = np.array([0.0, 30.0, np.nextafter(30.0, np.inf), 80.0])               # around foot_force_low = 30 (early contact needs ff > 30)
FORCE_EKF = np.array([-5.0, 0.0, np.nextafter(50.0, 0.0), 50.0, 100.0, 250.0])        # around the EKF's contact estimate (ff / 100 < 0.5 -> 0), both clamps included
FORCE_TICK = np.unique(np.concatenate([FORCE_CONTACT, FORCE_EKF]))                    # one foot_force array feeds both stages of the control tick


def gait_cycle_fleet(n, speeds=(2.0, 1.5, 3.0, 2.0), stagger_ticks=7, per_gait=PER_GAIT, reset=GAIT_RESET):
    """(gait_counter (n, 4), gait_counter_speed (n, 4)): leg l of every robot runs at speeds[l]; robot b starts stagger_ticks * b ticks after the reset pattern `reset` of
    a gait with period per_gait.  At any tick some robot of the fleet is at a lift-off, at the early-contact mark or at the wrap (the reference's gait, the default: 120,
    180 and 0)."""
    spd = np.tile(np.asarray(speeds, dtype=np.float64), (n, 1))
    gc = np.fmod(np.asarray(reset, dtype=np.float64) + spd * float(stagger_ticks) * np.arange(n, dtype=np.float64)[:, None], per_gait)
    return gc, spd


def stand_timetable(n, ticks):
    """(ticks, n) uint8 movement_mode: walk, stand for 1 .. 5 ticks, walk again -- at another tick for every robot.  A robot that has stood restarts from the reset pattern and
    has lost its stagger, so only the robots of every other block of eight stand; the other blocks walk throughout and keep every phase of the fleet present (a counter's
    phase repeats every 120 robots, and b and b + 120 lie in blocks of different kinds)."""
    t = np.arange(ticks)[:, None]; b = np.arange(n)[None, :]
    start = ticks // 8 + (11 * b) % max(1, ticks // 2)
    stand = (t >= start) & (t < start + 1 + b % 5) & ((b // 8) % 2 == 0)
    return np.where(stand, 0, 1).astype(np.uint8)


def gait_loop(gc, spd, mm, per_gait=PER_GAIT, per_swing=PER_SWING, reset=GAIT_RESET):
    """update_plan's counter rule as plain numpy (S/A1RobotControl.cpp:150-164): -> (gait_counter, plan_contacts) after one tick with movement_mode mm (n)"""
    walk = np.asarray(mm).astype(bool)[:, None]
    g = np.where(walk, np.fmod(gc + spd, per_gait), np.asarray(reset, dtype=np.float64))
    return g, np.where(walk, g <= per_swing, True).astype(np.uint8)


def gait_counts(gc0, spd, mm_table, per_gait=PER_GAIT, per_swing=PER_SWING, reset=GAIT_RESET, early_mark=None):
    """the counters after each tick of the timetable (ticks, n, 4) and hits = {x: how often a counter of a walking robot is exactly x after its increment} for x = the
    lift-off mark (per_swing), the early-contact mark (1.5 x the CONTACT stage's counter_per_swing; default 1.5 * per_swing) and the wrap (0)"""
    gc = gc0.copy(); seq = []
    for mm in mm_table:
        gc, _ = gait_loop(gc, spd, mm, per_gait, per_swing, reset); seq.append(gc)
    seq = np.array(seq); walking = np.asarray(mm_table).astype(bool)[:, :, None]
    early_mark = 1.5 * per_swing if early_mark is None else early_mark
    return seq, {x: int(((seq == x) & walking).sum()) for x in (float(per_swing), float(early_mark), 0.0)}


def assert_thresholds_are_hit(gc0, spd, mm_table, per_gait=PER_GAIT, per_swing=PER_SWING, reset=GAIT_RESET, early_mark=None):
    """The input-side assertion of the gait-cycle tests, made before any kernel output is looked at: over the run the counters equal the lift-off mark (per_swing), the
    early-contact mark (early_mark, default 1.5 * per_swing) and the wrap (0) at least n times each, once per robot on average.  A run shorter than the fastest leg's cycle
    (per_gait over the largest speed) cannot reach that; there every single tick must hit each of the three marks on some robot, and the count must reach n * ticks over
    the slowest leg's cycle length -- what that leg alone contributes to a uniformly staggered fleet.  The reference's gait with speeds (2, 1.5, 3, 2), the defaults: marks
    120 / 180 / 0, cycles of 80 and 160 ticks."""
    ticks, n = np.asarray(mm_table).shape
    seq, hits = gait_counts(gc0, spd, mm_table, per_gait, per_swing, reset, early_mark)
    lift, early = float(per_swing), float(1.5 * per_swing if early_mark is None else early_mark)
    fastest, slowest = int(per_gait / np.max(spd)), int(per_gait / np.min(spd))
    print(f"n {n} ticks {ticks}: gait_counter == {lift:g} / {early:g} / 0 after the increment {hits[lift]} / {hits[early]} / {hits[0.0]} times")
    if ticks >= fastest:
        assert min(hits.values()) >= n, hits
    else:
        walking = np.asarray(mm_table).astype(bool)[:, :, None]
        for x in hits:
            assert ((seq == x) & walking).any(axis=(1, 2)).all() and hits[x] >= n * ticks // slowest, (x, hits)
    return seq, hits


def threshold_forces(rng, shape, values=FORCE_CONTACT):
    """foot_force drawn from a few values that sit ON the thresholds of the kernels that read it"""
    return rng.choice(values, size=shape)


def tick_inputs_timetable(scen, rng, n, movement_mode, gait_counter_speed, forces=FORCE_TICK):
    """tick_inputs with the given movement_mode (one row of stand_timetable) and per-leg speeds, and foot_force on the thresholds"""
    inp = tick_inputs(scen, rng, n)
    inp.update(movement_mode=np.ascontiguousarray(movement_mode, dtype=np.uint8), gait_counter_speed=np.ascontiguousarray(gait_counter_speed, dtype=np.float64),
               foot_force=threshold_forces(rng, (n, 4), forces))
    return inp


def tick_world(n, dev, counters):
    """the device arrays of one handle's control ticks (state carried from tick to tick, outputs); counters: (4,) or (n, 4)"""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    init = dict(gait_counter=np.array(np.broadcast_to(np.asarray(counters, dtype=np.float64), (n, 4))), root_pos=np.tile([0.0, 0.0, 0.3], (n, 1)))
    return dict(state={k: T(init.get(k, np.zeros((n, m)))) for k, m in TICK_STATE.items()},
                outs={k: torch.zeros((n, m) if m > 1 else (n,), dtype=torch.float64, device=dev) for k, m in TICK_OUT_F64.items()},
                u8={k: torch.zeros((n, 4), dtype=torch.uint8, device=dev) for k in ("estimated_contacts", "plan_contacts", "contacts")},
                i32={k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("iters", "status")})


def tick_buffers(E, inp, w):
    bf = E.TickBuffers()
    for k in E.TICK_BUFFER_FIELDS:
        src = inp if k in inp else next(g for g in (w["state"], w["outs"], w["u8"], w["i32"]) if k in g)
        setattr(bf, k, src[k].data_ptr())
    return bf


def assert_worlds_equal(t, w1, w2):
    """every output and carried state of two tick worlds, NaN-aware"""
    for grp in ("state", "outs", "u8", "i32"):
        for k in w1[grp]:
            a, b = w1[grp][k].cpu().numpy(), w2[grp][k].cpu().numpy()
            assert np.array_equal(a, b, equal_nan=True), (t, k, np.abs(a.astype(float) - b.astype(float)).max())


class TickChain:
    """One control tick as the *_device entry points chained by hand on a handle of its own: leg state -> EKF -> plan -> swing legs -> contacts / terrain -> MPC from tick
    records -> joint torques (the seven entries a1mpc_control_tick_device is documented to equal).  With a preview config the solve is a1mpc_horizon_preview_batch_device
    (footholds=True: a1mpc_horizon_preview_footholds_batch_device fed the chain's own foot_pos_target_abs) + a1mpc_solve_batch_ticks_strided_device; the schedule and the
    per-step feet it produced stay readable in .sched_d / .feet_d."""

    def __init__(self, eng, prm, n, stream, preview=None, footholds=False):
        import ctypes as C
        import torch
        self.eng, self.prm, self.n, self.st, self.pv, self.footholds = eng, prm, n, stream, preview, footholds
        self.sp = C.c_void_p(stream.cuda_stream)
        h = eng.horizon; dev = torch.device("cuda", 0)
        self.sched_d = torch.zeros((n, 4 * h), dtype=torch.uint8, device=dev) if preview is not None and preview.contact_schedule else None
        self.feet_d = torch.zeros((n, 12 * h), dtype=torch.float64, device=dev) if preview is not None and preview.foot_preview else None

    def tick(self, inp, w):
        import ctypes as C
        import torch
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        dp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        n, prm, sp, st, pv = self.n, self.prm, self.sp, self.st, self.pv
        k = {f: np.array(getattr(prm, f)) for f in ("kp_foot", "kd_foot", "km_foot", "rho_fix", "rho_opt")}   # (read at every tick: the caller may change them between ticks)
        s7, o7, b7, j7, L, H_ = w["state"], w["outs"], w["u8"], w["i32"], self.eng.lib, self.eng._h
        rcs = [L.a1mpc_leg_state_batch_device(H_, n, ptr(inp["joint_pos"]), ptr(inp["joint_vel"]), ptr(inp["R_world"]), ptr(s7["root_pos"]), ptr(s7["root_lin_vel"]),
                                              dp_(k["rho_fix"]), dp_(k["rho_opt"]), ptr(o7["foot_pos_rel"]), ptr(o7["j_foot_blocks"]), ptr(o7["foot_vel_rel"]),
                                              ptr(o7["foot_pos_abs"]), ptr(o7["foot_vel_abs"]), ptr(o7["foot_pos_world"]), ptr(o7["foot_vel_world"]), sp),
               L.a1mpc_ekf_update_batch_device(H_, n, prm.control_dt, prm.assume_flat_ground, ptr(inp["movement_mode"]), ptr(inp["foot_force"]), ptr(inp["R_world"]), ptr(inp["imu_acc"]),
                                               ptr(inp["imu_ang_vel"]), ptr(o7["foot_pos_rel"]), ptr(o7["foot_vel_rel"]), ptr(s7["root_pos"]), ptr(s7["root_lin_vel"]),
                                               ptr(b7["estimated_contacts"]), sp),
               L.a1mpc_update_plan_batch_device(H_, C.byref(prm.gait), n, ptr(inp["movement_mode"]), ptr(s7["gait_counter"]), ptr(inp["gait_counter_speed"]),
                                                ptr(s7["root_lin_vel"]), ptr(inp["R_z"]), ptr(inp["R_world"]), ptr(s7["root_pos"]), ptr(inp["root_lin_vel_d"]),
                                                ptr(b7["plan_contacts"]), ptr(o7["foot_pos_target_rel"]), ptr(o7["foot_pos_target_abs"]), ptr(o7["foot_pos_target_world"]), sp),
               L.a1mpc_swing_legs_batch_device(H_, n, prm.gait.counter_per_swing, prm.control_dt, ptr(inp["R_z"]), ptr(o7["foot_pos_abs"]), ptr(s7["gait_counter"]),
                                               ptr(o7["foot_pos_target_rel"]), dp_(k["kp_foot"]), dp_(k["kd_foot"]), ptr(s7["foot_pos_start"]),
                                               ptr(s7["foot_pos_rel_last_time"]), ptr(s7["foot_pos_target_last_time"]), ptr(o7["foot_pos_cur"]), ptr(o7["foot_forces_kin"]), sp)]
        with torch.cuda.stream(st):
            pz = s7["root_pos"][:, 2].contiguous(); pitch = s7["root_euler_d"][:, 1].contiguous()
        rcs.append(L.a1mpc_contact_terrain_batch_device(H_, C.byref(prm.contact), n, ptr(s7["gait_counter"]), ptr(b7["plan_contacts"]), ptr(inp["foot_force"]),
                                                        ptr(o7["foot_pos_abs"]), ptr(pz), ptr(pitch), ptr(b7["contacts"]), ptr(o7["foot_pos_recent_contact"]),
                                                        ptr(o7["terrain_angle"]), sp))
        with torch.cuda.stream(st):
            s7["root_euler_d"][:, 1] = pitch
            tick = torch.cat([inp["root_euler"], s7["root_pos"], inp["root_ang_vel"], s7["root_lin_vel"], s7["root_euler_d"], inp["root_lin_vel_d"], inp["root_ang_vel_d"],
                              inp["root_pos_d_z"].reshape(n, 1)], 1).contiguous()
        if pv is None:
            rcs.append(L.a1mpc_solve_batch_ticks_device(H_, n, ptr(tick), ptr(inp["R_world"]), ptr(o7["foot_pos_abs"]), ptr(b7["contacts"]), ptr(o7["grf"]), None,
                                                        ptr(j7["iters"]), ptr(j7["status"]), sp))
        else:
            sched, feet = self.sched_d, self.feet_d
            head = (H_, C.byref(pv), C.byref(prm.gait), n, ptr(inp["movement_mode"]), ptr(s7["gait_counter"]), ptr(inp["gait_counter_speed"]), ptr(b7["contacts"]),
                    ptr(o7["foot_pos_abs"]), ptr(inp["R_world"]), ptr(inp["root_lin_vel_d"]))
            if self.footholds:
                rcs.append(L.a1mpc_horizon_preview_footholds_batch_device(*head, ptr(o7["foot_pos_target_abs"]), ptr(sched), ptr(feet), sp))
            else:
                rcs.append(L.a1mpc_horizon_preview_batch_device(*head, ptr(sched), ptr(feet), sp))
            rcs.append(L.a1mpc_solve_batch_ticks_strided_device(H_, n, ptr(tick), ptr(inp["R_world"]), ptr(feet if feet is not None else o7["foot_pos_abs"]),
                                                                12 if feet is not None else 0, ptr(sched if sched is not None else b7["contacts"]),
                                                                4 if sched is not None else 0, None, ptr(o7["grf"]), None, ptr(j7["iters"]), ptr(j7["status"]), sp))
        rcs.append(L.a1mpc_joint_torques_batch_device(H_, n, ptr(inp["mpc_active"]), ptr(b7["contacts"]), ptr(o7["j_foot_blocks"]), ptr(o7["grf"]), ptr(o7["foot_forces_kin"]),
                                                      dp_(k["km_foot"]), ptr(inp["torques_gravity"]), ptr(s7["joint_torques"]), sp))
        assert not any(rcs), (rcs, L.a1mpc_last_error())


# ---- N2b at its thresholds: the same rows for the GPU entry (tests/test_gpu_gait_cycle.py) and the host-compiled kernel text (tests/test_n2b_host.py) ----
# per tick (gait_counter, plan_contact, foot_force, the contact the reference computes: S/A1RobotControl.cpp:256-271).  An early contact needs gc above the early-contact
# mark AND ff above foot_force_low, and is kept until a gc at or below the mark clears it, whatever the force does meanwhile.
def contact_scripts(per_swing=PER_SWING, low=30.0, contact_per_swing=None, per_gait=PER_GAIT):
    """the two six-tick scripts for a gait whose legs lift off above per_swing, with the early-contact mark m = 1.5 x contact_per_swing (default per_swing) and the force
    threshold `low`: every counter is m, the double above it, or a whole number of counts on the stated side of m and per_swing, the last one two counts before the wrap"""
    m = 1.5 * (per_swing if contact_per_swing is None else contact_per_swing)
    up_m, up_low = np.nextafter(m, np.inf), np.nextafter(low, np.inf)
    swing_below = per_swing + 2.0   # a swing counter at or below the mark (122 by default)
    assert per_swing < swing_below <= m and m + 4.0 < per_gait - 2.0
    return [
        # the early-contact flag from tick to tick: set, kept at a low force up to the wrap, cleared in stance, NOT set again at the mark exactly
        [(m + 2.0, 0, low + 50.0, 1), (m + 4.0, 0, 5.0, 1), (per_gait - 2.0, 0, 5.0, 1), (0.0, 1, 5.0, 1), (swing_below, 0, 5.0, 0), (m, 0, low + 50.0, 0)],
        # the two comparisons on their own: the mark / the next double, the force threshold / the next double (the mark row in between clears the flag)
        [(m, 0, low + 50.0, 0), (up_m, 0, low + 50.0, 1), (m, 0, low + 50.0, 0), (m + 2.0, 0, low, 0), (m + 2.0, 0, up_low, 1), (m + 2.0, 0, 0.0, 1)],
    ]


CONTACT_SCRIPTS = contact_scripts()   # the reference's gait: 180 and the next double, 30 N and the next double
Z_STANDING = np.array([0.1, np.nextafter(0.1, 1.0), 0.3])    # root_pos_z > 0.1 is "standing": 0.1 itself is not


def contact_threshold_run(step, oracle, n, angle_tol, scripts=None, adapt=1, **contact_kw):
    """The scripts above tiled over n robots x 4 legs (robot b, leg l runs script (b + l) % 2) for six ticks, root_pos_z cycling through Z_STANDING, feet on the plane
    z = 0.2 x - 0.3.  First the ORACLE is held to the tabulated contacts and to the standing rule, then `step` (gait_counter, plan, foot_force, foot_pos_abs, root_pos_z,
    pitch -> dict) to the oracle: contacts and filtered positions bit for bit, terrain angle and pitch within angle_tol.  scripts / contact_kw (counter_per_swing,
    foot_force_low of oracle.contact_terrain_step): another contact config; adapt = 0: use_terrain_adapt off, the pitch must come back bit-unchanged.
    -> the worst angle / pitch distance"""
    scripts = CONTACT_SCRIPTS if scripts is None else scripts
    which = (np.arange(n)[:, None] + np.arange(4)[None, :]) % 2
    z = Z_STANDING[np.arange(n) % 3]
    xy = np.outer([0.2, 0.2, -0.2, -0.2], [1.0, 0.0]) + np.outer([1, -1, 1, -1], [0.0, 0.13])
    foot = np.tile(np.c_[xy, 0.2 * xy[:, 0] - 0.3].reshape(12), (n, 1))
    states = [oracle.contact_state() for _ in range(n)]
    pitch_k = np.full(n, 0.125); pitch_o = np.full(n, 0.125)
    seen = set(); worst = 0.0
    for t in range(6):
        row = np.array([[scripts[s][t] for s in w] for w in which])   # (n, 4, 4)
        gc, plan, ff, expect = row[:, :, 0], row[:, :, 1].astype(np.uint8), row[:, :, 2], row[:, :, 3].astype(np.uint8)
        ref = [oracle.contact_terrain_step(states[b], gc[b], plan[b], ff[b], foot[b], z[b], pitch_o[b], use_terrain_adapt=adapt, **contact_kw) for b in range(n)]
        ct_o = np.array([r[0] for r in ref]); rec_o = np.array([r[1] for r in ref]); ang_o = np.array([r[2] for r in ref]); pitch_o = np.array([r[3] for r in ref])
        assert np.array_equal(ct_o, expect), (t, np.argwhere(ct_o != expect)[:4])
        if adapt:
            assert (ang_o[z <= 0.1] == 0.0).all() and (pitch_o[z <= 0.1] == 0.0).all() and (ang_o[z > 0.1] > 0.0).all(), t   # z = 0.1: no angle is filtered, the pitch is +-0
        else:
            assert (ang_o[z <= 0.1] == 0.0).all() and (ang_o[z > 0.1] > 0.0).all() and (pitch_o == 0.125).all(), t
        seen |= set(expect.ravel().tolist())
        out = step(gc, plan, ff, foot, z, pitch_k); pitch_k = out["root_euler_d_pitch"]
        assert np.array_equal(out["contacts"], ct_o), (t, np.argwhere(out["contacts"] != ct_o)[:4])
        assert np.array_equal(out["foot_pos_recent_contact"], rec_o), t
        da, dp = np.abs(out["terrain_angle"] - ang_o).max(), np.abs(pitch_k - pitch_o).max()
        worst = max(worst, da, dp)
        assert da <= angle_tol and dp <= angle_tol, (t, da, dp)
        assert (out["terrain_angle"][z <= 0.1] == 0.0).all() and (out["terrain_angle"][z > 0.1] > 0.0).all(), t
        if not adapt:
            assert (pitch_k == 0.125).all(), t
    assert seen == {0, 1}
    return worst


def steep_plane_run(step, oracle, angle_tol, n=8, ticks=110):
    """All feet in contact on the plane z = +-0.75 x - 0.3 (rising for even robots, falling for odd ones): atan(0.75) = 0.6435 rad averaged over the 100-tick window passes
    the 0.5 clamp at tick 77, and root_euler_d_pitch ends at -0.5 (rising: F_R_diff > 0.05) / +0.5 (falling).  Both signs of the branch and the clamp are asserted to have
    occurred in the ORACLE's run; `step` is held to the oracle on every tick."""
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    xy = np.outer([0.2, 0.2, -0.2, -0.2], [1.0, 0.0]) + np.outer([1, -1, 1, -1], [0.0, 0.13])
    foot = np.array([np.c_[xy, s * 0.75 * xy[:, 0] - 0.3].reshape(12) for s in sign])
    gc = np.zeros((n, 4)); plan = np.ones((n, 4), np.uint8); ff = np.full((n, 4), 80.0); z = np.full(n, 0.3)
    states = [oracle.contact_state() for _ in range(n)]
    pitch_k = np.zeros(n); pitch_o = np.zeros(n)
    first_clamped = None
    for t in range(ticks):
        ref = [oracle.contact_terrain_step(states[b], gc[b], plan[b], ff[b], foot[b], z[b], pitch_o[b]) for b in range(n)]
        ang_o = np.array([r[2] for r in ref]); pitch_o = np.array([r[3] for r in ref])
        if first_clamped is None and (ang_o == 0.5).all():
            first_clamped = t
        out = step(gc, plan, ff, foot, z, pitch_k); pitch_k = out["root_euler_d_pitch"]
        assert np.array_equal(out["contacts"], np.array([r[0] for r in ref])) and np.array_equal(out["foot_pos_recent_contact"], np.array([r[1] for r in ref])), t
        da, dp = np.abs(out["terrain_angle"] - ang_o).max(), np.abs(pitch_k - pitch_o).max()
        assert da <= angle_tol and dp <= angle_tol, (t, da, dp)
    assert first_clamped == 77, first_clamped
    assert (pitch_o[sign > 0] == -0.5).all() and (pitch_o[sign < 0] == 0.5).all(), pitch_o
    assert np.array_equal(pitch_k, pitch_o)   # the clamp value itself is exact on either side


# ---- non-default settings and failure statuses on every kernel family (tests/test_gpu_settings_kernel_families.py) ----
FRICTION_CASES = [(0.6, 0.0, 120.0), (0.3, 5.0, 180.0), (0.15, 0.0, 60.0)]     # (mu, fz_min, fz_max) of test_other_friction_and_force_limits
PARAM_KEYS = ("mu", "fz_min", "fz_max")
# a case is one flat dict: OSQP settings of a1mpc_config and / or the friction / force-limit constants
# scaling = 1 beside SETTINGS_CASES' scaling = 3: Ruiz equilibration of these QPs is at its fixed point after two passes (2, 3, 9 and 10 passes give the same forces to the last
# bits -- measured), so scaling = 3 cannot see a pass count that is off by one.  scaling = 1 catches a kernel family that runs NO pass where one is asked for (one pass against
# none moves the forces far above the bar).  It catches nothing finer: one pass against two differs by 9e-11 N (h = 10) / 1.6e-10 N (h = 16) on the oracle, five orders below
# TOL_FORCE_N, and a slightly stale table or a missed exchange in a single pass is of that size too -- these stay with the bit-for-bit comparisons between the kernel families
FAMILY_CASES = SETTINGS_CASES + [dict(scaling=1)] + [dict(zip(PARAM_KEYS, c)) for c in FRICTION_CASES]
FAMILY_SUBSET = [dict(scaling=0), dict(scaling=1), dict(scaling=3), dict(rho=0.01, adaptive_rho=0), dict(check_termination=10, adaptive_rho_interval=35), dict(max_iter=30),
                 dict(zip(PARAM_KEYS, FRICTION_CASES[1]))]
# the cases on which ADMM amplifies the last bits of the linear solves most (the oracle's own two back ends part by more than the parity bar on up to 9 % of a batch there):
# up to 6 % of a batch may be settled by the extended-precision yardstick, under 1 % on every other case
NOISY_CASES = [dict(scaling=0), dict(rho=1.0), dict(check_termination=10, adaptive_rho_interval=35)]
X87_PCT_NOISY, X87_PCT = 6, 1


def case_id(case):
    return ",".join(f"{k}={v}" for k, v in case.items())


def split_case(case):
    """-> (OSQP settings overrides, robot-constant overrides) of one FAMILY_CASES entry"""
    return {k: v for k, v in case.items() if k not in PARAM_KEYS}, {k: v for k, v in case.items() if k in PARAM_KEYS}


def family_scenario(scen, h, n, par, seed=None):
    """n random QPs at horizon h from the generator the suite uses for that horizon (h = 20: the divergent configuration), seed 9100 + h, with the robot constants `par`"""
    gen = {16: scen.config4_random_h16, 20: scen.config5_divergent}.get(h)
    seed = 9100 + h if seed is None else seed
    sc = gen(nb=n, seed=seed) if gen is not None else scen.config3_random_flat(nb=n, seed=seed, horizon=h)
    sc["params"] = dict(sc["params"], **par)
    return sc


def oracle_sample(n, k=96):
    """k indices spread over a batch of n, the first and the last QP included"""
    return np.unique(np.round(np.linspace(0, n - 1, min(n, k))).astype(np.int64))


def oracle_strided(oracle, pr, st, sc, foot, fs, contact, cs, idx, threads=16):
    """the QPs `idx` of a general-path batch (per-step feet / a contact schedule) through oracle.mpc_solve, one call per QP spread over a few threads (the oracle is
    re-entrant and ctypes drops the GIL; its batch entry takes no strides) -> dict(u, grf, iters, status) in the order of idx"""
    from concurrent.futures import ThreadPoolExecutor
    h = pr.horizon
    ref = dict(u=np.zeros((len(idx), 12 * h)), grf=np.zeros((len(idx), 12)), iters=np.zeros(len(idx), np.int32), status=np.zeros(len(idx), np.int32))

    def one(j):
        b = int(idx[j])
        r = oracle.mpc_solve(pr, st, sc["x0"][b], sc["xref"][b], sc["R"][b], foot[b], contact[b], foot_stride=fs, contact_stride=cs)
        ref["u"][j], ref["grf"][j], ref["iters"][j], ref["status"][j] = r["u"], r["grf"], r["info"].iters, r["info"].status
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(len(idx))))
    return ref


def assert_all_three_outcomes(status):
    """the precondition of the max_iter = 30 cases, on the ORACLE's answer: MAX_ITER_REACHED, SOLVED_INACCURATE and SOLVED all occur"""
    seen = dict(zip(*np.unique(status, return_counts=True)))
    assert set(seen) == {-2, 1, 2}, seen
    return seen


def held_to_oracle(out, ref, x87_solve, case, label=""):
    """The gate of the settings x kernel-family matrix.  out / ref: dict(u, grf, iters, status) of the same k QPs (engine, oracle).
    1. every QP stops at the oracle's iteration with the oracle's status (helpers.compare, min_same = 1.0);
    2. forces (every horizon step and the first step's GRFs) within TOL_FORCE_N -- or, for fewer than X87_PCT per cent of the QPs (at most X87_PCT_NOISY per cent on NOISY_CASES), settled by the
       extended-precision build of the oracle: x87_solve(j) -> dict(u, grf, iters) of QP j re-solved in 80-bit arithmetic stops at the same iteration as both, and the engine
       is no further from it than 5 x the double-precision oracle's own distance + TOL_FORCE_N.
    -> dict(resolved, worst (N, engine vs oracle), worst_ratio (d(engine, x87) / d(oracle, x87) over the resolved QPs))"""
    from helpers import TOL_FORCE_N, compare
    compare(out, ref, tol=np.inf, min_same=1.0)
    k = len(out["iters"])
    d = np.maximum(np.abs(out["u"] - ref["u"]).reshape(k, -1).max(1), np.abs(out["grf"] - ref["grf"]).reshape(k, -1).max(1))
    cand = np.flatnonzero(~(d <= TOL_FORCE_N))       # (a NaN is a candidate, and fails below)
    noisy = case in NOISY_CASES
    allowed = (X87_PCT_NOISY * k) // 100 if noisy else (X87_PCT * k - 1) // 100     # noisy: at most 6 % of the batch; otherwise fewer than 1 %
    print(f"{label} {case_id(case)}: {k} QPs, worst engine-vs-oracle {d.max():.2e} N, {len(cand)} above the bar ({allowed} may be)")
    rows = []      # every figure is printed before anything is asserted; no more QPs are re-solved than a passing case could need (+ a few, for the report)
    for j in cand[np.argsort(-np.nan_to_num(d[cand], nan=np.inf))][:allowed + 4]:
        xr = x87_solve(int(j))
        full = lambda r: np.concatenate([np.ravel(r["u"][j]), np.ravel(r["grf"][j])])
        xe = np.concatenate([np.ravel(xr["u"]), np.ravel(xr["grf"])])
        rows.append((int(j), float(d[j]), float(np.abs(full(out) - xe).max()), float(np.abs(full(ref) - xe).max()), int(xr["iters"]), int(out["iters"][j])))
    if rows:
        print(f"{label} {case_id(case)}: (qp, engine-vs-oracle, engine-vs-x87, oracle-vs-x87, x87 iterations, engine iterations): {rows}")
    assert len(cand) <= allowed, (label, case, len(cand), k, rows)
    for j, dj, d_e, d_o, it_x, it_e in rows:
        assert it_x == it_e, (label, case, rows)
        assert d_e <= 5.0 * d_o + TOL_FORCE_N, (label, case, rows)
    worst_ratio = max([r[2] / max(r[3], 1e-300) for r in rows], default=0.0)
    return dict(resolved=int(len(cand)), worst=float(d.max()), worst_ratio=float(worst_ratio))


# ---- the caller-side kernels and control ticks at non-default parameters (tests/test_gpu_caller_side_params.py, and on the CPU tests/test_ref_pin.py, tests/test_n2b_host.py) ----
# Set A: every quantity that exists twice is different in its two places (gait.counter_per_swing 120 / contact.counter_per_swing 100, gait.control_dt 0.004 / control_dt
# 0.002) and nothing is at the reference's default.  Set B: another period, proportional (320 / 160 in both configs, both dt 0.005): the counters pass 240 and the swing spline
# reaches 1.  The counters are exact multiples of the speeds below and land on each set's lift-off mark (gait.counter_per_swing), early-contact mark (1.5 x
# contact.counter_per_swing) and wrap: every mark minus every reset value is a multiple of 10, and every speed divides 10.
PARAM_SPEEDS = (2.0, 2.5, 5.0, 10.0)
_RHO_FIX_A = np.array([[0.19, 0.05, 0.09, 0.25, 0.27], [0.17, -0.045, -0.08, 0.24, 0.26], [-0.185, 0.052, 0.085, 0.26, 0.28], [-0.175, -0.048, -0.088, 0.245, 0.265]])
PARAM_SET_A = dict(
    name="A", counter_per_gait=200.0, counter_per_swing=120.0, gait_dt=0.004, foot_delta_x_limit=0.06, foot_delta_y_limit=0.14,
    default_foot_pos=np.array([0.19, 0.14, -0.33, 0.16, -0.17, -0.36, -0.18, 0.13, -0.31, -0.15, -0.16, -0.38]), gait_counter_reset=(10.0, 110.0, 90.0, 0.0),
    contact_per_swing=100.0, foot_force_low=45.0, control_dt=0.002, assume_flat_ground=0, kp_foot=(250.0, 350.0, 450.0), kd_foot=(6.0, 7.0, 9.0), km_foot=(0.2, 0.05, 0.08),
    rho_fix=_RHO_FIX_A, rho_opt=np.random.default_rng(20).normal(0, 0.01, (4, 3)))
PARAM_SET_B = dict(PARAM_SET_A, name="B", counter_per_gait=320.0, counter_per_swing=160.0, contact_per_swing=160.0, gait_dt=0.005, control_dt=0.005)
PARAM_SETS = dict(A=PARAM_SET_A, B=PARAM_SET_B)
A1_REACH = 0.1805 + 0.047 + 0.0838 + 0.21 + 0.21                     # |ox| + |oy| + |d| + lt + lc of the A1's legs
LEG_BAR_SCALE = float(np.abs(_RHO_FIX_A).sum(axis=1).max() / A1_REACH)   # the leg bars (1e-14 positions / Jacobians, 1e-13 velocities) grow with the largest reach


def early_mark(ps):
    return 1.5 * ps["contact_per_swing"]


def gait_kw(ps):
    """the keyword arguments of gait_cycle_fleet / gait_loop / gait_counts / assert_thresholds_are_hit for a parameter set"""
    return dict(per_gait=ps["counter_per_gait"], per_swing=ps["counter_per_swing"], reset=np.array(ps["gait_counter_reset"]))


def force_bar(ps):
    """the swing legs' foot-force bar: 1e-9 at kp <= 400 and kd / dt = 3200, scaled where the gains scale the output"""
    return 1e-9 * max(1.0, max(ps["kp_foot"]) / 400.0, (max(ps["kd_foot"]) / ps["control_dt"]) / 3200.0)


def oracle_gait(oracle, ps, **over):
    """oracle.gait_params of a set; over: single fields put back (the sensitivity preconditions)"""
    kw = dict(default_foot_pos=ps["default_foot_pos"], counter_per_gait=ps["counter_per_gait"], counter_per_swing=ps["counter_per_swing"], control_dt=ps["gait_dt"],
              dx=ps["foot_delta_x_limit"], dy=ps["foot_delta_y_limit"], reset=ps["gait_counter_reset"])
    kw.update(over)
    return oracle.gait_params(kw.pop("default_foot_pos"), **kw)


def gait_config(E, ps):
    g = E.GaitConfig()
    g.counter_per_gait, g.counter_per_swing, g.control_dt = ps["counter_per_gait"], ps["counter_per_swing"], ps["gait_dt"]
    g.foot_delta_x_limit, g.foot_delta_y_limit = ps["foot_delta_x_limit"], ps["foot_delta_y_limit"]
    g.default_foot_pos[:] = list(ps["default_foot_pos"]); g.gait_counter_reset[:] = list(ps["gait_counter_reset"])
    return g


def contact_config(E, ps, adapt=1):
    c = E.ContactConfig()
    c.counter_per_swing, c.foot_force_low, c.use_terrain_adapt = ps["contact_per_swing"], ps["foot_force_low"], int(adapt)
    return c


def tick_params(E, ps, adapt=1):
    """a1mpc_tick_params of a set, every field written (nothing is taken from a1mpc_default_tick_params)"""
    p = E.TickParams()
    p.gait = gait_config(E, ps); p.contact = contact_config(E, ps, adapt)
    p.control_dt, p.assume_flat_ground = ps["control_dt"], int(ps["assume_flat_ground"])
    p.kp_foot[:] = list(ps["kp_foot"]); p.kd_foot[:] = list(ps["kd_foot"]); p.km_foot[:] = list(ps["km_foot"])
    p.rho_fix[:] = list(np.asarray(ps["rho_fix"]).reshape(20)); p.rho_opt[:] = list(np.asarray(ps["rho_opt"]).reshape(12))
    return p


def force_values(ps):
    """foot_force values ON the thresholds of a set's contact stage (foot_force_low) and of the EKF's contact estimate (50 N)"""
    low = ps["foot_force_low"]
    return np.unique(np.concatenate([[0.0, low, np.nextafter(low, np.inf), low + 50.0], FORCE_EKF]))


def assert_sensitive(label, full, variants):
    """The sensitivity precondition, on the YARDSTICK's results (oracle / numpy), before any kernel output is read: `full` is the tuple of compared arrays (first axis = robots)
    at the full parameter set, variants[name] the same tuple with the one parameter `name` put back to its default.  Every variant must differ from `full` on at least one
    compared element -- or the test could not notice a kernel that ignored that parameter.  Prints the share of robots that differ; -> {name: share}"""
    shares = {}
    for name, var in variants.items():
        n = len(np.asarray(full[0]))
        differ = np.zeros(n, bool)
        for a, b in zip(full, var):
            a, b = np.asarray(a, dtype=np.float64).reshape(n, -1), np.asarray(b, dtype=np.float64).reshape(n, -1)
            differ |= ~((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1)
        shares[name] = float(differ.mean())
    print(f"{label}: share of robots whose yardstick result changes when one parameter goes back to its default: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    dead = [k for k, v in shares.items() if v == 0.0]
    assert not dead, (label, dead)
    return shares


def np_update_plan(ps, mm, gc, spd, v, Rz, R, pos, vd, **over):
    """update_plan (S/A1RobotControl.cpp:148-202) restated in plain numpy for n robots at a parameter set, one rounding per operation in the reference's order:
    -> (gait_counter, plan_contacts, foot_pos_target_rel, _abs, _world).  What holds the oracle where the reference's own constants cannot be moved (the two
    FOOT_DELTA_*_LIMITs, gait_counter_reset); over: single fields of the set replaced"""
    ps = dict(ps, **over)
    n = len(mm); walk = np.asarray(mm).astype(bool)[:, None]
    g = np.where(walk, np.fmod(gc + spd, ps["counter_per_gait"]), np.asarray(ps["gait_counter_reset"], dtype=np.float64))
    pc = np.where(walk, g <= ps["counter_per_swing"], True).astype(np.uint8)
    dfp = np.asarray(ps["default_foot_pos"], dtype=np.float64)
    vrx = Rz[:, 0] * v[:, 0] + Rz[:, 3] * v[:, 1] + Rz[:, 6] * v[:, 2]; vry = Rz[:, 1] * v[:, 0] + Rz[:, 4] * v[:, 1] + Rz[:, 7] * v[:, 2]
    k = np.sqrt(np.abs(dfp[2]) / 9.8)                                  # default_foot_pos(2): the z of leg 0, for every leg
    half = ((ps["counter_per_swing"] / spd) * ps["gait_dt"]) / 2.0    # (n, 4)
    dx = k * (vrx - vd[:, 0])[:, None] + half * vd[:, 0:1]; dy = k * (vry - vd[:, 1])[:, None] + half * vd[:, 1:2]
    dx = np.clip(dx, -ps["foot_delta_x_limit"], ps["foot_delta_x_limit"]); dy = np.clip(dy, -ps["foot_delta_y_limit"], ps["foot_delta_y_limit"])
    rel = np.tile(dfp, (n, 1)).reshape(n, 4, 3).copy(); rel[:, :, 0] += dx; rel[:, :, 1] += dy
    ab = np.stack([R[:, 3 * r, None] * rel[:, :, 0] + R[:, 3 * r + 1, None] * rel[:, :, 1] + R[:, 3 * r + 2, None] * rel[:, :, 2] for r in range(3)], axis=2)
    wo = ab + pos[:, None, :]
    return g, pc, rel.reshape(n, 12), ab.reshape(n, 12), wo.reshape(n, 12)


def np_contacts(gc, plan, ff, early_prev, contact_per_swing, foot_force_low):
    """the early-contact lines (S/A1RobotControl.cpp:259-271) in plain numpy: -> (contacts, early_contacts)"""
    early = np.where(gc <= contact_per_swing * 1.5, False, np.asarray(early_prev, dtype=bool))
    early = early | ((plan == 0) & (gc > contact_per_swing * 1.5) & (ff > foot_force_low))
    return ((plan != 0) | early).astype(np.uint8), early


def plan_inputs(scen, rng, n, ps):
    """random attitude / velocities for update_plan; the commanded velocities of robots 0 .. 7 are +-3 m/s in x or y (both limits saturate on both sides, asserted by the
    caller on the yardstick), every ninth robot is commanded nothing"""
    yaw = rng.uniform(-np.pi, np.pi, n); R = scen.rot_zyx(rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), yaw).reshape(n, 9); Rz = scen.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)
    v = rng.normal(0, 0.3, (n, 3)); vd = np.c_[rng.normal(0, 0.3, (n, 2)), np.zeros(n)]; pos = rng.normal(0, 2.0, (n, 3))
    for b, (ax, sg) in enumerate([(0, 1), (0, -1), (1, 1), (1, -1)] * 2):
        if b < n:
            vd[b, :2] = 0.0; vd[b, ax] = 3.0 * sg
    vd[8::9] = 0.0
    return dict(v=v, Rz=Rz, R=R, pos=pos, vd=vd)


# ---- a generic set of robot constants (tests/test_generic_constants_host.py, tests/test_gpu_generic_constants.py) ----
# Every scenarios.PARAM_SETS entry has a diagonal inertia_body, q[3] = q[4] = 0 and one r repeated over the lanes of a leg (most: over all twelve).  No caller has to keep
# that structure and the kernels do not assume it: the set below has none of it.  inertia = Rr diag(0.0158533, 0.0377999, 0.0456542) Rr', symmetrised, Rr the Rodrigues
# rotation of the vector (-0.2405794275760342, -0.39730769868844346, -0.07450848662857455) (numpy's default_rng(5).normal(0, 0.3, 3)), written out so that it does not
# depend on a generator; r[k] = 1e-7 (1 + k / 4).  dt, mu and the force limits stay the scenario's.
GENERIC_CONSTANTS = dict(
    mass=11.3, q=[20.0, 10.0, 1.0, 3.0, 7.0, 420.0, 0.05, 0.07, 0.03, 30.0, 25.0, 10.0, 0.0],
    r=[1e-07, 1.25e-07, 1.5e-07, 1.75e-07, 2e-07, 2.25e-07, 2.5e-07, 2.75e-07, 3e-07, 3.2499999999999996e-07, 3.5e-07, 3.75e-07],
    inertia=[0.02033138319319339, -0.0002215375332723924, -0.010531835564711142, -0.0002215375332723924, 0.03826292733232652, 0.001943689135907053,
             -0.010531835564711142, 0.001943689135907053, 0.040713089474480074])
GENERIC_MOVE_N = 1e-3     # 100 x helpers.TOL_FORCE_N: what a variant below must move the yardstick's forces by, on at least half of a batch


def generic_params(params, **par):
    """a scenario's parameter dict with the generic constants in place of its mass, inertia, q and r (dt, mu, force limits and the nominal feet stay); par: overrides"""
    out = dict(params, **{k: (list(v) if isinstance(v, list) else v) for k, v in GENERIC_CONSTANTS.items()})
    out.update(par)
    return out


def generic_scenario(scen, h, n, seed=None, **par):
    """family_scenario with the generic constants; par: further robot constants (mu, fz_min, fz_max, or one of generic_variants())"""
    return family_scenario(scen, h, n, generic_params({}, **par), seed=seed)


def generic_variants():
    """{name: constants that replace GENERIC_CONSTANTS' with ONE property put back to the structure of scenarios.PARAM_SETS, or two words exchanged}: what a kernel computes
    that reads a wrong pair of inertia words, drops or swaps q[3] / q[4], indexes r by leg instead of by lane, or was handed the diagonal only"""
    G = GENERIC_CONSTANTS
    I = np.array(G["inertia"]).reshape(3, 3); q = np.array(G["q"]); r = np.array(G["r"])
    swap = I.copy(); swap[0, 1], swap[0, 2] = I[0, 2], I[0, 1]; swap[1, 0], swap[2, 0] = I[2, 0], I[1, 0]
    q67 = q.copy(); q67[[6, 7]] = q[[7, 6]]
    q34 = q.copy(); q34[[3, 4]] = q[[4, 3]]
    q00 = q.copy(); q00[[3, 4]] = 0.0
    return {"off-diagonals zeroed": dict(inertia=np.diag(np.diag(I)).reshape(9).tolist()), "I01 <-> I02": dict(inertia=swap.reshape(9).tolist()),
            "q[6] <-> q[7]": dict(q=q67.tolist()), "q[3] = q[4] = 0": dict(q=q00.tolist()), "q[3] <-> q[4]": dict(q=q34.tolist()),
            "r uniform at its mean": dict(r=[float(r.mean())] * 12), "r rolled by one lane": dict(r=np.roll(r, 1).tolist())}


def assert_variants_move(label, full, variants, move=GENERIC_MOVE_N, share=0.5):
    """The sensitivity precondition of the generic-constants tests, on the YARDSTICK's forces (k, ...) of one batch: every variant must move them by more than `move`
    (100 x TOL_FORCE_N) on at least `share` of the QPs -- or a pass of that batch could not tell the generic set from the structured one.  Prints the shares and medians;
    -> {name: (share, median move)}"""
    k = len(full); out = {}
    for name, var in variants.items():
        d = np.abs(np.asarray(var).reshape(k, -1) - np.asarray(full).reshape(k, -1)).max(axis=1)
        out[name] = (float((d > move).mean()), float(np.median(d)))
    print(f"{label}: share of {k} QPs whose yardstick forces move by more than {move:g} N (median move): " + ", ".join(f"{n} {s:.2f} ({m:.1e} N)" for n, (s, m) in out.items()))
    weak = {n: v for n, v in out.items() if not v[0] >= share}
    assert not weak, (label, weak)
    return out


def oracle_variant_forces(oracle, sc, idx, settings=None, foot=None, fs=0, contact=None, cs=0, **var):
    """the oracle's full-horizon forces (len(idx), 12 h) of the QPs idx of a batch with the robot constants `var` replacing the batch's own"""
    from helpers import oracle_params
    v = dict(sc, params=dict(sc["params"], **var))
    st = oracle.default_settings() if settings is None else settings
    return oracle_strided(oracle, oracle_params(oracle, v), st, v, sc["foot"] if foot is None else foot, fs, sc["contact"] if contact is None else contact, cs, idx)["u"]


def assert_batch_is_sensitive(label, oracle, sc, idx, ref_u, settings=None, **strided):
    """assert_variants_move for the QPs idx of a batch whose yardstick forces at the full set are ref_u"""
    return assert_variants_move(label, ref_u, {name: oracle_variant_forces(oracle, sc, idx, settings, **strided, **var) for name, var in generic_variants().items()})


# the settings cases of the generic-constants tests: the defaults, three Ruiz passes, and the friction / force-limit set with fz_min > 0 (its first iteration touches r)
GENERIC_FAST_CASES = [dict(), dict(scaling=3), dict(zip(PARAM_KEYS, FRICTION_CASES[1]))]


def generic_case_id(case):
    return case_id(case) or "default"


def generic_strided(scen, h, n):
    """_strided_inputs (per-step feet, a contact schedule) of n QPs at horizon h with the generic constants -> (sc, foot, foot_stride, contact, contact_stride)"""
    sc, foot, fs, contact, cs = _strided_inputs(scen, np.random.default_rng(9400 + h + n), h, n, True, True)
    sc["params"] = generic_params(sc["params"])
    return sc, foot, fs, contact, cs


def generic_warm_ticks(scen, h=10, n=64):
    """the four ticks of test_warm_start_modes_with_non_default_settings' pattern on a generic batch (slowly moving states, every leg changing role at tick 2) -> a list of
    four scenarios (the arrays of a tick are copies)"""
    rng = np.random.default_rng(9300 + 7 * h + n)
    sc = generic_scenario(scen, h, n, seed=9300 + h + n)
    ticks = []
    for t in range(4):
        if t > 0:
            sc["x0"][:, :12] += rng.normal(0, 2e-3, (n, 12)); sc["foot"] += rng.normal(0, 1e-3, (n, 12))
        if t == 2:
            sc["contact"][:] = 1 - sc["contact"]
            sc["contact"][sc["contact"].sum(1) == 0] = [1, 0, 0, 1]
        ticks.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()})
    return ticks


def oracle_warm_chain(oracle, x87, ticks, mode, h):
    """every robot of generic_warm_ticks chained through the oracle (mode 1: x, y, rho carried; mode 2: the update path) -> per tick (ref dict(u, grf, iters, status),
    x87_solve(j): the extended-precision solve of robot j's tick from the state the oracle's solve started from)"""
    from helpers import oracle_params
    n = len(ticks[0]["x0"])
    pr = oracle_params(oracle, ticks[0]); st = oracle.default_settings(warm_start=1)
    xpr = x87.params(ticks[0]["params"], h); xst = x87.settings(warm_start=1)
    carries = [oracle.update_carry(h) for _ in range(n)]
    wx = [np.zeros(12 * h) for _ in range(n)]; wy = [np.zeros(20 * h) for _ in range(n)]; rho = [None] * n
    out = []
    for sc in ticks:
        before = [(carries[b].copy(), wx[b].copy(), wy[b].copy(), rho[b]) for b in range(n)]
        ref = dict(u=np.zeros((n, 12 * h)), grf=np.zeros((n, 12)), iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        for b in range(n):
            a = (sc["x0"][b], sc["xref"][b], sc["R"][b], sc["foot"][b], sc["contact"][b])
            if mode == 2:
                o = oracle.mpc_solve_update(pr, st, *a, carries[b])
            else:
                o = oracle.mpc_solve(pr, st, *a, warm_x=wx[b], warm_y=wy[b], warm_rho=rho[b])
                wx[b], wy[b], rho[b] = o["warm_x"], o["warm_y"], o["rho"]
            ref["u"][b], ref["grf"][b], ref["iters"][b], ref["status"][b] = o["u"], o["grf"], o["info"].iters, o["info"].status

        def x87_solve(j, sc=sc, before=before):
            c, x, y, r = before[j]
            a = (sc["x0"][j], sc["xref"][j], sc["R"][j], sc["foot"][j], sc["contact"][j])
            return x87.mpc_solve_update(xpr, xst, *a, c) if mode == 2 else x87.mpc_solve(xpr, xst, *a, warm_x=x, warm_y=y, warm_rho=r)
        out.append((ref, x87_solve))
    return out


def yardstick_alone(label, ref, x87_solve, case, threads=16):
    """The precondition of held_to_oracle's cap, on the yardstick ONLY: ref = the oracle's dict(u, grf, iters, status) of k QPs, x87_solve(j) its extended-precision
    build on QP j.  Both stop at the same iteration on every QP, and the share of QPs further than TOL_FORCE_N apart is within the cap held_to_oracle grants `case`
    (fewer than X87_PCT per cent; at most X87_PCT_NOISY on NOISY_CASES).  -> dict(above, worst)"""
    from concurrent.futures import ThreadPoolExecutor
    from helpers import TOL_FORCE_N
    k = len(ref["iters"])
    with ThreadPoolExecutor(max_workers=threads) as pool:
        xs = list(pool.map(x87_solve, range(k)))
    it_x = np.array([x["iters"] for x in xs])
    d = np.array([max(np.abs(np.ravel(ref["u"][j]) - np.ravel(xs[j]["u"])).max(), np.abs(np.ravel(ref["grf"][j]) - np.ravel(xs[j]["grf"])).max()) for j in range(k)])
    above = int((~(d <= TOL_FORCE_N)).sum())
    allowed = (X87_PCT_NOISY * k) // 100 if case in NOISY_CASES else (X87_PCT * k - 1) // 100
    print(f"{label} {generic_case_id(case)}: {k} QPs, same iteration as x87 on {int((it_x == ref['iters']).sum())}, worst oracle-vs-x87 {d.max():.2e} N, {above} above the bar "
          f"({allowed} may be), statuses {dict(zip(*np.unique(ref['status'], return_counts=True)))}")
    assert np.array_equal(it_x, ref["iters"]), (label, case, np.flatnonzero(it_x != ref["iters"])[:8])
    assert above <= allowed, (label, case, above, allowed)
    return dict(above=above, worst=float(d.max()))
