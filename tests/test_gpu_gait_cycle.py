"""GPU, through the C ABI: the caller-side kernels ON their thresholds and over whole gait cycles.  The reference's gait counters are small multiples of the speed; once per
cycle and leg they are exactly 120 (lift-off: plan_contacts, the swing leg's start latch), 180 (the early-contact mark) and 0 (the wrap of fmod), and the sensor forces decide
at exactly 30 N (early contact) and 50 N (the EKF's contact estimate).  Uniform random floats never land there.  Here they do: threshold tables one stage at a time against
the oracle (which tests/test_ref_pin.py walks through the same boundaries against the reference's compiled sources), a whole cycle of the host chain against the oracle
chain, and a whole cycle of the one-call control ticks against the entries chained by hand, with numpy's fmod loop as the independent anchor of counters and schedules."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import (DEFAULT_FOOT_POS, FORCE_CONTACT, FORCE_EKF, PER_GAIT, PER_SWING, TickChain, _oracle_update_ticks, assert_thresholds_are_hit, assert_worlds_equal,
                        contact_threshold_run, gait_cycle_fleet, gait_loop, stand_timetable, steep_plane_run, threshold_forces, tick_buffers, tick_inputs_timetable, tick_world)
from helpers import TOL_FORCE_N, compare

pytestmark = pytest.mark.gpu

N_TABLE = 67   # 16 robots per wavefront in the leg-lane kernels, 64 in the contact kernel: the last wavefront is partial in both
_UP, _DOWN = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, 0.0))

# (gait_counter before, speed) -> (gait_counter after, plan_contact) of a walking robot, S/A1RobotControl.cpp:156-164
PLAN_ROWS = [(118.0, 2.0, 120.0, 1), (118.5, 1.5, 120.0, 1), (117.0, 3.0, 120.0, 1),
             (238.0, 2.0, 0.0, 1), (238.5, 1.5, 0.0, 1), (237.0, 3.0, 0.0, 1),
             (_UP(118.0), 2.0, 120.00000000000001, 0), (_DOWN(118.0), 2.0, 119.99999999999999, 1), (_DOWN(238.0), 2.0, 239.99999999999997, 0)]
# the counter of one leg over three consecutive calls of the swing-leg stage (each row an exact multiple of its speed, or one double beside the threshold)
SWING_ROWS = [(118.0, 120.0, 122.0), (119.5, 121.0, 122.5), (238.0, 0.0, 2.0), (120.0, _UP(120.0), 122.0), (238.0, _DOWN(240.0), 0.0)]


def _cfg(pkg, scen, h=10, **osqp):
    return pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h, **osqp)


def test_update_plan_at_lift_off_and_wrap(pkg, oracle, scen):
    """PLAN_ROWS tiled over 67 robots x 4 legs, every fifth robot standing.  The oracle is held to the tabulated counters and contacts first (120 <= 120 is stance, one
    double above it is swing; 240 wraps to 0, one double below it does not), then every output of a1mpc_update_plan_batch to the oracle bit for bit."""
    rng = np.random.default_rng(120)
    n = N_TABLE
    row = (4 * np.arange(n)[:, None] + np.arange(4)[None, :]) % len(PLAN_ROWS)
    tab = np.array(PLAN_ROWS)[row]   # (n, 4, 4)
    gc, spd = np.ascontiguousarray(tab[:, :, 0]), np.ascontiguousarray(tab[:, :, 1])
    mm = np.where(np.arange(n) % 5 == 4, 0, 1).astype(np.uint8)
    yaw = rng.uniform(-np.pi, np.pi, n); R = scen.rot_zyx(rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), yaw).reshape(n, 9); Rz = scen.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)
    v = rng.normal(0, 0.6, (n, 3)); vd = rng.normal(0, 0.6, (n, 3)); pos = rng.normal(0, 2.0, (n, 3))
    gp = oracle.gait_params(DEFAULT_FOOT_POS)
    ref = [oracle.update_plan(gp, mm[b], gc[b], spd[b], v[b], Rz[b], R[b], pos[b], vd[b]) for b in range(n)]
    gc_o = np.array([r[0] for r in ref]); pc_o = np.array([r[1] for r in ref])
    walk = mm == 1
    assert np.array_equal(gc_o[walk], tab[walk][:, :, 2]) and np.array_equal(pc_o[walk], tab[walk][:, :, 3].astype(np.uint8))
    assert np.array_equal(gc_o[~walk], np.tile([0.0, 120.0, 120.0, 0.0], ((~walk).sum(), 1))) and (pc_o[~walk] == 1).all()
    assert set(pc_o[walk].ravel().tolist()) == {0, 1}   # or the table is not doing its job
    with pkg.Engine(_cfg(pkg, scen), n, 0) as eng:
        out = eng.update_plan(mm, gc, spd, v, Rz, R, pos, vd)
    assert np.array_equal(out["gait_counter"], gc_o) and np.array_equal(out["plan_contacts"], pc_o)
    for k, j in (("foot_pos_target_rel", 2), ("foot_pos_target_abs", 3), ("foot_pos_target_world", 4)):
        assert np.array_equal(out[k], np.array([r[j] for r in ref])), k


def _bezier(t, start, fin):
    """Utils.cpp:64-104 with the integer powers as products; the z control points carry the 0.4 m clearance"""
    u = 1 - t
    t2, u2 = t * t, u * u
    t3, u3, t4, u4 = t2 * t, u2 * u, t2 * t2, u2 * u2
    P2 = fin + np.array([0.0, 0.0, float(np.float32(0.4))])   # FOOT_SWING_CLEARANCE2 is a float literal
    return u4 * start + 4.0 * t * u3 * start + 6.0 * t2 * u2 * P2 + 4.0 * t3 * u * fin + t4 * fin


def test_swing_legs_latch_at_120_and_float_spline_time(pkg, oracle, scen):
    """SWING_ROWS tiled over 67 robots x 4 legs, three consecutive calls of a1mpc_swing_legs_batch.  foot_pos_start equals foot_pos_cur up to and INCLUDING 120 and is kept
    from then on (one double above 120 already keeps it; one double below 240 is swing, 0 is stance again) -- asserted on the kernel's output itself and bit for bit against
    the oracle.  The spline time is a float quotient (S/A1RobotControl.cpp:233-236): at the non-integer counters the curve is held to a numpy restatement with float32 time
    within 1e-15, and that restatement with double time is shown to lie > 1e-13 away, so the cast is seen."""
    rng = np.random.default_rng(121)
    n = N_TABLE
    row = (4 * np.arange(n)[:, None] + np.arange(4)[None, :]) % len(SWING_ROWS)
    tab = np.array(SWING_ROWS)[row]   # (n, 4, 3)
    st_g = [rng.normal(0, 0.1, (n, 12)) for _ in range(3)]; st_o = [a.copy() for a in st_g]
    cast_seen = 0.0
    with pkg.Engine(_cfg(pkg, scen), n, 0) as eng:
        for call in range(3):
            gcs = np.ascontiguousarray(tab[:, :, call])
            yaw = rng.uniform(-3, 3, n); Rz = scen.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)
            foot = DEFAULT_FOOT_POS + rng.normal(0, 0.03, (n, 12)); tgt = DEFAULT_FOOT_POS + rng.normal(0, 0.05, (n, 12))
            start_before = st_g[0].copy()
            cur, kin = eng.swing_legs(Rz, foot, gcs, tgt, *st_g)
            stance = np.repeat(gcs <= PER_SWING, 3, axis=1)
            assert stance.any() and not stance.all()
            assert np.array_equal(st_g[0][stance], cur[stance]) and np.array_equal(st_g[0][~stance], start_before[~stance]), call   # the latch
            assert np.array_equal(st_g[1], cur)
            for b in range(n):
                c_o, k_o = oracle.swing_legs(Rz[b], foot[b], gcs[b], tgt[b], st_o[0][b], st_o[1][b], st_o[2][b])
                assert np.array_equal(cur[b], c_o) and np.array_equal(st_g[0][b], st_o[0][b]) and np.array_equal(st_g[1][b], st_o[1][b]), (call, b)
                assert np.abs(st_g[2][b] - st_o[2][b]).max() <= 1e-15 and np.abs(kin[b] - k_o).max() <= 1e-9, (call, b, np.abs(kin[b] - k_o).max())
            st_o[2][:] = st_g[2]   # keep the two state copies from drifting apart by the curve's ulp differences
            t32 = np.where(gcs > PER_SWING, ((gcs - PER_SWING).astype(np.float32) / np.float32(PER_SWING)).astype(np.float64), 0.0)
            t64 = np.where(gcs > PER_SWING, (gcs - PER_SWING) / PER_SWING, 0.0)
            y32 = _bezier(t32[:, :, None], st_g[0].reshape(n, 4, 3), tgt.reshape(n, 4, 3)); y64 = _bezier(t64[:, :, None], st_g[0].reshape(n, 4, 3), tgt.reshape(n, 4, 3))
            assert np.abs(st_g[2].reshape(n, 4, 3) - y32).max() <= 1e-15, (call, np.abs(st_g[2].reshape(n, 4, 3) - y32).max())
            frac = (gcs != np.floor(gcs)) & (gcs > PER_SWING + 1.0)   # 121 is 1 / 120 in float; 122.5 is 2.5 / 120
            frac |= gcs == 121.0
            if frac.any():
                cast_seen = max(cast_seen, np.abs(y32 - y64)[frac].max())
    assert cast_seen > 1e-13, cast_seen


def test_contact_terrain_at_180_at_30_newton_and_at_standing_height(pkg, oracle, scen):
    """gpu_common.CONTACT_SCRIPTS through a1mpc_contact_terrain_batch, 67 robots on a handle of 80: gc = 180 against the next double, ff = 30 against the next double, the
    early-contact flag kept over five ticks and cleared in stance, root_pos_z = 0.1 (not standing: angle 0) against the next double.  The same rows run through the
    host-compiled kernel text in tests/test_n2b_host.py."""
    with pkg.Engine(_cfg(pkg, scen), 80, 0) as eng:
        contact_threshold_run(eng.contact_terrain, oracle, N_TABLE, 1e-13)


def test_terrain_angle_clamp_and_both_pitch_signs(pkg, oracle, scen):
    """8 robots on the plane z = +-0.75 x - 0.3 for 110 ticks: the oracle's terrain angle reaches the 0.5 clamp at tick 77 and the pitch ends at -0.5 (rising) / +0.5
    (falling), so both sides of F_R_diff > 0.05 and the clamp have occurred; the kernel is held to the oracle on every tick."""
    with pkg.Engine(_cfg(pkg, scen), 8, 0) as eng:
        steep_plane_run(eng.contact_terrain, oracle, 1e-13)


def test_ekf_contact_estimate_at_50_newton(pkg, oracle, scen):
    """Five ticks of a1mpc_ekf_update_batch, 67 robots, foot_force from {-5, 0, the double below 50, 50, 100, 250} and mixed movement_mode: every output bit for bit against
    the oracle's device variant; the oracle's estimated_contacts is 1 at 50 N and 0 one double below it on walking robots (ec < 0.5, S/A1BasicEKF.cpp:151-157)."""
    rng = np.random.default_rng(50)
    n, ticks = N_TABLE, 5
    states = [oracle.ekf_state() for _ in range(n)]
    base = np.array([0.18, 0.13, -0.3, 0.18, -0.13, -0.3, -0.18, 0.13, -0.3, -0.18, -0.13, -0.3])
    at50 = below50 = 0
    with pkg.Engine(_cfg(pkg, scen), n, 0) as eng:
        for t in range(ticks):
            mm = np.where(rng.random(n) < 0.75, 1, 0).astype(np.uint8) if t > 0 else np.zeros(n, np.uint8)
            yaw = rng.uniform(-3, 3, n); eul = rng.normal(0, 0.05, (n, 2)); R = scen.rot_zyx(eul[:, 0], eul[:, 1], yaw).reshape(n, 9)
            fk = base + rng.normal(0, 0.01, (n, 12)); fv = rng.normal(0, 0.3, (n, 12)); acc = np.array([0.0, 0.0, 9.81]) + rng.normal(0, 0.3, (n, 3))
            w = rng.normal(0, 0.3, (n, 3)); ff = threshold_forces(rng, (n, 4), FORCE_EKF)
            ref = [oracle.ekf_step(states[b], 0.0025, mm[b], ff[b], R[b], acc[b], w[b], fk[b], fv[b], device=True) for b in range(n)]
            ec_o = np.array([r[2] for r in ref])
            if t > 0:   # (the first call of a state initialises it and estimates nothing)
                walk = np.repeat((mm == 1)[:, None], 4, axis=1)
                assert (ec_o[walk & (ff == 50.0)] == 1).all() and (ec_o[walk & (ff == _DOWN(50.0))] == 0).all() and (ec_o[~walk] == 1).all(), t
                at50 += int((walk & (ff == 50.0)).sum()); below50 += int((walk & (ff == _DOWN(50.0))).sum())
            pos, vel, ec = eng.ekf_update(0.0025, mm, ff, R, acc, w, fk, fv)
            assert np.array_equal(ec, ec_o), (t, np.argwhere(ec != ec_o)[:4])
            assert np.array_equal(pos, np.array([r[0] for r in ref])) and np.array_equal(vel, np.array([r[1] for r in ref])), t
    assert at50 >= n and below50 >= n, (at50, below50)


@pytest.mark.parametrize("warm,n", [(0, 32), (2, 16)])
def test_whole_cycle_host_chain_matches_the_oracle_chain(pkg, oracle, scen, warm, n):
    """test_control_tick_chain's composition (update_plan -> swing_legs -> contact_terrain -> solve_ticks -> joint_torques, synthetic sensors) over 125 ticks of the staggered
    fleet, with sensor forces on the 30 N threshold so that early contacts occur: every leg lifts off, passes 180, wraps and touches down while the chain runs.  Per tick and
    robot: counters, planned and actual contacts, footholds, swing start / current positions and filtered contact positions bit for bit; the curve <= 1e-15, the foot force
    <= 1e-9, terrain angle and pitch <= 1e-13; the MPC through helpers.compare (same iterations and status on every QP, forces within TOL_FORCE_N); torques < 1e-5.
    warm_start 0: the oracle's tick is one mpc_solve_batch; warm_start 2: the update path with one oracle carry per robot, across every contact-pattern change -- the
    engine's workspace chains through all 125 ticks, the oracle takes every step from the engine's workspace of the tick before (see the comment at the hand-over)."""
    rng = np.random.default_rng(770 + warm)
    ticks, h = 125, 10
    P = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
    cfg = pkg.make_config(P, h, warm_start=warm)
    pr = oracle.mpc_params(h, P["dt"], P["mu"], P["fz_min"], P["fz_max"], P["q"], P["r"], P["mass"], P["inertia"])
    st = oracle.default_settings(warm_start=1) if warm == 2 else oracle.default_settings()
    carries = [oracle.update_carry(h) for _ in range(n)]
    dfp = DEFAULT_FOOT_POS; gp = oracle.gait_params(dfp); km = np.array([0.1, 0.1, 0.04])
    gc0, spd = gait_cycle_fleet(n)
    mm = np.ones(n, np.uint8)
    assert_thresholds_are_hit(gc0, spd, np.ones((ticks, n), np.uint8))
    G = dict(gc=gc0.copy(), start=np.zeros((n, 12)), rl=np.tile(dfp, (n, 1)), tl=np.tile(dfp, (n, 1)), pitch=np.zeros(n), tau=np.zeros((n, 12)))
    O = dict(gc=gc0.copy(), start=np.zeros((n, 12)), rl=G["rl"].copy(), tl=G["tl"].copy(), pitch=np.zeros(n), tau=np.zeros((n, 12)), ct=[oracle.contact_state() for _ in range(n)])
    worst = dict(tau=0.0, grf=0.0, kin=0.0, angle=0.0, carry_x=0.0, carry_rho=0.0); early = 0; patterns = set()
    with pkg.Engine(cfg, n, 0) as eng:
        for t in range(ticks):
            # synthetic sensors of this tick
            eul = rng.normal(0, 0.05, (n, 3)); eul[:, 2] = rng.uniform(-1, 1, n); pos = np.c_[rng.normal(0, 1, (n, 2)), 0.3 + rng.normal(0, 0.01, n)]
            w = rng.normal(0, 0.3, (n, 3)); v = rng.normal(0, 0.3, (n, 3)); vd = np.c_[rng.uniform(-0.5, 0.5, (n, 2)), np.zeros(n)]; wd = np.c_[np.zeros((n, 2)), rng.uniform(-0.5, 0.5, n)]
            R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9); Rz = scen.rot_zyx(0 * eul[:, 0], 0 * eul[:, 0], eul[:, 2]).reshape(n, 9)
            foot_rel = dfp + rng.normal(0, 0.02, (n, 12))
            foot_abs = np.einsum("nij,nlj->nli", R.reshape(n, 3, 3), foot_rel.reshape(n, 4, 3)).reshape(n, 12)
            ff = threshold_forces(rng, (n, 4), FORCE_CONTACT); Jb = rng.normal(0, 0.2, (n, 36)); Jb[:, [0, 4, 8, 9, 13, 17, 18, 22, 26, 27, 31, 35]] += 0.3
            tg = rng.normal(0, 0.5, (n, 12))
            # ---- device chain
            up = eng.update_plan(mm, G["gc"], spd, v, Rz, R, pos, vd); G["gc"] = up["gait_counter"]
            cur, kin = eng.swing_legs(Rz, foot_abs, G["gc"], up["foot_pos_target_rel"], G["start"], G["rl"], G["tl"])
            ctr = eng.contact_terrain(G["gc"], up["plan_contacts"], ff, foot_abs, pos[:, 2], G["pitch"]); G["pitch"] = ctr["root_euler_d_pitch"]
            tick = scen.pack_tick(eul, pos, w, v, np.c_[np.zeros(n), G["pitch"], eul[:, 2]], vd, wd, np.full(n, 0.3))
            sol = eng.solve_ticks(tick, R, foot_abs, ctr["contacts"])
            G["tau"] = eng.joint_torques(np.ones(n, np.uint8), ctr["contacts"], Jb, sol["grf"], kin, km, tg, G["tau"])
            # ---- oracle chain
            x0 = scen.pack_x0(eul, pos, w, v); xref = np.zeros((n, 13 * h)); ct_o = np.zeros((n, 4), np.uint8); kin_o = np.zeros((n, 12))
            for b in range(n):
                gc2, pc, rel, ab, wo = oracle.update_plan(gp, 1, O["gc"][b], spd[b], v[b], Rz[b], R[b], pos[b], vd[b]); O["gc"][b] = gc2
                c_o, kin_o[b] = oracle.swing_legs(Rz[b], foot_abs[b], gc2, rel, O["start"][b], O["rl"][b], O["tl"][b])
                ct_o[b], rec, ang, O["pitch"][b] = oracle.contact_terrain_step(O["ct"][b], gc2, pc, ff[b], foot_abs[b], pos[b, 2], O["pitch"][b])
                xref[b] = oracle.mpc_reference(h, P["dt"], eul[b], pos[b], R[b], np.array([0.0, O["pitch"][b], eul[b, 2]]), vd[b], wd[b], 0.3)
                early += int(((ct_o[b] == 1) & (pc == 0)).sum())
                assert np.array_equal(G["gc"][b], gc2) and np.array_equal(up["plan_contacts"][b], pc) and np.array_equal(ctr["contacts"][b], ct_o[b]), (t, b)
                assert np.array_equal(up["foot_pos_target_rel"][b], rel) and np.array_equal(up["foot_pos_target_abs"][b], ab) and np.array_equal(up["foot_pos_target_world"][b], wo), (t, b)
                assert np.array_equal(cur[b], c_o) and np.array_equal(G["start"][b], O["start"][b]) and np.array_equal(G["rl"][b], O["rl"][b]), (t, b)
                assert np.array_equal(ctr["foot_pos_recent_contact"][b], rec), (t, b)
                assert np.abs(G["tl"][b] - O["tl"][b]).max() <= 1e-15 and np.abs(kin[b] - kin_o[b]).max() <= 1e-9, (t, b, np.abs(kin[b] - kin_o[b]).max())
                assert abs(ctr["terrain_angle"][b] - ang) <= 1e-13 and abs(G["pitch"][b] - O["pitch"][b]) <= 1e-13, (t, b)
                worst["kin"] = max(worst["kin"], np.abs(kin[b] - kin_o[b]).max()); worst["angle"] = max(worst["angle"], abs(ctr["terrain_angle"][b] - ang))
            if warm == 2:
                grf_o, it_o, stt_o = _oracle_update_ticks(oracle, pr, st, dict(x0=x0, xref=xref, R=R, foot=foot_abs, contact=ct_o), carries)
                ref = dict(grf=grf_o, iters=it_o, status=stt_o)
                # Hand the ENGINE's workspace of this tick to the oracle, as O["tl"] is handed over below: every tick of every robot is then ONE update-path step of both
                # sides from one state.  Chained apart, the two drift: each solve starts from iterates scaled for an unrelated QP (the sensors are redrawn every tick),
                # which makes the sequence a chaotic map (test_ten_thousand_warm_started_ticks_batch_1) -- measured here without the hand-over: 1e-11 N at tick 0,
                # 2e-6 N at tick 14, 1.3e-5 N at tick 22, 0.5 N at tick 124, the iteration counts equal throughout.  What is handed over is held to the oracle's own
                # carry first: x is the full-horizon force vector (the quantity TOL_FORCE_N bounds), z its friction-cone rows f_xy +- mu f_z.
                ex, ey, erho = eng.get_warm_start(n); ez = eng.get_workspace_z(n); eD, eE, ec = eng.get_workspace_scaling(n)
                for b in range(n):
                    x_o = carries[b][2:2 + 12 * h] * eD[b]; z_o = carries[b][2 + 12 * h:2 + 32 * h] / eE[b]
                    dx, dz = np.abs(ex[b] - x_o).max(), np.abs(ez[b] - z_o).max()
                    assert dx <= TOL_FORCE_N and dz <= (1.0 + P["mu"]) * TOL_FORCE_N, (t, b, dx, dz)
                    worst["carry_x"] = max(worst["carry_x"], dx); worst["carry_rho"] = max(worst["carry_rho"], abs(erho[b] / carries[b][1] - 1.0))
                    Pq, gq, _, lq, uq, _ = oracle.mpc_form(pr, x0[b], xref[b], R[b], foot_abs[b], ct_o[b])
                    carries[b] = oracle.carry_from_workspace(h, ex[b], ey[b], ez[b], erho[b], eD[b], eE[b], ec[b], Pq, gq, lq, uq)
            else:
                ref = oracle.mpc_solve_batch(pr, st, x0, xref, R, foot_abs, ct_o)
            try:
                worst["grf"] = max(worst["grf"], compare(sol, ref)["dgrf"])
            except AssertionError as e:
                raise AssertionError(f"tick {t}: {e}; iterations {sol['iters'].tolist()} vs {ref['iters'].tolist()}") from e
            for b in range(n):
                O["tau"][b] = oracle.joint_torques(1, ct_o[b], Jb[b], ref["grf"][b], kin_o[b], km, tg[b], O["tau"][b])
            d_tau = np.abs(G["tau"] - O["tau"]).max()
            assert d_tau < 1e-5, (t, d_tau)
            worst["tau"] = max(worst["tau"], d_tau)
            patterns |= {tuple(c) for c in ct_o.tolist()}
            O["tl"][:] = G["tl"]  # the curve's ulp differences must not accumulate into the comparison (see test_swing_legs_N4a_sequence)
    print(f"warm {warm} n {n}: {early} early contacts, {len(patterns)} contact patterns, worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # a leg spends a quarter of its cycle behind 180 and two of the four forces exceed 30 N, so nearly all of that quarter is early contact (~0.9 per robot and tick): half of it
    assert early >= n * ticks // 2, early
    assert len(patterns) >= 8, patterns   # the MPC has met the contact-pattern changes of the cycle


# name -> (contact_schedule, foot_preview, ticks_per_step, footholds) of the one-call tick; None = a1mpc_control_tick_device
TICK_VARIANTS = dict(plain=None, schedule=(1, 0, 1, False), schedule_feet=(1, 2, 3, False), footholds=(1, 1, 2, True))
ONE_CALL_CASES = [(v, n, warm, 165) for v in TICK_VARIANTS for n, warm in ((64, 2), (300, 1))] + [("plain", 2500, 1, 12)]


@pytest.mark.parametrize("variant,n,warm,ticks", ONE_CALL_CASES)
def test_whole_cycle_one_call_tick_matches_the_chain(pkg, scen, variant, n, warm, ticks):
    """a1mpc_control_tick_device / _preview_device / _preview_footholds_device on one handle against gpu_common.TickChain (the *_device entries chained by hand) on a second one
    for 165 ticks -- a full cycle of the slowest leg -- of the staggered fleet, with a movement_mode timetable (walk, stand a few ticks, walk again) and forces on the 30 N
    and 50 N thresholds: legs touch down, wrap and keep early contacts from tick to tick, the warm-started MPC meets every change of contact pattern, and the fused plan /
    swing kernel latches foot_pos_start from a register-carried counter that is exactly 120.  (64, 2): latency kernel, update path; (300, 1): fused kernel; (2500, 1), 12
    ticks: the cost-ordered fused kernel above 2048 robots, where the staggered fleet changes contacts on every tick.  On every tick: every output and carried state of the
    two worlds equal (NaN-aware), status 1, torques_fused as include/a1mpc.h documents it; the INDEPENDENT anchor is numpy's fmod(gc + spd, 240) / <= 120 loop with the reset
    values where the timetable says stand, for the world's counters, planned contacts and start latch and, run forward t * ticks_per_step ticks, for steps >= 1 of the schedule."""
    import torch
    rng = np.random.default_rng(4242 + n)
    h = 10
    cfg = _cfg(pkg, scen, h, warm_start=warm)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E = pkg.engine
    gc0, spd = gait_cycle_fleet(n)
    mm_table = stand_timetable(n, ticks)
    assert (mm_table == 0).any(axis=0).mean() >= 0.5 and (mm_table[0] == 1).all() and (mm_table[-1] == 1).all()
    assert_thresholds_are_hit(gc0, spd, mm_table)
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e7:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        assert prm.gait.counter_per_gait == PER_GAIT and prm.gait.counter_per_swing == PER_SWING
        st = torch.cuda.Stream(device=dev)
        pv = footholds = None
        if TICK_VARIANTS[variant] is not None:
            sched, feet, tps, footholds = TICK_VARIANTS[variant]
            pv = e1.preview_config(contact_schedule=sched, foot_preview=feet, ticks_per_step=tps)
        chain = TickChain(e7, prm, n, st, preview=pv, footholds=bool(footholds))
        w1, w7 = tick_world(n, dev, gc0), tick_world(n, dev, gc0)
        gc_np = gc0.copy(); start_prev = np.zeros((n, 12)); fused_seen = []; early = 0; touchdowns = 0; patterns = set()
        for t in range(ticks):
            mm = mm_table[t]
            inp = {k: T(v) for k, v in tick_inputs_timetable(scen, rng, n, mm, spd).items()}
            # ---- one call
            bf = tick_buffers(E, inp, w1)
            if pv is None:
                e1.control_tick_device(prm, bf, n, stream=st.cuda_stream)
            elif footholds:
                e1.control_tick_preview_footholds_device(prm, pv, bf, n, stream=st.cuda_stream)
            else:
                e1.control_tick_preview_device(prm, pv, bf, n, stream=st.cuda_stream)
            fused_seen.append(e1.last_control_tick_ms()[1])
            assert e1.last_warm_start_mode() == warm
            # ---- the chain
            chain.tick(inp, w7)
            st.synchronize()
            assert e7.last_warm_start_mode() == warm
            assert_worlds_equal(t, w1, w7)
            assert (w1["i32"]["status"].cpu().numpy() == 1).all(), (t, np.flatnonzero(w1["i32"]["status"].cpu().numpy() != 1)[:8])
            # ---- the anchor: counters and planned contacts are the numpy loop
            gc_np, pc_np = gait_loop(gc_np, spd, mm)
            pc1 = w1["u8"]["plan_contacts"].cpu().numpy(); ct1 = w1["u8"]["contacts"].cpu().numpy()
            assert np.array_equal(w1["state"]["gait_counter"].cpu().numpy(), gc_np) and np.array_equal(pc1, pc_np), t
            assert (ct1 >= pc1).all()
            # ... and so is the swing leg's start latch: foot_pos_start <- foot_pos_cur up to and including 120, kept after that (S/A1RobotControl.cpp:227-236)
            start1 = w1["state"]["foot_pos_start"].cpu().numpy(); stance = np.repeat(gc_np <= PER_SWING, 3, axis=1)
            assert np.array_equal(start1[stance], w1["outs"]["foot_pos_cur"].cpu().numpy()[stance]) and np.array_equal(start1[~stance], start_prev[~stance]), t
            start_prev = start1
            if t > 0:
                touchdowns += int(((pc1 == 1) & (pc_prev == 0)).sum())
            pc_prev = pc1
            early += int(((ct1 == 1) & (pc1 == 0)).sum()); patterns |= {tuple(c) for c in ct1.tolist()}
            if chain.sched_d is not None:
                sd = chain.sched_d.cpu().numpy().reshape(n, h, 4)
                assert np.array_equal(sd[:, 0], ct1), t
                g = gc_np
                for step in range(1, h):
                    for _ in range(pv.ticks_per_step):
                        g = np.fmod(g + spd, PER_GAIT)
                    assert np.array_equal(sd[:, step], np.where(mm[:, None] == 1, g <= PER_SWING, True).astype(np.uint8)), (t, step)
        assert np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1
        if pv is not None and pv.foot_preview:
            assert fused_seen == [False] * ticks, fused_seen      # per-step feet solve on the general kernels: the torques are a launch of their own
        else:
            assert fused_seen == ([True] * ticks if n <= 2048 else [False] + [True] * (ticks - 1)), fused_seen
        print(f"{variant} n {n} warm {warm}: {touchdowns} touchdowns, {early} early contacts, {len(patterns)} contact patterns")
        assert touchdowns >= n * ticks // 160 and early >= n * ticks // 8 and len(patterns) >= 8, (touchdowns, early, patterns)
