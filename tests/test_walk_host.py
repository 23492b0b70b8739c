"""The walking plant's kernels on the CPU: the product's kernel text compiled for the host (tests/emu/walk_step_host.py, walk_sensors_host.py: 64 host threads in lock
step are one wavefront) against the elementwise numpy restatements of tests/walk_ref.py; the reductions to the plant step and the sensor synthesis; the geometry of the
swing and of the ground; and the trot of tests/walk_loop.py on the CPU, the yardstick of the GPU loop of tests/test_gpu_walk.py."""
import itertools

import numpy as np
import pytest

import plant_host
import plant_ref as PR
import sensor_loop as SL
import sensor_synthesis_host as synth_host
import sensor_synthesis_ref as SR
import walk_loop as WL
import walk_ref as WR
import walk_sensors_host as sensors_host
import walk_step_host as host

SIZES = (1, 15, 16, 17, 65)
_SHARED = {}


def _walkers(scen):
    """65 random robots with yaw frames and swing targets (all 16 contact patterns), with three extra words per stride: computed once, never changed"""
    if "walk" not in _SHARED:
        rng = np.random.default_rng(7100)
        sc = WR.random_walkers(scen, rng, max(SIZES))
        sc["wide"] = np.concatenate([sc["state"], rng.normal(0, 1, (max(SIZES), 10))], 1)
        for v in sc.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SHARED["walk"] = sc
    return _SHARED["walk"]


def _step_args(sc, n, stride=12, ext=True):
    return (sc["params"], sc["wide"][:n, :stride], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n], sc["target"][:n], sc["ext"][:n] if ext else None)


def _same_step(out, ref, n):
    so, Ro, fo, vo = out
    assert not np.isnan(so[:n, :12]).any() and not np.isnan(Ro[:n]).any() and not np.isnan(fo[:n]).any() and not np.isnan(vo[:n]).any()
    assert np.isnan(so[n:]).all() and np.isnan(Ro[n:]).all() and np.isnan(fo[n:]).all() and np.isnan(vo[n:]).all() and np.isnan(so[:n, 12:]).all()
    assert PR.bits_equal(so[:n, 3:12], ref[0][:, 3:12]) and PR.bits_equal(Ro[:n], ref[1]) and PR.bits_equal(fo[:n], ref[2]) and PR.bits_equal(vo[:n], ref[3])
    worst = float(np.abs(so[:n, :3] - ref[0][:, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("stride", [12, 13, 22])
@pytest.mark.parametrize("n", SIZES)
def test_step_kernel_text_on_the_host_equals_the_restatement_bit_for_bit(scen, n, stride):
    """a lone robot, either side of a wavefront edge, several workgroups with a partly filled last one; the three row widths; all 16 contact patterns from 16 robots on;
    sub-steps 1 and 3; swing_track 0 / 0.5 / 1; the ground off and on; the wrench null and given.  pos, R, v, omega, the feet and foot_vel_body bit for bit, the angles
    within 1e-12; NaN-poisoned rows beyond n and words [12:stride) stay NaN"""
    sc = _walkers(scen)
    if n >= 16:
        assert len({tuple(c) for c in sc["contacts"][:n]}) == 16
    worst = 0.0
    for substeps, track, ground, ext in itertools.product((1, 3), (0.0, 0.5, 1.0), (0, 1), (False, True)):
        kw = dict(dt=0.0025, substeps=substeps, swing_track=track, flat_ground=ground, ground_z=0.05)
        a = _step_args(sc, n, stride, ext)
        ref = WR.step(*a, **kw)
        worst = max(worst, _same_step(host.run(*a, rows=n + 5, **kw), ref, n))
        if track and n >= 16:
            swing = np.repeat(sc["contacts"][:n] == 0, 3, axis=1)
            assert (np.abs(ref[3][swing]) > 1e-3).any() and not ref[3][~swing].any()
    print(f"n {n} stride {stride}: 24 configurations bit for bit; angles within {worst:.1e}")


def test_the_inputs_reach_both_sides_of_the_plane(scen):
    """with the ground at 0.05 the random robots have swing feet below the plane (lifted), above it (left alone) and stance feet on either side (put on it)"""
    sc = _walkers(scen)
    a = _step_args(sc, 65)
    off = WR.step(*a, flat_ground=0)
    hz = off[2].reshape(65, 4, 3)[:, :, 2] + off[0][:, 5:6] - 0.05
    swing = sc["contacts"] == 0
    assert (hz[swing] < 0).sum() >= 10 and (hz[swing] > 0).sum() >= 10 and (hz[~swing] < 0).sum() >= 10 and (hz[~swing] > 0).sum() >= 10


@pytest.mark.parametrize("substeps", [1, 4])
def test_the_walk_step_reduces_to_the_plant_step(scen, substeps):
    """swing_track = 0 and flat_ground = 0, R_z and foot_target NULL: state, R and the feet are the plant step's kernel text's and plant_ref.step's bit for bit, in and
    out of place; foot_vel_body is all +0 bits"""
    sc = _walkers(scen)
    n = 65
    P, st = sc["params"], sc["wide"][:, :13]
    a = (sc["R"], sc["foot"], sc["grf"], sc["contacts"])
    w = host.run(P, st, *a, None, None, sc["ext"], 0.0025, substeps, swing_track=0.0, flat_ground=0)
    p = plant_host.run(P, st, *a, sc["ext"], 0.0025, substeps)
    r = PR.step(P, st, *a, sc["ext"], 0.0025, substeps)
    assert PR.bits_equal(w[0], p[0]) and PR.bits_equal(w[1], p[1]) and PR.bits_equal(w[2], p[2])
    assert PR.bits_equal(w[0][:, 3:12], r[0][:, 3:12]) and PR.bits_equal(w[1], r[1]) and PR.bits_equal(w[2], r[2])
    assert np.array_equal(w[3].view(np.uint64), np.zeros((n, 12), np.uint64))
    wi = host.run(P, st, *a, None, None, sc["ext"], 0.0025, substeps, swing_track=0.0, flat_ground=0, in_place=True)
    assert PR.bits_equal(wi[0][:, :12], p[0][:, :12]) and np.array_equal(wi[0][:, 12:], st[:, 12:]) and PR.bits_equal(wi[1], p[1]) and PR.bits_equal(wi[2], p[2])
    moved = host.run(P, st, *a, sc["Rz"], sc["target"], sc["ext"], 0.0025, substeps, swing_track=1.0, flat_ground=0)
    assert not PR.bits_equal(moved[2], p[2]) and PR.bits_equal(moved[0], p[0]) and PR.bits_equal(moved[1], p[1])   # (massless legs: the swing moves the feet alone)


def test_step_structural_bit_equalities(scen):
    """in place == out of place; robot i alone == robot i of the batch; a NaN target on a stance leg and a NaN force on a swing leg change no bit; a NaN pos stays with
    its robot (pos, and with the ground on the z of its feet)"""
    sc = _walkers(scen)
    n = 37
    kw = dict(dt=0.0025, substeps=2, swing_track=1.0, flat_ground=1, ground_z=0.05)
    a = _step_args(sc, n, 22)
    base = host.run(*a, **kw)
    inp = host.run(*a, in_place=True, **kw)
    assert all(PR.bits_equal(x[:, :12], y[:, :12]) for x, y in zip(inp, base)) and np.array_equal(inp[0][:, 12:], sc["wide"][:n, 12:])
    for i in (0, 15, 16, 36):
        one = host.run(*[None if v is None else (v if isinstance(v, dict) else v[i:i + 1]) for v in a], **kw)
        assert all(PR.bits_equal(x[:, :12], y[i:i + 1, :12]) for x, y in zip(one, base)), i
    target, grf = sc["target"][:n].copy(), sc["grf"][:n].copy()
    for i, l in np.argwhere(sc["contacts"][:n] != 0):
        target[i, 3 * l + (i + l) % 3] = np.nan
    for i, l in np.argwhere(sc["contacts"][:n] == 0):
        grf[i, 3 * l + (i + l) % 3] = np.nan
    b = list(a); b[4] = grf; b[7] = target
    nan = host.run(*b, **kw)
    assert all(PR.bits_equal(x[:, :12], y[:, :12]) for x, y in zip(nan, base))
    st = sc["wide"][:n].copy(); st[20, 5] = np.nan
    b = list(a); b[1] = st
    bad = host.run(*b, **kw)
    keep = np.arange(n) != 20
    assert all(PR.bits_equal(x[keep, :12], y[keep, :12]) for x, y in zip(bad, base))
    assert np.isnan(bad[0][20, 5]) and np.isfinite(np.delete(bad[0][20, :12], 5)).all() and PR.bits_equal(bad[1][20], base[1][20]) and PR.bits_equal(bad[3][20], base[3][20])
    stance = sc["contacts"][20] != 0   # gz is a NaN: a stance foot is put there; `r_z < gz` is false, so a swing foot keeps its own finite z
    assert stance.any() and not stance.all() and np.isnan(bad[2][20, 2::3][stance]).all() and np.isfinite(bad[2][20, 2::3][~stance]).all()
    assert PR.bits_equal(np.delete(bad[2][20], [2, 5, 8, 11]), np.delete(base[2][20], [2, 5, 8, 11]))


def test_swing_geometry(scen):
    """swing_track = 1, one sub-step: a swing foot ends at R' (R^T R_z y), R the polished attitude, within 1e-15 max|r| (the other side in 80 bits); swing_track = 0.5
    on a body that does not turn: the distance to a fixed target halves per call within 1e-12; foot_vel_body is the body-frame move over dt"""
    sc = _walkers(scen)
    n = 65
    a = _step_args(sc, n)
    so, Ro, fo, vo = host.run(*a, swing_track=1.0, flat_ground=0)
    ld = np.longdouble
    Rp = np.stack(PR.polish([sc["R"][:, k] for k in range(9)]), 1).astype(ld).reshape(n, 3, 3)
    body = lambda R, r: np.stack([sum(R[:, j, i] * r[:, l, j] for j in range(3)) for l in range(4) for i in range(3)], 1).reshape(n, 4, 3)     # R^T r
    world = lambda R, p: np.stack([sum(R[:, i, j] * p[:, l, j] for j in range(3)) for l in range(4) for i in range(3)], 1).reshape(n, 4, 3)    # R p
    pt = body(Rp, world(sc["Rz"].astype(ld).reshape(n, 3, 3), sc["target"].astype(ld).reshape(n, 4, 3)))
    want = world(Ro.astype(ld).reshape(n, 3, 3), pt)
    swing = sc["contacts"] == 0
    err = float(np.abs(fo.reshape(n, 4, 3).astype(ld) - want)[swing].max()); scale = float(np.abs(fo).max())
    print(f"swing feet against R' (R^T R_z y): {err:.1e}, max|r| {scale:.2f}")
    assert err <= 1e-15 * scale
    p0 = body(Rp, sc["foot"].astype(ld).reshape(n, 4, 3))
    assert float(np.abs(vo.reshape(n, 4, 3) * 0.0025 - (pt - p0))[swing].max()) <= 1e-15 and not vo.reshape(n, 4, 3)[~swing].any()
    # half way per call, towards a target fixed in the body: omega = 0 and no leg in stance, so R does not move (the body falls, which the body frame does not see)
    st = sc["state"].copy(); st[:, 6:9] = 0.0
    ct = np.zeros((n, 4), np.uint8)
    R, foot = sc["R"], sc["foot"]
    dist = []
    for _ in range(6):
        Rl = R.astype(ld).reshape(n, 3, 3)
        dist.append(np.linalg.norm((body(Rl, world(sc["Rz"].astype(ld).reshape(n, 3, 3), sc["target"].astype(ld).reshape(n, 4, 3))) -
                                    body(Rl, foot.astype(ld).reshape(n, 4, 3))).astype(np.float64), axis=2))
        st, R, foot, _ = host.run(sc["params"], st, R, foot, sc["grf"], ct, sc["Rz"], sc["target"], None, swing_track=0.5, flat_ground=0)
    assert dist[0].min() > 1e-3 and all(np.abs(dist[k + 1] - 0.5 * dist[k]).max() <= 1e-12 for k in range(5))


def test_ground_geometry(scen):
    """the ground on: stance feet satisfy r_z + pos_z == ground_z within one ulp of pos_z; no swing foot is below the plane; a swing foot above the plane is untouched,
    bit for bit, and so are x and y of every foot and the body"""
    sc = _walkers(scen)
    n = 65
    a = _step_args(sc, n)
    gz = 0.05
    off = host.run(*a, substeps=3, swing_track=0.5, flat_ground=0)
    on = host.run(*a, substeps=3, swing_track=0.5, flat_ground=1, ground_z=gz)
    assert PR.bits_equal(on[0], off[0]) and PR.bits_equal(on[1], off[1]) and PR.bits_equal(on[3], off[3])
    f_on, f_off, pz = on[2].reshape(n, 4, 3), off[2].reshape(n, 4, 3), on[0][:, 5:6]
    assert PR.bits_equal(f_on[:, :, :2], f_off[:, :, :2])
    stance = sc["contacts"] != 0
    ulp = np.spacing(np.abs(pz))
    assert (np.abs((f_on[:, :, 2] + pz) - gz) <= ulp)[stance].all()
    assert ((f_on[:, :, 2] + pz) - gz >= -ulp)[~stance].all()
    above = ~stance & (f_off[:, :, 2] >= gz - pz)
    lifted = ~stance & ~above
    assert above.sum() >= 10 and lifted.sum() >= 10
    assert PR.bits_equal(f_on[:, :, 2][above], f_off[:, :, 2][above]) and PR.bits_equal(f_on[:, :, 2][lifted], np.broadcast_to(gz - pz, (n, 4))[lifted])


# ---- the sensors
def _sensor_cases(scen):
    """sensor_synthesis_ref.random_robots (65, all four quaternion branches, all 16 contact patterns, reachable feet) with a commanded velocity on every leg, and the
    restatement in float64 and 80 bits, with and without the wrench: computed once, never changed"""
    if "sens" not in _SHARED:
        rng = np.random.default_rng(7200)
        sc = SR.random_robots(scen, rng, max(SIZES), rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        sc["vel"] = rng.normal(0, 1.0, (max(SIZES), 12))
        refs = {}
        for ext in (False, True):
            for dt in (np.float64, np.longdouble):
                r = WR.sensors(sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["vel"], sc["ext"] if ext else None, rho_opt=sc["rho_opt"], dtype=dt)
                for v in r.values():
                    v.setflags(write=False)
                refs[(ext, dt)] = r
        _SHARED["sens"] = (sc, refs)
    return _SHARED["sens"]


@pytest.mark.parametrize("stride", [12, 13, 22])
@pytest.mark.parametrize("with_ext", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sensors_kernel_text_on_the_host_equals_the_restatement(scen, n, stride, with_ext):
    """the cases of tests/test_sensor_synthesis_host.py with a commanded velocity on every leg: BITS bit for bit (foot_vel_rel among them), NOISY within 4 E; rows beyond n
    stay poisoned"""
    sc, refs = _sensor_cases(scen)
    r64, r80 = refs[(with_ext, np.float64)], refs[(with_ext, np.longdouble)]
    state = np.concatenate([sc["state"], np.random.default_rng(stride).normal(0, 1, (max(SIZES), stride - 12))], 1)
    out = sensors_host.run(sc["mass"], state[:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["vel"][:n], sc["ext"][:n] if with_ext else None,
                           rho_opt=sc["rho_opt"], rows=n + 3)
    figs = SR.assert_is_ref(out, r64, r80, n, (n, stride, with_ext))
    assert all((v[n:] == 0xFF).all() if k == "reach" else np.isnan(v[n:]).all() for k, v in out.items())
    assert not any(np.isnan(v[:n]).any() for k, v in out.items() if k != "reach")
    swing = np.repeat(sc["contacts"][:n] == 0, 3, axis=1)
    assert SR.bits_equal(out["foot_vel_rel"][:n][swing], sc["vel"][:n][swing])
    print(f"n {n} stride {stride} wrench {with_ext}: " + ", ".join(f"{k} {e:.1e} (E {E:.1e})" for k, (e, E) in figs.items()))


def test_the_walk_sensors_reduce_to_the_synthesis(scen):
    """foot_vel_body NULL, or all +0: every output is the synthesis kernel text's bit for bit (the same host libm on both sides); a NaN velocity on a stance leg changes
    no bit; the optional outputs NULL change nothing else"""
    sc, _ = _sensor_cases(scen)
    n = 65
    a = (sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"])
    syn = synth_host.run(*a, sc["ext"], rho_opt=sc["rho_opt"])
    same = lambda x, y: all(SR.bits_equal(x[k], y[k]) for k in SR.OUTPUTS if k != "reach" and x[k] is not None) and np.array_equal(x["reach"], y["reach"])
    assert same(sensors_host.run(*a, None, sc["ext"], rho_opt=sc["rho_opt"]), syn)
    assert same(sensors_host.run(*a, np.zeros((n, 12)), sc["ext"], rho_opt=sc["rho_opt"]), syn)
    full = sensors_host.run(*a, sc["vel"], sc["ext"], rho_opt=sc["rho_opt"])
    assert not same(full, syn)
    vel = sc["vel"].copy()
    vel[np.repeat(sc["contacts"] != 0, 3, axis=1)] = np.nan
    assert same(sensors_host.run(*a, vel, sc["ext"], rho_opt=sc["rho_opt"]), full)
    lean = sensors_host.run(*a, sc["vel"], sc["ext"], rho_opt=sc["rho_opt"], want_foot_rel=False)
    assert lean["foot_pos_rel"] is None and lean["foot_vel_rel"] is None and same(lean, full)


def test_joint_rates_give_the_commanded_velocity_back(oracle, scen):
    """on the swing legs J(q) joint_vel == foot_vel_body within 1e-13 (rates of a few m/s); the oracle's leg stage (a1mpc_leg_state_batch's arithmetic) returns
    foot_vel_body from the synthesised angles and rates within 4 E of the restated round trip's 80-bit evaluation; a reach flag still zeroes the rates"""
    sc, refs = _sensor_cases(scen)
    n = max(SIZES)
    out = sensors_host.run(sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["vel"], None, rho_opt=sc["rho_opt"])
    swing = np.repeat(sc["contacts"] == 0, 3, axis=1)
    trip = {}
    for dt in (np.float64, np.longdouble):
        r = refs[(False, dt)]; cols = []
        for l in range(4):
            _, J = SR.forward_leg(SR.leg_geometry(SR.A1_RHO_FIX, sc["rho_opt"], l, dt), [r["joint_pos"][:, 3 * l + k] for k in range(3)])
            qd = [r["joint_vel"][:, 3 * l + k] for k in range(3)]
            cols += [(J[i] * qd[0] + J[3 + i] * qd[1]) + J[6 + i] * qd[2] for i in range(3)]
        trip[dt] = np.stack(cols, 1)
    assert np.abs(trip[np.longdouble] - sc["vel"])[swing].max() <= 1e-13
    Jq = np.zeros((n, 12))
    for l in range(4):
        _, J = SR.forward_leg(SR.leg_geometry(SR.A1_RHO_FIX, sc["rho_opt"], l), [out["joint_pos"][:, 3 * l + k] for k in range(3)])
        for i in range(3):
            Jq[:, 3 * l + i] = (J[i] * out["joint_vel"][:, 3 * l] + J[3 + i] * out["joint_vel"][:, 3 * l + 1]) + J[6 + i] * out["joint_vel"][:, 3 * l + 2]
    assert np.abs(Jq - sc["vel"])[swing].max() <= 1e-13
    leg = np.stack([oracle.leg_state(out["joint_pos"][b], out["joint_vel"][b], sc["R"][b], np.zeros(3), np.zeros(3), rho_opt=sc["rho_opt"])["foot_vel_rel"] for b in range(n)])
    E = float(np.abs(trip[np.float64].astype(np.longdouble) - trip[np.longdouble])[swing].max())
    err = float(np.abs(leg.astype(np.longdouble) - trip[np.longdouble])[swing].max())
    print(f"the leg stage's foot_vel_rel on the swing legs against the commanded velocity: {err:.1e} (E {E:.1e})")
    assert err <= SR.FACTOR * E
    # leg 0 out of reach: rates +0 whatever the command
    table = SR.unreachable_feet()
    m = len(table)
    u = SR.random_robots(scen, np.random.default_rng(7300), m, rho_opt=SR.UNREACHABLE_OPT)
    foot = SR.forward_feet(SR.A1_RHO_FIX, SR.UNREACHABLE_OPT, u["q"]); foot[:, 0:3] = np.array([p for p, _ in table])
    o = sensors_host.run(u["mass"], u["state"], np.tile(np.eye(3).reshape(9), (m, 1)), foot, u["grf"], np.zeros((m, 4), np.uint8), np.ones((m, 12)), None,
                         rho_opt=SR.UNREACHABLE_OPT)
    assert (o["reach"][:, 0] != 0).all() and not o["reach"][:, 1:].any()
    assert np.array_equal(o["joint_vel"][:, 0:3].view(np.uint64), np.zeros((m, 3), np.uint64)) and (np.abs(o["joint_vel"][:, 3:]) > 1e-3).any(axis=1).all()
    assert np.array_equal(o["foot_vel_rel"], np.ones((m, 12)))


# ---- the trot
def run_trot(loop, n):
    """the schedule of walk_loop on `loop`: the per-tick conditions asserted on the way -> (history over the WALK ticks, figures)"""
    hist = dict(contacts=[], foot=[], state=[], R=[])
    herr, tilt, lo, hi = 0.0, 0.0, np.inf, -np.inf
    for t, (stepped, cmd, toggle) in enumerate(WL.schedule(n)):
        loop.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
        if not stepped:
            continue
        finite = all(np.isfinite(np.asarray(v, float)).all() for v in loop.sensors.values()) and np.isfinite(loop.grf).all() and np.isfinite(loop.x).all()
        bad = SL.conditions_hold(loop.x, loop.sensors["reach"], loop.status, finite)
        assert not bad, (t, bad)
        e = float(np.abs(loop.pos[:, 2] - loop.x[:, 5]).max())
        if loop.walk["flat_ground"]:
            assert e <= WL.HEIGHT_ESTIMATE, (t, e)
        herr, tilt, lo, hi = max(herr, e), max(tilt, float(np.abs(loop.x[:, :2]).max())), min(lo, float(loop.x[:, 5].min())), max(hi, float(loop.x[:, 5].max()))
        if t >= WL.PRIME + WL.STAND:
            for k, v in (("contacts", loop.ct), ("foot", loop.foot), ("state", loop.x), ("R", loop.R)):
                hist[k].append(v.copy())
    return {k: np.stack(v) for k, v in hist.items()}, dict(height_estimate=herr, tilt=tilt, height=(lo, hi))


def test_trot_on_the_cpu(oracle, scen):
    """4 perturbed standing robots (seed 5), IMU window 1, the default gait, swing_track 1, the ground on at 0: 10 priming ticks, 100 standing, 360 walking at 0.2 m/s.
    On every closed tick sensor_loop.conditions_hold is empty and the EKF's height is within 1e-2 of the plant's (prototype: 4.0e-3); over the walk the contacts are the
    planned diagonal pairs, every touchdown is on the plane within 1e-12, every leg's swing rises 0.10 m at least (prototype: 0.13) and no foot is below the plane; the
    mean velocity along the heading over the last 120 ticks is in [0.15, 0.25]"""
    n = 4
    sc = SL.perturbed_standing_robots(scen)
    hist, figs = run_trot(WL.WalkLoop(oracle, scen, sc, n), n)
    bad, walk = WL.walk_conditions(hist, n)
    print(f"trot on the CPU, {WL.WALK} ticks: height estimate off by {figs['height_estimate']:.1e} at most, |roll, pitch| <= {figs['tilt']:.3f}, height "
          f"{figs['height'][0]:.3f} .. {figs['height'][1]:.3f}; {walk['touchdowns']} touchdowns at z {walk['touchdown_z'][0]:.1e} .. {walk['touchdown_z'][1]:.1e}, swings rise "
          f"{walk['swing_rise']:.3f} at least, heading speed {walk['heading_speed'].min():.3f} .. {walk['heading_speed'].max():.3f}")
    assert not bad, bad
    assert walk["touchdowns"] == 12 * n and max(abs(z) for z in walk["touchdown_z"]) <= 1e-12 and walk["below_plane"] >= -1e-12
    assert walk["swing_rise"] >= WL.SWING_RISE
    assert (walk["heading_speed"] >= WL.HEADING_SPEED[0]).all() and (walk["heading_speed"] <= WL.HEADING_SPEED[1]).all()


def test_trot_without_the_ground_still_walks(oracle, scen):
    """the same schedule with flat_ground = 0: conditions_hold stays empty on every tick; the touchdown scatter is printed, nothing else is asserted"""
    n = 4
    sc = SL.perturbed_standing_robots(scen)
    hist, figs = run_trot(WL.WalkLoop(oracle, scen, sc, n, flat_ground=0), n)
    _, walk = WL.walk_conditions(hist, n)
    print(f"trot without the ground: touchdowns at z {walk['touchdown_z'][0] * 1e3:+.1f} .. {walk['touchdown_z'][1] * 1e3:+.1f} mm, height estimate off by "
          f"{figs['height_estimate'] * 1e3:.1f} mm at most, height {figs['height'][0]:.3f} .. {figs['height'][1]:.3f}")
