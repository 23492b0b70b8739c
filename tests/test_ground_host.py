"""Sloped ground and sensed touchdowns on the CPU: the product's kernel text compiled for the host (tests/emu/walk_step_ground_host.py, walk_sensors_touch_host.py: 64
host threads in lock step are one wavefront) against the elementwise numpy restatements of tests/ground_ref.py; the reductions to the walk step and the walk sensors;
the geometry of the planes; isolation; and the closed loops of tests/ground_loop.py -- the reduction to the flat blind trot, the ramps and the touch sensor -- the
yardsticks of the GPU loops of tests/test_gpu_ground.py."""
import itertools

import numpy as np
import pytest

import ground_loop as GL
import ground_ref as GR
import plant_ref as PR
import sensor_loop as SL
import sensor_synthesis_ref as SR
import walk_loop as WL
import walk_ref as WR
import walk_sensors_host
import walk_sensors_touch_host as touch_host
import walk_step_ground_host as host
import walk_step_host

SIZES = (1, 15, 16, 17, 65)
NMAX = max(SIZES)
GROUND_Z = 0.05
_SHARED = {}


def _walkers(scen):
    """65 random walkers (all 16 contact patterns), three extra words per stride and a random plane each, |sx|, |sy| <= 0.3, through the middle of the robot's feet:
    computed once, never changed"""
    if "walk" not in _SHARED:
        rng = np.random.default_rng(8100)
        sc = WR.random_walkers(scen, rng, NMAX)
        # the bodies at standing height above feet 0.3 below them: r_z = fl(hz - pos_z) is off by ulp(r_z) / 2, which the geometry test holds to one ulp of pos_z -- a bound
        # that only means something where |pos_z| is not far below |r_z| (random_walkers draws pos_z from N(0, 1), 6 % of it within 0.075 of zero)
        sc["state"][:, 5] = rng.uniform(0.25, 0.45, NMAX)
        sc["wide"] = np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1)
        sc["ground"] = GR.random_planes(sc, rng, NMAX)
        for v in sc.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SHARED["walk"] = sc
    return _SHARED["walk"]


def _args(sc, n, stride=12, ext=True, ground=True, sl=None):
    sl = slice(0, n) if sl is None else sl
    return (sc["params"], sc["wide"][sl, :stride], sc["R"][sl], sc["foot"][sl], sc["grf"][sl], sc["contacts"][sl], sc["Rz"][sl], sc["target"][sl],
            sc["ground"][sl] if ground else None, sc["ext"][sl] if ext else None)


def _same_step(out, ref, n):
    so, Ro, fo, vo, to = out
    assert not np.isnan(so[:n, :12]).any() and not np.isnan(Ro[:n]).any() and not np.isnan(fo[:n]).any() and not np.isnan(vo[:n]).any()
    assert np.isnan(so[n:]).all() and np.isnan(Ro[n:]).all() and np.isnan(fo[n:]).all() and np.isnan(vo[n:]).all() and np.isnan(so[:n, 12:]).all() and (to[n:] == 0xFF).all()
    assert PR.bits_equal(so[:n, 3:12], ref[0][:, 3:12]) and PR.bits_equal(Ro[:n], ref[1]) and PR.bits_equal(fo[:n], ref[2]) and PR.bits_equal(vo[:n], ref[3])
    assert np.array_equal(to[:n], ref[4])
    worst = float(np.abs(so[:n, :3] - ref[0][:, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("stride", [12, 13, 22])
@pytest.mark.parametrize("n", SIZES)
def test_step_kernel_text_on_the_host_equals_the_restatement_bit_for_bit(scen, n, stride):
    """a lone robot, either side of a wavefront edge, several workgroups with a partly filled last one; the three row widths; all 16 contact patterns from 16 robots on;
    sub-steps 1 (no wrench) and 3 (with one); swing_track 0 / 0.5 / 1; a random plane per robot, cfg's flat plane, no ground.  pos, R, v, omega, the feet, foot_vel_body
    and touch bit for bit, the angles within the walk tests' bar; poisoned rows beyond n and words [12:stride) stay poisoned"""
    sc = _walkers(scen)
    if n >= 16:
        assert len({tuple(c) for c in sc["contacts"][:n]}) == 16
    worst = 0.0
    for substeps, track, mode in itertools.product((1, 3), (0.0, 0.5, 1.0), ("planes", "flat", "none")):
        kw = dict(dt=0.0025, substeps=substeps, swing_track=track, flat_ground=1 if mode == "flat" else 0, ground_z=GROUND_Z)
        a = _args(sc, n, stride, ext=substeps == 3, ground=mode == "planes")
        ref = GR.step(*a, **kw)
        worst = max(worst, _same_step(host.run(*a, rows=n + 5, **kw), ref, n))
        if mode == "none":
            assert np.array_equal(ref[4], (sc["contacts"][:n] != 0).astype(np.uint8))
    print(f"n {n} stride {stride}: 18 configurations bit for bit; angles within {worst:.1e}")


def test_the_inputs_reach_both_sides_of_the_planes(scen):
    """the random planes have swing feet below them (lifted, touch 1), above them (left alone, touch 0) and stance feet on either side (put on them)"""
    sc = _walkers(scen)
    off = GR.step(*_args(sc, NMAX, ground=False), flat_ground=0)
    f = off[2].reshape(NMAX, 4, 3)
    h = (f[:, :, 2] + off[0][:, 5:6]) - GR.plane(sc["ground"], off[0][:, 3:4] + f[:, :, 0], off[0][:, 4:5] + f[:, :, 1])
    swing = sc["contacts"] == 0
    assert (h[swing] < 0).sum() >= 10 and (h[swing] > 0).sum() >= 10 and (h[~swing] < 0).sum() >= 10 and (h[~swing] > 0).sum() >= 10
    assert np.abs(sc["ground"][:, 1:]).max() <= 0.3 and (np.abs(sc["ground"][:, 1:]) > 0.2).any()


@pytest.mark.parametrize("substeps", [1, 3])
def test_the_ground_step_reduces_to_the_walk_step(scen, substeps):
    """ground NULL: every output but touch is the walk step's kernel text's bit for bit, with cfg's plane off and on; ground = (ground_z, 0, 0): the walk step's with
    flat_ground = 1, bit for bit, whatever cfg's own plane says (it is not read).  In place as out of place"""
    sc = _walkers(scen)
    P, st = sc["params"], sc["wide"][:, :13]
    a = (sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"])
    same = lambda g, w: all(PR.bits_equal(x, y) for x, y in zip(g[:4], w))
    for track, flat in itertools.product((0.0, 1.0), (0, 1)):
        kw = dict(dt=0.0025, substeps=substeps, swing_track=track, flat_ground=flat, ground_z=GROUND_Z)
        w = walk_step_host.run(P, st, *a, sc["ext"], **kw)
        assert same(host.run(P, st, *a, None, sc["ext"], **kw), w), (track, flat)
    w = walk_step_host.run(P, st, *a, sc["ext"], dt=0.0025, substeps=substeps, swing_track=1.0, flat_ground=1, ground_z=GROUND_Z)
    level = np.tile([GROUND_Z, 0.0, 0.0], (NMAX, 1))
    for flat, gz in ((0, 0.0), (1, 0.7), (1, np.nan)):
        g = host.run(P, st, *a, level, sc["ext"], dt=0.0025, substeps=substeps, swing_track=1.0, flat_ground=flat, ground_z=gz)
        assert same(g, w), (flat, gz)
    gi = host.run(P, st, *a, level, sc["ext"], dt=0.0025, substeps=substeps, swing_track=1.0, in_place=True)
    assert all(PR.bits_equal(x[:, :12], y[:, :12]) for x, y in zip(gi[:3], w[:3])) and np.array_equal(gi[0][:, 12:], st[:, 12:]) and np.array_equal(gi[4], g[4])


def test_ground_geometry(scen):
    """every stance foot satisfies pos_z + r_z == hz(X, Y) within one ulp of pos_z; no swing foot is below its plane; a swing foot above its plane is untouched bit for
    bit, and so are x and y of every foot and the body; touch equals `stance, or lifted`, recomputed from the outputs of the run without a ground"""
    sc = _walkers(scen)
    n = NMAX
    off = host.run(*_args(sc, n, ground=False), substeps=3, swing_track=0.5, flat_ground=0)
    on = host.run(*_args(sc, n), substeps=3, swing_track=0.5)
    assert PR.bits_equal(on[0], off[0]) and PR.bits_equal(on[1], off[1]) and PR.bits_equal(on[3], off[3])
    f_on, f_off, pos = on[2].reshape(n, 4, 3), off[2].reshape(n, 4, 3), on[0][:, 3:6]
    assert PR.bits_equal(f_on[:, :, :2], f_off[:, :, :2])
    ld = np.longdouble
    hz = GR.plane(sc["ground"], pos[:, 0:1] + f_on[:, :, 0], pos[:, 1:2] + f_on[:, :, 1]).astype(ld)   # (hz in doubles, as stated; the sums below in 80 bits)
    gap =((f_on[:, :, 2].astype(ld) + pos[:, 2:3].astype(ld)) - hz).astype(np.float64)
    gap_off = ((f_off[:, :, 2].astype(ld) + pos[:, 2:3].astype(ld)) - hz).astype(np.float64)
    stance = sc["contacts"] != 0
    ulp = np.broadcast_to(np.spacing(np.abs(pos[:, 2:3])), (n, 4))
    assert (np.abs(gap) <= ulp)[stance].all() and (gap >= -ulp)[~stance].all()
    above, below = ~stance & (gap_off > ulp), ~stance & (gap_off < -ulp)
    assert above.sum() >= 10 and below.sum() >= 10 and (above | below | stance).all()
    assert PR.bits_equal(f_on[:, :, 2][above], f_off[:, :, 2][above]) and (np.abs(gap) <= ulp)[below].all()
    assert np.array_equal(on[4], (stance | below).astype(np.uint8)) and np.array_equal(off[4], stance.astype(np.uint8))


def test_step_structure_and_isolation(scen):
    """in place == out of place; robot i alone == robot i of the batch; a ground row that is not finite changes no bit of any other robot, and of its own robot only the
    z of the feet (a NaN plane: the stance feet are put on it, `r_z < NaN` is false so the swing feet keep their z and touch nothing)"""
    sc = _walkers(scen)
    n = 37
    kw = dict(dt=0.0025, substeps=2, swing_track=1.0)
    a = _args(sc, n, 22)
    base = host.run(*a, **kw)
    inp = host.run(*a, in_place=True, **kw)
    assert all(PR.bits_equal(x[:, :12], y[:, :12]) for x, y in zip(inp[:4], base[:4])) and np.array_equal(inp[0][:, 12:], sc["wide"][:n, 12:]) and np.array_equal(inp[4], base[4])
    for i in (0, 15, 16, 36):
        one = host.run(*_args(sc, 1, 22, sl=slice(i, i + 1)), **kw)
        assert all(PR.bits_equal(x[:, :12], y[i:i + 1, :12]) for x, y in zip(one[:4], base[:4])) and np.array_equal(one[4], base[4][i:i + 1]), i
    for col, val in ((0, np.nan), (1, np.inf), (2, np.nan)):
        ground = sc["ground"][:n].copy(); ground[20, col] = val
        b = list(a); b[8] = ground
        bad = host.run(*b, **kw)
        keep = np.arange(n) != 20
        assert all(PR.bits_equal(x[keep, :12], y[keep, :12]) for x, y in zip(bad[:4], base[:4])) and np.array_equal(bad[4][keep], base[4][keep])
        assert PR.bits_equal(bad[0][20, :12], base[0][20, :12]) and PR.bits_equal(bad[1][20], base[1][20]) and PR.bits_equal(bad[3][20], base[3][20])
        assert PR.bits_equal(np.delete(bad[2][20], [2, 5, 8, 11]), np.delete(base[2][20], [2, 5, 8, 11]))
        stance = sc["contacts"][20] != 0
        assert stance.any() and not stance.all() and not np.isfinite(bad[2][20, 2::3][stance]).any()
        if np.isnan(val):
            assert np.isfinite(bad[2][20, 2::3][~stance]).all() and np.array_equal(bad[4][20], stance.astype(np.uint8))


# ---- the sensors
def _sensor_cases(scen):
    """sensor_synthesis_ref.random_robots (65, all four quaternion branches, all 16 contact patterns), a commanded velocity and a random touch byte (0, 1 or 200) on every
    leg, and the restatement in float64 and 80 bits, with and without the wrench: computed once, never changed"""
    if "sens" not in _SHARED:
        rng = np.random.default_rng(8200)
        sc = SR.random_robots(scen, rng, NMAX, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        sc["vel"] = rng.normal(0, 1.0, (NMAX, 12))
        sc["touch"] = rng.choice(np.array([0, 1, 200], np.uint8), (NMAX, 4))
        refs = {}
        for ext in (False, True):
            for dt in (np.float64, np.longdouble):
                r = GR.sensors(sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["vel"], sc["touch"], GL.TOUCH_FORCE, sc["ext"] if ext else None,
                               rho_opt=sc["rho_opt"], dtype=dt)
                for v in r.values():
                    v.setflags(write=False)
                refs[(ext, dt)] = r
        _SHARED["sens"] = (sc, refs)
    return _SHARED["sens"]


@pytest.mark.parametrize("stride", [12, 13, 22])
@pytest.mark.parametrize("with_ext", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sensors_kernel_text_on_the_host_equals_the_restatement(scen, n, stride, with_ext):
    """the cases of tests/test_walk_host.py with a touch byte on every leg and touch_force = 60: BITS bit for bit (foot_force among them), NOISY within 4 E; rows beyond n
    stay poisoned; foot_force on a touched swing leg is touch_force exactly and +0 on an untouched one"""
    sc, refs = _sensor_cases(scen)
    r64, r80 = refs[(with_ext, np.float64)], refs[(with_ext, np.longdouble)]
    state = np.concatenate([sc["state"], np.random.default_rng(stride).normal(0, 1, (NMAX, stride - 12))], 1)
    out = touch_host.run(sc["mass"], state[:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["vel"][:n], sc["touch"][:n], GL.TOUCH_FORCE,
                         sc["ext"][:n] if with_ext else None, rho_opt=sc["rho_opt"], rows=n + 3)
    SR.assert_is_ref(out, r64, r80, n, (n, stride, with_ext))
    assert all((v[n:] == 0xFF).all() if k == "reach" else np.isnan(v[n:]).all() for k, v in out.items())
    assert not any(np.isnan(v[:n]).any() for k, v in out.items() if k != "reach")
    swing, hit = sc["contacts"][:n] == 0, sc["touch"][:n] != 0
    ff = out["foot_force"][:n]
    assert (ff[swing & hit] == GL.TOUCH_FORCE).all() and np.array_equal(ff[swing & ~hit].view(np.uint64), np.zeros((swing & ~hit).sum(), np.uint64))
    if n >= 16:
        assert (swing & hit).any() and (swing & ~hit).any()


def test_the_touch_sensors_reduce_to_the_walk_sensors(scen):
    """touch NULL, or touch_force +0 (or -0): every output is the walk sensors' kernel text's bit for bit; with a force, a stance leg's touch byte changes no bit and
    every output but foot_force is the walk sensors'; the optional outputs NULL change nothing else"""
    sc, _ = _sensor_cases(scen)
    a = (sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["vel"])
    kw = dict(ext=sc["ext"], rho_opt=sc["rho_opt"])
    walk = walk_sensors_host.run(*a, **kw)
    same = lambda x, y, skip=(): all(SR.bits_equal(x[k], y[k]) for k in SR.OUTPUTS if k != "reach" and k not in skip and x[k] is not None) and np.array_equal(x["reach"], y["reach"])
    assert same(touch_host.run(*a, None, GL.TOUCH_FORCE, **kw), walk)
    assert same(touch_host.run(*a, sc["touch"], 0.0, **kw), walk) and same(touch_host.run(*a, sc["touch"], -0.0, **kw), walk)
    full = touch_host.run(*a, sc["touch"], GL.TOUCH_FORCE, **kw)
    assert not same(full, walk) and same(full, walk, skip=("foot_force",))
    stance = sc["contacts"] != 0
    assert SR.bits_equal(full["foot_force"][stance], walk["foot_force"][stance])
    flipped = sc["touch"].copy(); flipped[stance] = np.where(flipped[stance] != 0, 0, 1)
    assert same(touch_host.run(*a, flipped, GL.TOUCH_FORCE, **kw), full)
    lean = touch_host.run(*a, sc["touch"], GL.TOUCH_FORCE, want_foot_rel=False, **kw)
    assert lean["foot_pos_rel"] is None and lean["foot_vel_rel"] is None and same(lean, full)


# ---- the closed loops
def _loops(oracle, scen):
    """the four CPU loops, each run once: reduction (ground 0, force 0), WalkLoop itself, the ramp at GL.RAMP_SLOPE, the touch loop"""
    if "loops" not in _SHARED:
        n = 4
        sc = SL.perturbed_standing_robots(scen)
        out = {}
        out["reduction"] = GL.run(GL.GroundLoop(oracle, scen, sc, n), n)
        walk = WL.WalkLoop(oracle, scen, sc, n)
        hw = dict(contacts=[], foot=[], state=[], R=[])
        for t, (stepped, cmd, toggle) in enumerate(WL.schedule(n)):
            walk.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
            if t >= WL.PRIME + WL.STAND:
                for k, v in (("contacts", walk.ct), ("foot", walk.foot), ("state", walk.x), ("R", walk.R)):
                    hw[k].append(v.copy())
        out["walk"] = {k: np.stack(v) for k, v in hw.items()}
        out["planes"] = GL.ramp_planes(sc, GL.RAMP_SLOPE)
        out["ramp"] = GL.run(GL.GroundLoop(oracle, scen, sc, n, ground=out["planes"]), n)
        out["touch"] = GL.run(GL.GroundLoop(oracle, scen, sc, n, touch_force=GL.TOUCH_FORCE), n)
        _SHARED["loops"] = out
    return _SHARED["loops"]


def test_loop_reduction(oracle, scen):
    """ground = 0 and touch_force = 0: the loop's history is WalkLoop's bit for bit, conditions_hold stays empty and no contact differs from the plan"""
    L = _loops(oracle, scen)
    hist, failed = L["reduction"]
    assert not failed, failed[:3]
    for k, v in L["walk"].items():
        assert v.shape == hist[k].shape and np.array_equal(v.view(np.uint8), hist[k].view(np.uint8)), k
    assert not GL.early_contacts(hist)


def test_loop_ramp(oracle, scen):
    """four robots on (sx, sy) = (+s, 0), (-s, 0), (0, +s), (0, 0), s = 0.15 (the first of 0.15 / 0.10 / 0.05 tried, and it held), touch_force 0: conditions_hold (height
    above the robot's own plane) stays empty on every tick; every touchdown is on the robot's own plane within 1e-12; the flat robot's history is the reduction run's
    bit for bit; on the two pitch ramps the tick's terrain_angle over the last 120 ticks is atan(s) within GL.TERRAIN_BAR (measured worst deviation 8.72e-5);
    root_euler_d[1] carries the reference's sign on every tick: -terrain_angle where the front feet's recent contacts lie more than 0.05 above the rear feet's, else
    +terrain_angle -- negative on the uphill robot, positive on the downhill one over those ticks.  The body pitch against the flat robot's is printed"""
    L = _loops(oracle, scen)
    s = GL.RAMP_SLOPE
    assert s == GL.SLOPES[0]
    hist, failed = L["ramp"]
    assert not failed, failed[:3]
    td, h = GL.touchdown_heights(hist, L["planes"])
    assert len(td) == 12 * 4 and np.abs(td).max() <= GL.TOUCHDOWN and h.min() >= -GL.TOUCHDOWN
    red = L["reduction"][0]
    for k in GL.KEYS:
        assert np.array_equal(np.ascontiguousarray(hist[k][:, 3]).view(np.uint8), np.ascontiguousarray(red[k][:, 3]).view(np.uint8)), k
    ta = hist["terrain_angle"][-GL.TERRAIN_TICKS:]
    dev = float(np.abs(ta[:, :2] - np.arctan(s)).max())
    assert GL.TERRAIN_BAR <= np.arctan(s) / 2
    frd = (hist["recent"][:, :, 2] + hist["recent"][:, :, 5]) - hist["recent"][:, :, 8] - hist["recent"][:, :, 11]
    want = np.where(frd > 0.05, -hist["terrain_angle"], hist["terrain_angle"])
    pitch = hist["state"][-GL.TERRAIN_TICKS:, :, 1].mean(axis=0)
    print(f"ramp s = {s}: terrain angle on the pitch ramps off atan(s) = {np.arctan(s):.5f} by {dev:.2e} at most (bar {GL.TERRAIN_BAR:.2e}), on the roll ramp "
          f"{ta[:, 2].min():.5f} .. {ta[:, 2].max():.5f}, flat {ta[:, 3].max():.1e}; root_euler_d[1] at the end {hist['pitch_d'][-1]}; mean body pitch over the last "
          f"{GL.TERRAIN_TICKS} ticks {pitch} (flat robot: {pitch[3]:+.4f})")
    assert dev <= GL.TERRAIN_BAR, dev
    assert np.array_equal(hist["pitch_d"], want)
    assert (hist["pitch_d"][-GL.TERRAIN_TICKS:, 0] < 0).all() and (hist["pitch_d"][-GL.TERRAIN_TICKS:, 1] > 0).all()


def test_loop_touch(oracle, scen):
    """flat ground, touch_force = 60: conditions_hold stays empty; every tick where contacts differ from the plan is an early contact -- there the gait counter is above
    1.5 counter_per_swing and the leg's touch byte out of the previous step was 1; every robot has at least one (without the touch sensor: none -- the reduction run);
    the contacts are exactly those of the reference's latch rule recomputed from the history, so the latch clears as the reference's does.  Early contacts per swing and
    the height-estimate error against the blind run are printed"""
    L = _loops(oracle, scen)
    hist, failed = L["touch"]
    assert not failed, failed[:3]
    ec = GL.early_contacts(hist)
    for t, b, l in ec:
        assert hist["plan"][t, b, l] == 0 and hist["contacts"][t, b, l] == 1
        assert hist["gc"][t, b, l] > 1.5 * WL.PER_SWING and hist["touch_read"][t, b, l] == 1, (t, b, l)
    per_robot = [sum(1 for e in ec if e[1] == b) for b in range(4)]
    assert min(per_robot) >= 1, per_robot
    assert np.array_equal(GL.latch_by_the_reference_rule(hist), hist["contacts"])
    assert any(hist["contacts"][t + 1, b, l] == 1 and hist["plan"][t + 1, b, l] == 1 for t, b, l in ec if t + 1 < WL.WALK)   # (an early contact runs into the planned stance)
    seen = set(ec)
    swings = int(((hist["plan"][1:] == 0) & (hist["plan"][:-1] == 1)).sum()) + int((hist["plan"][0] == 0).sum())
    first = sum(1 for t, b, l in ec if (t - 1, b, l) not in seen)
    herr = float(np.abs(hist["root_pos"][:, :, 2] - hist["state"][:, :, 5]).max())
    blind = L["reduction"][0]
    berr = float(np.abs(blind["root_pos"][:, :, 2] - blind["state"][:, :, 5]).max())
    td, h = GL.touchdown_heights(hist, np.zeros((4, 3)))
    assert np.abs(td).max() <= GL.TOUCHDOWN and h.min() >= -GL.TOUCHDOWN
    print(f"touch loop: {len(ec)} early-contact ticks, per robot {per_robot}, in {first} of {swings} swings ({first / swings:.2f} per swing); height estimate off by "
          f"{herr:.2e} at most (blind run: {berr:.2e})")
