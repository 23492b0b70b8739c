"""The shipped kernel text under the host sanitizers, on exact-fit buffers.  Each emulation of tests/emu/*_host.py is built as a stand-alone program (tests/emu/sanitize.py:
its own `main`, the sanitizer's runtime linked statically, nothing loaded into python) twice: under AddressSanitizer + UBSan, where every argument is an allocation of its
own of exactly the bytes include/a1mpc.h states for it -- a tail load that is not clamped reads the redzone even though its value is discarded -- and under
ThreadSanitizer, where the 64 host threads of a wavefront race on the LDS image wherever a WaveStage::sync() / __syncthreads() is missing.  In both runs the outputs are
held to the numpy restatements under the rule of the family's own host test: bit for bit, or that test's bar for the libm outputs; never to the unsanitized emulation.
Shapes: the smallest at which the tails differ -- n in {1, 15, 16, 17, 33} for the 16-robot waves, {1, 63, 64, 65} for the 64-robot ones; the strides 12 / 13 / 22;
sub-steps 1 and 3; every optional pointer null and given; the in-place calls; a NaN input where the header defines the outcome.  Behind the ten thread-per-lane
families: the contact / terrain kernels with their LDS staging (tests/emu/n2b_wave_host.py; plain as well), and the solver source on its fibers under asan, one program
per horizon.  Build and run times, the seeded defects each sanitizer reports, and the findings: profiles/host_sanitizers.md."""
import os, sys
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import sanitize
import episode_host, horizon_states_host, n2b_host, n2b_wave_host, plant_host, respawn_host, sensor_noise_host, sensor_synthesis_host, walk_sensors_host, walk_sensors_touch_host
import walk_step_ground_host, walk_step_host
import episode_ref as ER
import ground_ref as GR
import horizon_states_ref as HS
import noise_ref as NR
import plant_ref as PR
import respawn_ref as RR
import sensor_synthesis_ref as SR
import walk_ref as WR
from gpu_common import _strided_inputs

SANITIZERS = ("asan", "tsan")
WAVE16 = (1, 15, 16, 17, 33)
WAVE64 = (1, 63, 64, 65)
TOUCH_FORCE = 60.0
_FAMILIES = {   # name -> (host module, what sanitize.Library needs beyond it: the modules that borrow a preamble or compile more than their own section)
    "horizon_states": (horizon_states_host, {}),
    "plant": (plant_host, {}),
    "walk": (walk_step_host, {}),
    "ground": (walk_step_ground_host, dict(pre=lambda: walk_step_host._PRE)),
    "synthesis": (sensor_synthesis_host, {}),
    "walk_sensors": (walk_sensors_host, dict(pre=lambda: walk_step_host._PRE)),
    "touch_sensors": (walk_sensors_touch_host, dict(pre=lambda: walk_step_host._PRE)),
    "noise": (sensor_noise_host, {}),
    "episode": (episode_host, dict(body=lambda: plant_host.section() + episode_host.section())),
    "respawn": (respawn_host, {}),
    "n2b_wave": (n2b_wave_host, {}),
}
_LIBS, _SHARED = {}, {}


def _lib(family, sanitizer):
    key = (family, sanitizer)
    if key not in _LIBS:
        module, kw = _FAMILIES[family]
        _LIBS[key] = sanitize.Library(module, sanitizer, **{k: v() for k, v in kw.items()})
    return _LIBS[key]


@pytest.fixture(scope="module")
def programs():
    """every program of this file, built side by side (at most 16 compilers) before the first case needs one"""
    libs = [_lib(f, s) for f in _FAMILIES for s in SANITIZERS]
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda l: l.exe(), libs))
    return _lib


@pytest.fixture(params=SANITIZERS)
def sanitizer(request):
    return request.param


def _once(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _swing_nan(grf, contacts):
    """a NaN in one word of every swing leg's force: the header says it is not read"""
    grf = grf.copy(); swing = np.argwhere(contacts == 0)
    assert len(swing) > 0
    for i, l in swing:
        grf[i, 3 * l + (i + l) % 3] = np.nan
    return grf


# ---- horizon states: the states within HS.BAR of the scale of their terms, the costs within HS.BAR (tests/test_horizon_states_host.py)
HS_CASES = [   # n, H (a four-step chunk with remainder 0 and 2), per-step feet, u, x_pred, cost, a yaw of its own
    (1, 4, False, True, True, True, False), (15, 6, True, True, True, False, True), (16, 10, True, False, True, True, False), (17, 6, False, True, False, True, False),
    (33, 10, True, True, True, True, True), (33, 4, False, False, False, True, False)]


@pytest.mark.parametrize("n,h,feet,with_u,want_x,want_cost,own_yaw", HS_CASES)
def test_horizon_states(scen, programs, sanitizer, n, h, feet, with_u, want_x, want_cost, own_yaw):
    rng = np.random.default_rng(100 * h + n)
    sc, foot, fs, _, _ = _strided_inputs(scen, rng, h, n, feet, False)
    u = rng.uniform(-60.0, 180.0, (n, 12 * h)) if with_u else None
    yaw = sc["x0"][:, 2] + rng.uniform(-0.5, 0.5, n) if own_yaw else None
    with sanitize.instead_of_load(horizon_states_host, programs("horizon_states", sanitizer)):
        xp, cost = horizon_states_host.run(sc["params"], h, sc["R"], foot, x0=sc["x0"], xref=sc["xref"] if want_cost else None, u=u, foot_stride=fs, yaw_A=yaw, want_x=want_x,
                                           want_cost=want_cost)
    X, S = HS.rollout(sc["params"], h, sc["x0"], sc["R"], foot, fs, u, yaw)
    if want_x:
        assert xp.shape == (n, h, 13) and HS.states_ratio(xp, X, S) <= HS.BAR
        assert np.array_equal(xp[:, :, 12], np.broadcast_to(sc["x0"][:, 12:13], (n, h)))
    else:
        assert xp is None
    if want_cost:
        cy = HS.costs(sc["params"], h, X, sc["xref"], u)
        q = np.asarray(sc["params"]["q"], np.float64)[:12]
        scale0 = (q * (S[..., :12] + np.abs(sc["xref"].reshape(n, h, 13)[..., :12])) ** 2).sum((1, 2))
        assert cost.shape == (n, 2) and float((np.abs(cost[:, 0] - cy[:, 0]) / scale0).max()) <= HS.BAR
        if with_u:
            assert float((np.abs(cost[:, 1] - cy[:, 1]) / cy[:, 1]).max()) <= HS.BAR
        else:
            assert (cost[:, 1] == 0.0).all()
    else:
        assert cost is None


# ---- plant step: pos, R, v, omega and the feet bit for bit, the angles within PR.ANGLE_BAR (tests/test_plant_host.py)
PLANT_CASES = [   # n, stride, substeps, ext, in place, a NaN force on every swing leg
    (1, 12, 1, False, False, False), (15, 13, 3, True, False, False), (16, 22, 1, True, True, False), (17, 12, 3, False, True, False), (33, 13, 1, True, False, True),
    (33, 22, 3, False, False, False)]


@pytest.mark.parametrize("n,stride,substeps,with_ext,in_place,nan_swing", PLANT_CASES)
def test_plant_step(scen, programs, sanitizer, n, stride, substeps, with_ext, in_place, nan_swing):
    rng = np.random.default_rng(7000 + 100 * n + stride)
    sc = PR.random_robots(scen, rng, n)
    state = np.concatenate([sc["state"], rng.normal(0, 1, (n, stride - 12))], 1)
    ext = sc["ext"] if with_ext else None
    ref = PR.step(sc["params"], state, sc["R"], sc["foot"], sc["grf"], sc["contacts"], ext, 0.0025, substeps)
    grf = _swing_nan(sc["grf"], sc["contacts"]) if nan_swing else sc["grf"]
    with sanitize.instead_of_load(plant_host, programs("plant", sanitizer)):
        so, Ro, fo = plant_host.run(sc["params"], state, sc["R"], sc["foot"], grf, sc["contacts"], ext, 0.0025, substeps, in_place=in_place)
    assert so.shape == (n, stride) and Ro.shape == (n, 9) and fo.shape == (n, 12)
    assert PR.bits_equal(so[:, 3:12], ref[0][:, 3:12]) and PR.bits_equal(Ro, ref[1]) and PR.bits_equal(fo, ref[2])
    assert np.abs(so[:, :3] - ref[0][:, :3]).max() <= PR.ANGLE_BAR
    assert np.array_equal(so[:, 12:], state[:, 12:]) if in_place else np.isnan(so[:, 12:]).all()


# ---- walk step and ground step: as the plant step, foot_vel_body (and touch) bit for bit as well (tests/test_walk_host.py, tests/test_ground_host.py)
def _walkers(scen):
    def make():
        rng = np.random.default_rng(8100)
        sc = WR.random_walkers(scen, rng, max(WAVE16))
        sc["state"][:, 5] = rng.uniform(0.25, 0.45, max(WAVE16))   # (standing height above the planes: tests/test_ground_host.py)
        sc["wide"] = np.concatenate([sc["state"], rng.normal(0, 1, (max(WAVE16), 10))], 1)
        sc["ground"] = GR.random_planes(sc, rng, max(WAVE16))
        return _freeze(sc)
    return _once("walkers", make)


WALK_CASES = [   # n, stride, substeps, swing_track (0: R_z and foot_target null), the ground, ext, in place, NaNs that are not read
    (1, 12, 1, 1.0, "planes", True, False, False), (15, 13, 3, 0.5, "flat", False, False, False), (16, 22, 1, 0.0, "none", True, True, False),
    (17, 12, 3, 1.0, "planes", True, True, False), (33, 13, 1, 0.5, "none", False, False, False), (33, 22, 3, 1.0, "flat", True, False, True)]


def _walk_inputs(scen, n, stride, track, with_ext, nan):
    sc = _walkers(scen)
    grf, target = sc["grf"][:n], sc["target"][:n]
    if nan:   # a NaN force on every swing leg and a NaN target on every stance leg: neither is read
        grf = _swing_nan(grf, sc["contacts"][:n])
        target = target.copy()
        for i, l in np.argwhere(sc["contacts"][:n] != 0):
            target[i, 3 * l + (i + l) % 3] = np.nan
    tracked = track != 0.0
    clean = (sc["params"], sc["wide"][:n, :stride], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n] if tracked else None,
             sc["target"][:n] if tracked else None)
    given = clean[:4] + (grf, clean[5], clean[6], target if tracked else None)
    return sc, clean, given, (sc["ext"][:n] if with_ext else None)


def _same_step(out, ref, n, stride, state, in_place):
    so, Ro, fo, vo = out[:4]
    assert so.shape == (n, stride) and Ro.shape == (n, 9) and fo.shape == (n, 12) and vo.shape == (n, 12)
    assert PR.bits_equal(so[:, 3:12], ref[0][:, 3:12]) and PR.bits_equal(Ro, ref[1]) and PR.bits_equal(fo, ref[2]) and PR.bits_equal(vo, ref[3])
    assert np.abs(so[:, :3] - ref[0][:, :3]).max() <= PR.ANGLE_BAR
    assert np.array_equal(so[:, 12:], state[:, 12:]) if in_place else np.isnan(so[:, 12:]).all()


@pytest.mark.parametrize("n,stride,substeps,track,ground,with_ext,in_place,nan", WALK_CASES)
def test_walk_step(scen, programs, sanitizer, n, stride, substeps, track, ground, with_ext, in_place, nan):
    """(the walk step knows cfg's flat plane alone: `planes` is the plane at 0.05 here as well)"""
    sc, clean, given, ext = _walk_inputs(scen, n, stride, track, with_ext, nan)
    kw = dict(dt=0.0025, substeps=substeps, swing_track=track, flat_ground=0 if ground == "none" else 1, ground_z=0.05)
    ref = WR.step(*clean, ext, **kw)
    with sanitize.instead_of_load(walk_step_host, programs("walk", sanitizer)):
        out = walk_step_host.run(*given, ext, in_place=in_place, **kw)
    _same_step(out, ref, n, stride, clean[1], in_place)


@pytest.mark.parametrize("n,stride,substeps,track,ground,with_ext,in_place,nan", WALK_CASES)
def test_ground_step(scen, programs, sanitizer, n, stride, substeps, track, ground, with_ext, in_place, nan):
    sc, clean, given, ext = _walk_inputs(scen, n, stride, track, with_ext, nan)
    planes = sc["ground"][:n] if ground == "planes" else None
    kw = dict(dt=0.0025, substeps=substeps, swing_track=track, flat_ground=1 if ground == "flat" else 0, ground_z=0.05)
    ref = GR.step(*clean, planes, ext, **kw)
    with sanitize.instead_of_load(walk_step_ground_host, programs("ground", sanitizer)):
        out = walk_step_ground_host.run(*given, planes, ext, in_place=in_place, **kw)
    _same_step(out, ref, n, stride, clean[1], in_place)
    assert out[4].shape == (n, 4) and np.array_equal(out[4], ref[4])


# ---- sensor synthesis, walk sensors, touch sensors: SR.BITS bit for bit, SR.NOISY within 4 E of the 80-bit evaluation, E over the 65 robots of the host tests' own
# scenes (tests/test_sensor_synthesis_host.py, tests/test_walk_host.py, tests/test_ground_host.py: the same seeds, so the same bar)
SENSOR_ROBOTS = 65
SENSOR_CASES = [   # n, stride, ext, the optional outputs, the optional inputs (foot_vel_body; touch)
    (1, 12, False, True, True), (15, 13, True, False, True), (16, 22, True, True, False), (17, 12, False, False, False), (33, 13, True, True, True)]


def _sensor_refs(scen, kind, with_ext, with_opt):
    """the scene of the family's host test and its restatement in float64 and in 80 bits on all 65 robots, computed once"""
    def scene():
        rng = np.random.default_rng(dict(synthesis=6100, walk_sensors=7200, touch_sensors=8100)[kind])
        sc = SR.random_robots(scen, rng, SENSOR_ROBOTS, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        if kind != "synthesis":
            sc["vel"] = rng.normal(0, 1.0, (SENSOR_ROBOTS, 12))
        if kind == "touch_sensors":
            sc["touch"] = rng.choice(np.array([0, 1, 200], np.uint8), (SENSOR_ROBOTS, 4))
        return _freeze(sc)
    sc = _once(("scene", kind), scene)

    def refs():
        a = (sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"])
        ext = sc["ext"] if with_ext else None
        out = []
        for dt in (np.float64, np.longdouble):
            if kind == "synthesis":
                out.append(SR.synthesise(*a, ext, rho_opt=sc["rho_opt"], dtype=dt))
            elif kind == "walk_sensors":
                out.append(WR.sensors(*a, sc["vel"] if with_opt else None, ext, rho_opt=sc["rho_opt"], dtype=dt))
            else:
                out.append(GR.sensors(*a, sc["vel"], sc["touch"] if with_opt else None, TOUCH_FORCE, ext, rho_opt=sc["rho_opt"], dtype=dt))
        return out
    return sc, _once(("refs", kind, with_ext, with_opt if kind != "synthesis" else True), refs)


def _same_sensors(out, r64, r80, n, want_rel):
    assert all(v is None if (k in ("foot_pos_rel", "foot_vel_rel") and not want_rel) else v.shape[0] == n for k, v in out.items())
    SR.assert_is_ref(out, r64, r80, n)
    assert not any(np.isnan(v).any() for k, v in out.items() if v is not None and k != "reach")


@pytest.mark.parametrize("n,stride,with_ext,want_rel,with_opt", SENSOR_CASES)
def test_sensor_synthesis(scen, programs, sanitizer, n, stride, with_ext, want_rel, with_opt):
    sc, (r64, r80) = _sensor_refs(scen, "synthesis", with_ext, True)
    state = np.concatenate([sc["state"], np.random.default_rng(stride).normal(0, 1, (SENSOR_ROBOTS, stride - 12))], 1)[:n]
    with sanitize.instead_of_load(sensor_synthesis_host, programs("synthesis", sanitizer)):
        out = sensor_synthesis_host.run(sc["mass"], state, sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["ext"][:n] if with_ext else None,
                                        rho_opt=sc["rho_opt"], want_foot_rel=want_rel)
    _same_sensors(out, r64, r80, n, want_rel)


@pytest.mark.parametrize("n,stride,with_ext,want_rel,with_opt", SENSOR_CASES)
def test_walk_sensors(scen, programs, sanitizer, n, stride, with_ext, want_rel, with_opt):
    """(17 robots: the wrench, foot_vel_body and both optional outputs null at once)"""
    sc, (r64, r80) = _sensor_refs(scen, "walk_sensors", with_ext, with_opt)
    state = np.concatenate([sc["state"], np.random.default_rng(stride).normal(0, 1, (SENSOR_ROBOTS, stride - 12))], 1)[:n]
    with sanitize.instead_of_load(walk_sensors_host, programs("walk_sensors", sanitizer)):
        out = walk_sensors_host.run(sc["mass"], state, sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["vel"][:n] if with_opt else None,
                                    sc["ext"][:n] if with_ext else None, rho_opt=sc["rho_opt"], want_foot_rel=want_rel)
    _same_sensors(out, r64, r80, n, want_rel)


@pytest.mark.parametrize("n,stride,with_ext,want_rel,with_opt", SENSOR_CASES)
def test_touch_sensors(scen, programs, sanitizer, n, stride, with_ext, want_rel, with_opt):
    sc, (r64, r80) = _sensor_refs(scen, "touch_sensors", with_ext, with_opt)
    state = np.concatenate([sc["state"], np.random.default_rng(stride).normal(0, 1, (SENSOR_ROBOTS, stride - 12))], 1)[:n]
    with sanitize.instead_of_load(walk_sensors_touch_host, programs("touch_sensors", sanitizer)):
        out = walk_sensors_touch_host.run(sc["mass"], state, sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["vel"][:n],
                                          sc["touch"][:n] if with_opt else None, TOUCH_FORCE, sc["ext"][:n] if with_ext else None, rho_opt=sc["rho_opt"], want_foot_rel=want_rel)
    _same_sensors(out, r64, r80, n, want_rel)
    if with_opt:
        hit = (sc["contacts"][:n] == 0) & (sc["touch"][:n] != 0)
        assert (out["foot_force"][hit] == TOUCH_FORCE).all()


# ---- sensor noise: z within NR.HOST_BAR, every array within its level times the bar plus an ulp (tests/test_noise_host.py); the arrays are changed in place
NOISE_CASES = [   # n, robot0, tick, seed, the bias, z_out, the sensors that are null
    (1, 0, 0, 2026, True, True, ()), (15, 2 ** 32 - 65, 7, 0x9E3779B97F4A7C15, True, False, ()), (16, 0, 2 ** 33, 2026, False, True, ("quat", "joint_vel")),
    (17, 100, 7, 2026, True, True, ("imu_acc_raw", "imu_gyro_raw", "joint_pos", "foot_force")), (33, 2 ** 32 - 65, 2 ** 33, 0x9E3779B97F4A7C15, True, True, ()),
    (33, 5, 3, 2026, False, True, NR.SENSORS)]


@pytest.mark.parametrize("n,robot0,tick,seed,with_bias,want_z,nulls", NOISE_CASES)
def test_sensor_noise(programs, sanitizer, n, robot0, tick, seed, with_bias, want_z, nulls):
    s = _once("noise", lambda: NR.random_sensors(max(WAVE16)))
    sens = {k: s[k][:n] for k in NR.SENSORS if k not in nulls}
    bias = s["imu_bias"][:n] if with_bias else None
    cfg = dict(NR.LOUD, seed=seed) if with_bias else dict(NR.LOUD, seed=seed, gyro_bias_walk=0.0, acc_bias_walk=0.0)   # (a walk without a bias is refused)
    ref, rbias, rz = NR.apply(cfg, robot0, tick, sens, bias) if (sens or with_bias) else ({}, None, NR.normals(seed, np.arange(n, dtype=np.uint64) + np.uint64(robot0), tick))
    with sanitize.instead_of_load(sensor_noise_host, programs("noise", sanitizer)):
        out, obias, z = sensor_noise_host.run(cfg, robot0, tick, sens, bias, n=n, want_z=want_z)
    assert set(out) == set(sens) and all(v.shape == sens[k].shape for k, v in out.items())
    if want_z:
        e = float(np.abs(z - rz).max())
        assert z.shape == (n, 44) and e <= NR.CEILING and e <= NR.HOST_BAR, e
    else:
        assert z is None
    got, want = dict(out), dict(ref)
    if with_bias:
        got["imu_bias"], want["imu_bias"] = obias, rbias
    if got:
        excess, figs = NR.worst_excess(got, want, cfg, NR.HOST_BAR, with_bias, n)
        assert excess <= 0.0, (excess, figs)
        assert all(not NR.bits_equal(got[k], s[k][:n]) for k in got)


def test_sensor_noise_levels_zero_keep_a_nan_row(programs, sanitizer):
    """all levels 0 and the bias null: every array keeps its bits, a -0 row, a NaN row and a NaN with a payload included"""
    n = 17
    s = {k: v[:n].copy() for k, v in _once("noise", lambda: NR.random_sensors(max(WAVE16))).items()}
    for k in NR.SENSORS:
        s[k][3] = -0.0; s[k][9] = np.nan
        s[k][16].view(np.uint64)[:] = 0x7FF8DEADBEEF0001
    sens = {k: s[k] for k in NR.SENSORS}
    with sanitize.instead_of_load(sensor_noise_host, programs("noise", sanitizer)):
        out, _, z = sensor_noise_host.run(NR.config(seed=2026), 0, 7, sens, None, n=n)
    assert all(NR.bits_equal(out[k], sens[k]) for k in NR.SENSORS)
    assert float(np.abs(z - NR.normals(2026, np.arange(n, dtype=np.uint64), 7)).max()) <= NR.HOST_BAR


# ---- episode update and summary: bit for bit (tests/test_episode_host.py)
EPISODE_CASES = [   # n, stride, the optional inputs that are null, a robot with a NaN in its state (ends with code 1)
    (1, 12, (), False), (15, 13, ("estimate",), False), (16, 22, ("forces", "ground"), False), (17, 12, ER.OPTIONAL, False), (33, 13, (), True), (33, 22, ("status", "reach"), False)]


@pytest.mark.parametrize("n,stride,nulls,nan", EPISODE_CASES)
def test_episode_update(programs, sanitizer, n, stride, nulls, nan):
    """two consecutive ticks from the all-zero record, the record updated in place"""
    ticks = _once(("episode", stride), lambda: ER.random_inputs(max(WAVE16), seed=9100 + stride, stride=stride, ticks=2))
    ref = out = np.zeros((n, ER.WORDS))
    for t, d in enumerate(ticks):
        d = {k: v[:n] for k, v in d.items()}
        for key in nulls:
            d = ER.without(d, key)
        if nan and t == 1:
            d["state"] = d["state"].copy(); d["state"][n // 2, 10] = np.nan
        ref = ER.update(ref, 1000 + t, **d)
        with sanitize.instead_of_load(episode_host, programs("episode", sanitizer)):
            out = episode_host.update(out, 1000 + t, **d)
        assert out.shape == (n, ER.WORDS) and ER.bits_equal(out, ref), t
    if nan:
        assert ref[n // 2, 2] == 1.0 and ref[n // 2, 1] == 1002.0 and (np.delete(ref[:, 2], n // 2) == 0.0).all()
    else:
        assert (ref[:, 0] == 2).all()


@pytest.mark.parametrize("n", WAVE64 + (4097,))
def test_episode_summary(programs, sanitizer, n):
    """one, two and three levels of launches; the workspace holds the partials of every level but the last and not a word more"""
    ep = np.ascontiguousarray(ER.random_records(n, seed=9200 + n))
    out = np.full(20, np.nan)
    words, rows = 0, n
    while rows > 64:
        rows = (rows + 63) // 64; words += 20 * rows
    ws = np.full(words, np.nan)
    launches = programs("episode", sanitizer).episode_summary_run(n, ep, out, ws)
    assert ER.bits_equal(out, ER.summary(ep)) and launches == (1 if n <= 64 else (2 if n <= 4096 else 3))


# ---- respawn: bit for bit (tests/test_respawn_host.py).  Every region of the kernel's table lies in an allocation of its own, sized for max_batch = n
def _split_images(images, geom):
    """the handle's blocks as the allocations the regions get: the contact block is three (records, leg rings, terrain ring) -> [(offset in the block, part)] per block"""
    M = geom["max_batch"]
    leg = 4 * RR.LEG_WINDOW * 4 * 8
    cuts = dict(contact=[0, M * RR.CT_RECORD, M * (RR.CT_RECORD + leg)])
    return {k: [(a, np.array(v[a:b])) for a, b in zip(cuts.get(k, [0]), cuts.get(k, [0])[1:] + [len(v)])] for k, v in images.items()}


def _respawn(lib, n, mask, ep, life, fin, mask_out, cfg, images, geom):
    """respawn_host.reset / decide on the sanitized program: the launcher's table for `images`, every base address replaced by that of the part it lies in"""
    g = respawn_host.regions(images, cfg["what"], geom)
    parts = _split_images(images, geom)
    fix = []
    for r in range(g.shape[0]):
        k, off = next((k, int(g[r, 0]) - v.ctypes.data) for k, v in images.items() if v.ctypes.data <= g[r, 0] < v.ctypes.data + v.nbytes)
        start, part = [(a, p) for a, p in parts[k] if a <= off][-1]
        assert off - start + (g[r, 4] - 1) * g[r, 2] + g[r, 3] + (n - 1) * g[r, 1] <= part.nbytes   # (the region ends inside its part, for the n robots)
        fix.append((g, 5 * r, part, off - start)); g[r, 0] = 0
    lib.respawn_run(n, mask, ep, life, fin, mask_out, cfg["codes"], cfg["hold_ticks"], cfg["max_ticks"], g.shape[0], g, fixups=fix,
                    extra=[p for ps in parts.values() for _, p in ps])
    return {k: np.concatenate([p for _, p in ps]) for k, ps in parts.items()}


@pytest.mark.parametrize("horizon,window", [(10, 5), (1, 1)])
@pytest.mark.parametrize("n", WAVE64)
def test_respawn_masked_reset(programs, sanitizer, n, horizon, window):
    geom = dict(max_batch=n, horizon=horizon, window=window)
    im = RR.pattern_images(geom, seed=8100 + window + horizon + n)
    mask = RR.make_mask("half" if n > 1 else "all", n)
    out = _respawn(programs("respawn", sanitizer), n, mask, None, None, None, None, dict(codes=0, hold_ticks=0, max_ticks=0, what=RR.ALL), im, geom)
    ref = RR.reset(im, mask, RR.ALL, geom)
    assert out.keys() == ref.keys() and all(RR.bits_equal(out[k], ref[k]) for k in ref)
    assert mask.any() and any(not RR.bits_equal(out[k], im[k]) for k in im)


@pytest.mark.parametrize("with_finished", [True, False])
@pytest.mark.parametrize("n", WAVE64)
def test_respawn_decision(programs, sanitizer, n, with_finished):
    geom = dict(max_batch=n, horizon=10, window=5)
    im = RR.pattern_images(geom, seed=8200 + n)
    ep0, life0 = RR.decision_cases(n, seed=8200 + n)
    for cfg in (dict(RR.DEFAULT, max_ticks=50), dict(codes=0x4, max_ticks=50, hold_ticks=0, what=RR.EKF | RR.SENSOR)):
        ep, life, mask = ep0.copy(), life0.copy(), np.full(n, 0xEE, dtype=np.uint8)
        fin = np.full((n, RR.WORDS), -1.0) if with_finished else None
        out = _respawn(programs("respawn", sanitizer), n, None, ep, life, fin, mask, cfg, im, geom)
        re, rl, rf, rm = RR.decide(ep0, life0, cfg, None if fin is None else np.full((n, RR.WORDS), -1.0))
        assert RR.bits_equal(ep, re) and RR.bits_equal(life, rl) and RR.bits_equal(mask, rm) and (fin is None or RR.bits_equal(fin, rf)), cfg
        ref = RR.reset(im, (rm == 1).astype(np.uint8), cfg["what"], geom)
        assert all(RR.bits_equal(out[k], ref[k]) for k in ref), cfg


@pytest.mark.parametrize("n,when", [(1, 3), (63, 1), (64, 2), (65, 3)])
def test_respawn_rows(programs, sanitizer, n, when):
    """rows of 1, 8, 13 and 96 bytes (the word path and the byte path), a row per robot and one row for all; every dst exactly n rows"""
    rng = np.random.default_rng(8300 + n)
    mask = rng.integers(0, 4, size=n, dtype=np.uint8)
    table = [(rng.integers(0, 256, size=(n, rb), dtype=np.uint8), rng.integers(0, 256, size=(n if per_robot else 1, rb), dtype=np.uint8), when)
             for rb in (1, 8, 13, 96) for per_robot in (False, True)]
    want = RR.rows(mask, table)
    t = np.array([(0, 0, d.shape[1], s.shape[0], w) for d, s, w in table], dtype=np.int64)
    fix = [(t, 5 * k + c, (d, s)[c], 0) for k, (d, s, _) in enumerate(table) for c in (0, 1)]
    programs("respawn", sanitizer).respawn_rows_run(n, mask, len(table), t, fixups=fix, extra=[a for d, s, _ in table for a in (d, s)])
    assert all(RR.bits_equal(d, ref) for (d, _, _), ref in zip(table, want))
    assert any(not RR.bits_equal(d, s if s.shape[0] == n else np.tile(s, (n, 1))) for d, s, _ in table) or n == 1


# ---- the contact / terrain kernels WITH their LDS staging (tests/emu/n2b_wave_host.py), plain and under both sanitizers, held to n2b_host.HostN2b -- the per-robot body
# on the records themselves -- stepped over the same 130 ticks, bit for bit; rec, leg_ring and terrain_ring are three exact-fit allocations
N2B_TICKS = 130
PK_FIELDS = 7


def _n2b_reference(n):
    """130 ticks of the fleet of tests/test_n2b_host.py (the leg window of 60 and the terrain window of 100 both wrap, a tenth of the robots lie down) on HostN2b: the
    full entry, and the terrain-only entry fed the full entry's positions; computed once per n"""
    def make():
        rng = np.random.default_rng(2100 + n)
        base = np.outer([0.2, 0.2, -0.2, -0.2], [1.0, 0.0, 0.3]).reshape(12) + np.outer([1, -1, 1, -1], [0.0, 0.13, 0.0]).reshape(12)
        gcs = np.zeros((N2B_TICKS, n, 4)); gc = rng.uniform(0, 240, (n, 4))
        for t in range(N2B_TICKS):
            gc = np.fmod(gc + 2.0, 240.0); gcs[t] = gc
        d = dict(gc=gcs, plan=(gcs <= 120).astype(np.uint8), ff=rng.uniform(0, 80, (N2B_TICKS, n, 4)),
                 foot=base + rng.normal(0, 0.03, (N2B_TICKS, n, 12)) + np.tile([0.0, 0.0, -0.3], 4), z=np.where(rng.random((N2B_TICKS, n)) < 0.9, 0.3, 0.05),
                 pitch0=np.full(n, 0.0625), pk=rng.normal(0, 1, 22 * n))
        A, B = n2b_host.HostN2b(n), n2b_host.HostN2b(n)
        pa, pb = d["pitch0"], d["pitch0"]
        full = {k: [] for k in ("contacts", "foot_pos_recent_contact", "terrain_angle", "root_euler_d_pitch")}
        only = {k: [] for k in ("terrain_angle", "root_euler_d_pitch")}
        for t in range(N2B_TICKS):
            oa = A.tick(d["gc"][t], d["plan"][t], d["ff"][t], d["foot"][t], d["z"][t], pa); pa = oa["root_euler_d_pitch"]
            ob = B.tick(d["gc"][t], d["plan"][t], d["ff"][t], d["foot"][t], d["z"][t], pb, recent_in=oa["foot_pos_recent_contact"]); pb = ob["root_euler_d_pitch"]
            for k in full: full[k].append(oa[k])
            for k in only: only[k].append(ob[k])
        d["full"] = {k: np.stack(v) for k, v in full.items()}; d["only"] = {k: np.stack(v) for k, v in only.items()}
        words = n * n2b_wave_host.RECORD // 8
        cut = lambda H: (H.base[:words].copy(), H.base[words:words + n * n2b_wave_host.LEG_RING].copy(),
                         H.base[words + n * n2b_wave_host.LEG_RING:words + n * (n2b_wave_host.LEG_RING + n2b_wave_host.TERRAIN_WINDOW)].copy())
        d["full_state"], d["only_state"] = cut(A), cut(B)
        assert d["full"]["contacts"].any() and not d["full"]["contacts"].all() and np.abs(d["full"]["terrain_angle"]).max() > 0 and (d["z"] < 0.1).any()
        return _freeze(d)
    return _once(("n2b", n), make)


@pytest.mark.parametrize("mode", ["full", "full+tick", "terrain", "contacts"])
@pytest.mark.parametrize("n", WAVE64)
@pytest.mark.parametrize("how", ("plain",) + SANITIZERS)
def test_contact_terrain_wavefront(programs, how, n, mode):
    d = _n2b_reference(n)
    a = (d["gc"], d["plan"], d["ff"], d["foot"], d["z"], d["pitch0"])
    call = lambda: (n2b_wave_host.run("full", *a, pk=d["pk"] if mode == "full+tick" else None) if mode.startswith("full") else
                    n2b_wave_host.run("terrain", None, None, None, None, d["z"], d["pitch0"], recent_in=d["full"]["foot_pos_recent_contact"]) if mode == "terrain" else
                    n2b_wave_host.run("contacts", *a))
    if how == "plain":
        out = call()
    else:
        with sanitize.instead_of_load(n2b_wave_host, programs("n2b_wave", how)):
            out = call()
    same = lambda x, y: x.shape == y.shape and x.tobytes() == y.tobytes()
    rec, leg, ter = (v.view(np.float64) for v in out["state"])
    rrec, rleg, rter = d["only_state"] if mode == "terrain" else d["full_state"]
    if mode == "terrain":
        ref = d["only"]
        assert out["contacts"] is None and out["foot_pos_recent_contact"] is None and not leg.any()
        assert same(rec, rrec) and same(ter, rter)
    else:
        ref = d["full"]
        assert same(out["contacts"], ref["contacts"]) and same(out["foot_pos_recent_contact"], ref["foot_pos_recent_contact"]) and same(leg, rleg)
    if mode == "contacts":   # the contact block alone: the legs' filters and foot_pos_recent_contact are the full entry's, the terrain filter stays empty
        assert out["terrain_angle"] is None and out["root_euler_d_pitch"] is None and not ter.any()
        assert same(rec.reshape(n, 48)[:, :44], rrec.reshape(n, 48)[:, :44]) and not rec.reshape(n, 48)[:, 44:].any()
    else:
        assert same(out["terrain_angle"], ref["terrain_angle"]) and same(out["root_euler_d_pitch"], ref["root_euler_d_pitch"])
    if mode.startswith("full"):
        assert same(rec, rrec) and same(ter, rter)
    if mode == "full+tick":   # the 22 words of the tick record are the eight arrays' words, copied
        pk = d["pk"]
        want = np.concatenate([pk[3 * n * k:3 * n * (k + 1)].reshape(n, 3) for k in range(PK_FIELDS)] + [pk[21 * n:].reshape(n, 1)], 1)
        assert same(out["tick"], np.broadcast_to(want, (N2B_TICKS, n, 22)).copy())
    else:
        assert out["tick"] is None


# ---- the solver source on the host fibers of tests/emu/emu_harness.cpp, under asan: one program per horizon.  The harness keeps the LDS image, the set-up hand-off and
# the tables in std::vectors of exactly Layout<H>::ROW_STRIDE / Prep<H>::STRIDE / 2 H H doubles, and here every argument and the carry are exact-fit allocations too.
# Held to the oracle by tests/test_emu_parity.py's rule: the oracle's iteration count and status, forces within helpers.TOL_FORCE_N (the balance QP: its own bound there)
SOLVER_HORIZONS = (1, 4, 10, 16)


@pytest.fixture(scope="module")
def solver_programs():
    """one program per horizon, built side by side"""
    libs = {h: _once(("solver", h), lambda: sanitize.solver_library(h)) for h in SOLVER_HORIZONS}
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda l: l.exe(), libs.values()))
    return libs


def _params_bytes(P):
    return np.frombuffer(bytes(P), dtype=np.uint8).copy()


def _three_qps(scen, h):
    """a standing robot, a trot pair (two diagonal legs down), and a random QP with a NaN in its state"""
    def make():
        parts = [scen.scenario_stand(horizon=h), scen.config2_trot_sequence(1, horizon=h), scen.config3_random_flat(nb=1, horizon=h)]
        sc = dict(parts[0])
        for k in ("x0", "xref", "R", "foot", "contact"):
            sc[k] = np.ascontiguousarray(np.concatenate([p[k] for p in parts]))
        sc["x0"][2, 4] = np.nan
        assert sc["contact"].tolist()[:2] in ([[1, 1, 1, 1], [1, 0, 0, 1]], [[1, 1, 1, 1], [0, 1, 1, 0]]) and all(p["params"] == sc["params"] for p in parts)
        return _freeze(sc)
    return _once(("qps", h), make)


def _solver_outputs(n, h):
    return dict(grf=np.full((n, 12), np.nan), u=np.full((n, 12 * h), np.nan), iters=np.full(n, -1, np.int32), status=np.full(n, -99, np.int32), nfact=np.full(n, -1, np.int32))


def _same_as_oracle(out, ref, bad=2):
    """every QP stops at the oracle's iteration with the oracle's status; the finite ones within TOL_FORCE_N; the NaN input gives status -7 and zeros"""
    from helpers import TOL_FORCE_N
    ok = np.arange(len(out["iters"])) != bad
    assert np.array_equal(out["iters"][ok], ref["iters"][ok]) and np.array_equal(out["status"][ok], ref["status"][ok]) and (out["status"][ok] == 1).all()
    assert np.abs(out["grf"][ok] - ref["grf"][ok]).max() <= TOL_FORCE_N and np.abs(out["u"][ok] - ref["u"][ok]).max() <= TOL_FORCE_N
    assert out["status"][bad] == -7 == ref["status"][bad] and not out["grf"][bad].any() and np.isnan(out["u"][bad]).all() and np.isnan(ref["u"][bad]).all()


SOLVER_PATHS = [(h, path) for h in (4, 10, 16) for path in ("row", "twin", "quad", "latency", "split", "split pairs") if path != "quad" or h % 4 == 0]   # (a quad of rows: H % 4 == 0)


@pytest.mark.parametrize("h,path", SOLVER_PATHS)
def test_solver_source_fast_path(oracle, scen, solver_programs, h, path):
    import emu
    from helpers import oracle_batch
    sc = _three_qps(scen, h)
    ref = _once(("oracle", h), lambda: oracle_batch(oracle, sc, 3))
    P = _params_bytes(emu.make_params(sc["params"]))
    o = _solver_outputs(3, h)
    a = (sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], o["grf"], o["u"], None, None, None, o["iters"], o["status"], o["nfact"])
    lib = solver_programs[h]
    if path.startswith("split"):   # behind the set-up kernel two persistent rows drain the queue -- or two main / twin PAIRS of rows, as on the device
        rc = lib.san_solve_split(0, 0, None, P, h, 3, -2 if path == "split pairs" else 2, *a)
    else:
        rc = lib.san_solve(dict(row=0, twin=1, quad=2, latency=3)[path], 0, None, P, h, 3, *a)
    assert rc == 0
    _same_as_oracle(o, ref)


@pytest.mark.parametrize("h", [4, 10, 16])
def test_solver_source_general_path_with_per_step_feet(oracle, scen, solver_programs, h):
    import emu
    from helpers import oracle_params
    sc = _three_qps(scen, h)
    rng = np.random.default_rng(4100 + h)
    vd = rng.uniform(-0.6, 0.6, (3, 1, 1, 3))
    foot = np.ascontiguousarray((sc["foot"].reshape(3, 1, 4, 3) - vd * sc["params"]["dt"] * np.arange(h).reshape(1, h, 1, 1) * 40.0).reshape(3, h * 12))
    pr, st = oracle_params(oracle, sc), oracle.default_settings()
    ref = _solver_outputs(3, h)
    for b in range(3):
        r = oracle.mpc_solve(pr, st, sc["x0"][b], sc["xref"][b], sc["R"][b], foot[b], sc["contact"][b], foot_stride=12, contact_stride=0)
        ref["grf"][b], ref["u"][b], ref["iters"][b], ref["status"][b] = r["grf"], r["u"], r["info"].iters, r["info"].status
    o = _solver_outputs(3, h)
    P = _params_bytes(emu.make_params(sc["params"]))
    rc = solver_programs[h].san_solve_gen(1, None, P, h, 3, sc["x0"], sc["xref"], sc["R"], foot, 12, sc["contact"], 0, o["grf"], o["u"], None, None, None, o["iters"],
                                          o["status"], o["nfact"])
    assert rc == 0
    _same_as_oracle(o, ref)


@pytest.mark.parametrize("h", [4, 10, 16])
def test_solver_source_update_path_ticks_with_a_carry(oracle, scen, solver_programs, h):
    """warm_start = 2 on main / twin pairs, three QPs with a carry each (3 x (72 H + 14) doubles in one allocation, not one more) over three ticks: the first fills
    the carries, the later ones run the update path from them.  A standing robot (the same QP every tick), a trot (ticks 0 - 2 of the sequence) and a second trot
    (ticks 3 - 5) whose middle tick has a NaN in its state: that tick gives status -7 and zeros, and the tick behind it starts from cold iterates on the update path
    (tests/test_emu_parity.py::test_emulated_update_path_matches_oracle).  Every QP of every tick is held to oracle.mpc_solve_update on a carry of its own"""
    import emu
    from helpers import TOL_FORCE_N, oracle_params
    stand, seq = scen.scenario_stand(horizon=h), scen.config2_trot_sequence(6, horizon=h)
    assert stand["params"] == seq["params"]
    pr, st = oracle_params(oracle, seq), oracle.default_settings(warm_start=1)
    keys = ("x0", "xref", "R", "foot", "contact")
    carries_o = [oracle.update_carry(h) for _ in range(3)]
    wx, wy, rho, carry = np.zeros((3, 12 * h)), np.zeros((3, 20 * h)), np.zeros(3), np.zeros((3, RR.carry_stride(h)))
    P = _params_bytes(emu.make_params(seq["params"], warm_start=2))
    for k in range(3):
        tick = {key: np.ascontiguousarray(np.concatenate([stand[key][0:1], seq[key][k:k + 1], seq[key][3 + k:4 + k]])) for key in keys}
        if k == 1:
            tick["x0"][2, 4] = np.nan
        ref = [oracle.mpc_solve_update(pr, st, *[tick[key][b] for key in keys], carries_o[b]) for b in range(3)]
        o = _solver_outputs(3, h)
        rc = solver_programs[h].san_solve(1, 0, carry, P, h, 3, *[tick[key] for key in keys], o["grf"], o["u"], wx, wy, rho, o["iters"], o["status"], o["nfact"])
        assert rc == 0
        for b, r in enumerate(ref):
            assert o["iters"][b] == r["info"].iters and o["status"][b] == r["info"].status, (k, b, o["iters"], o["status"], r["info"].iters, r["info"].status)
            if k == 1 and b == 2:
                assert o["status"][b] == -7 and not o["grf"][b].any()
            else:
                assert o["status"][b] == 1 and np.abs(o["grf"][b] - r["grf"]).max() <= TOL_FORCE_N, (k, b)
    assert carry.any(axis=1).all() and (rho > 0).all()


def test_solver_source_balance_qp(oracle, scen, solver_programs):
    """H = 1: a standing robot, a trot pair and a NaN wrench through the row; the oracle's iteration count, forces within the balance QP's bound of tests/test_emu_parity.py"""
    import emu
    from helpers import TOL_FORCE_BALANCE_N
    parts = [scen.config1_balance_stand(), scen.balance_random(2), scen.balance_random(1, seed=77)]
    sc = {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])[[0, 1, 3]]) for k in ("root_acc", "R", "Rz", "foot", "contact")}
    sc["contact"][1] = (1, 0, 0, 1); sc["root_acc"][2, 1] = np.nan
    n = 3
    grf, f, iters, status = np.full((n, 12), np.nan), np.full((n, 12), np.nan), np.full(n, -1, np.int32), np.full(n, -99, np.int32)
    rc = solver_programs[1].san_balance(_params_bytes(emu.balance_params()), n, sc["root_acc"], sc["R"], sc["Rz"], sc["foot"], sc["contact"], grf, f, iters, status)
    assert rc == 0
    qp, st = oracle.default_qp_params(), oracle.default_settings()
    for b in range(n):
        r = oracle.balance_solve(qp, st, sc["root_acc"][b], sc["R"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
        assert iters[b] == r["info"].iters and status[b] == r["info"].status, (b, iters[b], status[b], r["info"].iters, r["info"].status)
        if b < 2:
            assert status[b] == 1 and np.abs(f[b] - r["f_world"]).max() < TOL_FORCE_BALANCE_N
        else:
            assert status[b] == -7 and not grf[b].any()
