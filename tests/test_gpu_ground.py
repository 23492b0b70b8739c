"""GPU: a1mpc_ground_step_batch(_device) and a1mpc_touch_sensors_batch(_device) -- the walk step over a ground plane per robot with a touch byte per leg, and the walk
sensors with a touch force.  Yardsticks: the elementwise numpy restatements of tests/ground_ref.py (the step's pos, R, v, omega, feet, foot_vel_body and touch BIT FOR
BIT, its angles within the walk tests' bar; the sensors by the rule of tests/sensor_synthesis_ref.py); the walk entries, which the new ones must reduce to bit for bit;
and the closed loops  touch sensors -> tick -> ground step  on one stream against the same loops on the CPU (tests/ground_loop.py).  One handle of 512 robots, gazebo
parameter set, h = 10, cold solves."""
import ctypes as C
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
from gpu_common import _engine, tick_buffers, tick_world

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 65, 257]
NMAX = max(SIZES)
TAIL = 3
GROUND_Z = 0.05
STEP_CONFIGS = list(itertools.product((1, 3), (0.0, 0.5, 1.0), ("planes", "flat", "none")))   # substeps (3: with a wrench), swing_track, the ground
WIDTHS = dict(quat=4, imu_acc_raw=3, imu_gyro_raw=3, joint_pos=12, joint_vel=12, foot_force=4, reach=4, foot_pos_rel=12, foot_vel_rel=12)
OK, INVALID, TOO_LARGE = 0, 1, 5
_SHARED = {}


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(rows, w):
    import torch
    return torch.full((rows, w), float("nan"), dtype=torch.float64, device=_dev())


def _ff(rows, w=4):
    import torch
    return torch.full((rows, w), 0xFF, dtype=torch.uint8, device=_dev())


@pytest.fixture(scope="module")
def eng(pkg, scen):
    e = _engine(pkg, scen.scenario_stand(), 512, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


def _walkers(scen):
    """257 random walkers as tick records at standing height with a random plane each (tests/test_ground_host.py's construction), and the restatement of every step
    configuration: computed once, never changed"""
    if "walk" not in _SHARED:
        rng = np.random.default_rng(8400)
        sc = WR.random_walkers(scen, rng, NMAX)
        sc["state"][:, 5] = rng.uniform(0.25, 0.45, NMAX)
        sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1))
        sc["ground"] = GR.random_planes(sc, rng, NMAX)
        refs = {}
        for cfg in STEP_CONFIGS:
            sub, track, mode = cfg
            refs[cfg] = GR.step(sc["params"], sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], sc["ground"] if mode == "planes" else None,
                                sc["ext"] if sub == 3 else None, 0.0025, sub, swing_track=track, flat_ground=1 if mode == "flat" else 0, ground_z=GROUND_Z)
            for a in refs[cfg]:
                a.setflags(write=False)
        _SHARED["walk"] = (sc, refs)
    return _SHARED["walk"]


def _walk_cfg(eng, sub, track, mode):
    return eng.walk_config(substeps=sub, swing_track=track, flat_ground=1 if mode == "flat" else 0, ground_z=GROUND_Z)


def _device_step(eng, sc, n, sub, track, mode, stride=22, stream=None, in_place=False, sl=None, ground="ground", walk_entry=False):
    """the device entry on the first n robots (or the slice sl) -> numpy (state (n + TAIL, stride), R, foot, foot_vel_body, touch): poisoned outputs, or in place.
    walk_entry: a1mpc_walk_step_batch_device instead (touch stays poisoned)"""
    import torch
    sl = slice(0, n) if sl is None else sl
    st = _t(sc["tick"][sl, :stride]); R = _t(sc["R"][sl]); foot = _t(sc["foot"][sl]); grf = _t(sc["grf"][sl]); ct = _t(sc["contacts"][sl])
    Rz, tg = _t(sc["Rz"][sl]), _t(sc["target"][sl])
    gr = _t(sc[ground][sl]) if mode == "planes" else None
    ew = _t(sc["ext"][sl]) if sub == 3 else None
    so, Ro, fo = (None, None, None) if in_place else (_nan(n + TAIL, stride), _nan(n + TAIL, 9), _nan(n + TAIL, 12))
    vo, to = _nan(n + TAIL, 12), _ff(n + TAIL)
    torch.cuda.synchronize()
    if walk_entry:
        eng.walk_step_device(n, st, stride, R, foot, grf, ct, Rz, tg, vo, ew, so, Ro, fo, walk=_walk_cfg(eng, sub, track, mode), stream=stream)
    else:
        eng.walk_step_ground_device(n, st, stride, R, foot, grf, ct, Rz, tg, vo, to, gr, ew, so, Ro, fo, walk=_walk_cfg(eng, sub, track, mode), stream=stream)
    torch.cuda.synchronize()
    if in_place:
        so, Ro, fo = st, R, foot
    return so.cpu().numpy(), Ro.cpu().numpy(), fo.cpu().numpy(), vo.cpu().numpy(), to.cpu().numpy()


def _assert_is_ref(out, ref, n, rows=slice(None)):
    so, Ro, fo, vo, to = out
    assert PR.bits_equal(so[:n, 3:12], ref[0][rows][:n, 3:12]) and PR.bits_equal(Ro[:n], ref[1][rows][:n]) and PR.bits_equal(fo[:n], ref[2][rows][:n])
    assert PR.bits_equal(vo[:n], ref[3][rows][:n]) and np.array_equal(to[:n], ref[4][rows][:n])
    worst = float(np.abs(so[:n, :3] - ref[0][rows][:n, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_step_device_and_host_entries_equal_the_restatement_bit_for_bit(eng, scen, n):
    """the first n of 257 robots; sub-steps 1 and 3 (with a wrench), swing_track 0 / 0.5 / 1, a plane per robot / cfg's flat plane / no ground: the device entry writes
    the restatement's bits (touch among them), nothing beyond row n and nothing into words [12:22) of the tick records; the host entry returns the device entry's bits"""
    sc, refs = _walkers(scen)
    worst = 0.0
    for cfg in STEP_CONFIGS:
        sub, track, mode = cfg
        out = _device_step(eng, sc, n, *cfg)
        assert all(np.isnan(a[n:]).all() for a in out[:4]) and (out[4][n:] == 0xFF).all() and np.isnan(out[0][:n, 12:]).all()
        assert not any(np.isnan(a[:n, :w]).any() for a, w in zip(out[:4], (12, 9, 12, 12)))
        worst = max(worst, _assert_is_ref(out, refs[cfg], n))
        h = eng.walk_step_ground(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n], sc["target"][:n],
                                 sc["ground"][:n] if mode == "planes" else None, sc["ext"][:n] if sub == 3 else None, walk=_walk_cfg(eng, *cfg))
        assert PR.bits_equal(h["state"][:, :12], out[0][:n, :12]) and PR.bits_equal(h["R"], out[1][:n]) and PR.bits_equal(h["foot"], out[2][:n])
        assert PR.bits_equal(h["foot_vel_body"], out[3][:n]) and np.array_equal(h["state"][:, 12:], sc["tick"][:n, 12:]) and np.array_equal(h["touch"], out[4][:n])
    print(f"n {n}: {len(STEP_CONFIGS)} configurations, device and host entries carry the restatement's bits; angles within {worst:.1e}")


def test_step_reductions_in_place_strides_streams_a_robot_alone_and_isolation(eng, scen):
    """ground NULL: every output but touch is a1mpc_walk_step_batch_device's bit for bit, cfg's plane off and on; ground = (ground_z, 0, 0): its bits with flat_ground =
    1.  In place == out of place, the command half of the tick records surviving; strides 12 and 13 give the same bits; a side stream; robot i alone has the bits of
    robot i of the 257; a NaN ground row stays with its robot"""
    import torch
    sc, refs = _walkers(scen)
    same = lambda g, w, n: all(PR.bits_equal(x[:n], y[:n]) for x, y in zip(g[:4], w[:4]))
    for sub, track, mode in ((1, 1.0, "none"), (3, 0.5, "flat"), (3, 0.0, "none")):
        assert same(_device_step(eng, sc, NMAX, sub, track, mode), _device_step(eng, sc, NMAX, sub, track, mode, walk_entry=True), NMAX)
    level = dict(sc, level=np.tile([GROUND_Z, 0.0, 0.0], (NMAX, 1)))
    flat = _device_step(eng, sc, NMAX, 3, 1.0, "flat", walk_entry=True)
    g = _device_step(eng, level, NMAX, 3, 1.0, "planes", ground="level")
    assert same(g, flat, NMAX) and np.array_equal(g[4][:NMAX], refs[(3, 1.0, "flat")][4])
    cfg = (3, 1.0, "planes")
    ref = refs[cfg]
    n = 65
    ip = _device_step(eng, sc, n, *cfg, in_place=True)
    _assert_is_ref(ip, ref, n)
    assert np.array_equal(ip[0][:, 12:], sc["tick"][:n, 12:])
    for stride in (12, 13):
        out = _device_step(eng, sc, n, *cfg, stride=stride)
        _assert_is_ref(out, ref, n)
        assert np.isnan(out[0][:n, 12:]).all() and all(np.isnan(a[n:]).all() for a in out[:4]) and (out[4][n:] == 0xFF).all()
    stream = torch.cuda.Stream()
    _assert_is_ref(_device_step(eng, sc, n, *cfg, stream=stream.cuda_stream), ref, n)
    for i in (0, 63, 64, 200, 256):
        _assert_is_ref(_device_step(eng, sc, 1, *cfg, sl=slice(i, i + 1)), ref, 1, rows=slice(i, i + 1))
    ground = sc["ground"].copy(); ground[37, 1] = np.nan
    so, Ro, fo, vo, to = _device_step(eng, dict(sc, bad=ground), n, *cfg, ground="bad")
    keep = np.arange(n) != 37
    assert PR.bits_equal(so[:n, 3:12], ref[0][:n, 3:12]) and PR.bits_equal(Ro[:n], ref[1][:n]) and PR.bits_equal(vo[:n], ref[3][:n])
    assert PR.bits_equal(fo[:n][keep], ref[2][:n][keep]) and np.array_equal(to[:n][keep], ref[4][:n][keep])
    stance = sc["contacts"][37] != 0
    assert np.isnan(fo[37, 2::3][stance]).all() and np.isfinite(fo[37, 2::3][~stance]).all() and np.array_equal(to[37], stance.astype(np.uint8))
    assert PR.bits_equal(np.delete(fo[37], [2, 5, 8, 11]), np.delete(ref[2][37], [2, 5, 8, 11]))


def test_step_refusals_leave_the_outputs_untouched(eng, scen):
    """every refusal of the walk step and a NULL touch_out: A1MPC_ERR_INVALID_ARGUMENT (1) from both entries, the argument named in a1mpc_last_error, before any launch;
    with ground given cfg's ground_z is not looked at; n == 0 is OK and writes nothing"""
    import torch
    sc, _ = _walkers(scen)
    n = 16
    L = eng.lib
    names = ["state_in", "R_world", "foot_abs", "grf_body", "contacts", "R_z", "foot_target"]
    keys = ("tick", "R", "foot", "grf", "contacts", "Rz", "target")
    ins = [_t(sc[k][:n]) for k in keys]
    outs = [_nan(n, 22), _nan(n, 9), _nan(n, 12), _nan(n, 12), _ff(n)]
    hins = [np.ascontiguousarray(sc[k][:n]) for k in keys]
    houts = [np.full((n, 22), np.nan), np.full((n, 9), np.nan), np.full((n, 12), np.nan), np.full((n, 12), np.nan), np.full((n, 4), 0xFF, np.uint8)]
    gr, hgr = _t(sc["ground"][:n]), np.ascontiguousarray(sc["ground"][:n])
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))

    def call(wc, n_, stride, ins_=ins, outs_=outs, hins_=hins, houts_=houts, ground=True):
        wp = None if wc is None else C.byref(wc)
        rd = L.a1mpc_ground_step_batch_device(eng._h, wp, n_, ptr(ins_[0]), stride, *[ptr(t) for t in ins_[1:5]], None, ptr(ins_[5]), ptr(ins_[6]), ptr(gr) if ground else None,
                                              *[ptr(t) for t in outs_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_ground_step_batch(eng._h, wp, n_, hp(hins_[0]), stride, *[hp(a) for a in hins_[1:5]], None, hp(hins_[5]), hp(hins_[6]), hp(hgr) if ground else None,
                                       *[hp(a) for a in houts_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    cfg = lambda **kw: eng.walk_config(**kw)
    nan, inf = float("nan"), float("inf")
    bad = [(cfg(substeps=0), n, 22, "substeps"), (cfg(substeps=65), n, 22, "substeps"), (cfg(dt=0.0), n, 22, "dt"), (cfg(dt=nan), n, 22, "dt"),
           (cfg(gravity_z=inf), n, 22, "gravity_z"), (cfg(), n, 14, "state_stride"), (cfg(), n, 0, "state_stride"), (cfg(), -1, 22, "negative n"), (cfg(), 513, 22, "max_batch"),
           (None, n, 22, "a1mpc_walk_config"), (cfg(swing_track=-0.1), n, 22, "swing_track"), (cfg(swing_track=1.5), n, 22, "swing_track"),
           (cfg(swing_track=nan), n, 22, "swing_track"), (cfg(swing_track=inf), n, 22, "swing_track")]
    for wc, n_, stride, word in bad:
        rd, md, rh, mh = call(wc, n_, stride)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    for gz in (nan, -inf):
        rd, md, rh, mh = call(cfg(flat_ground=1, ground_z=gz), n, 22, ground=False)
        assert rd == INVALID and rh == INVALID and "ground_z" in md and "ground_z" in mh
    for k, name in enumerate(names):
        for track in ((1.0, 0.25) if k >= 5 else (1.0,)):
            rd, md, rh, mh = call(cfg(swing_track=track), n, 22, ins_=[None if j == k else t for j, t in enumerate(ins)], hins_=[None if j == k else t for j, t in enumerate(hins)])
            assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for k, name in enumerate(["state_out", "R_world_out", "foot_abs_out", "foot_vel_body_out", "touch_out"]):
        rd, md, rh, mh = call(cfg(), n, 22, outs_=[None if j == k else t for j, t in enumerate(outs)], houts_=[None if j == k else t for j, t in enumerate(houts)])
        assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    rd, _, rh, _ = call(cfg(), 0, 22)
    assert rd == OK and rh == OK
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all().item() for o in outs[:4]) and (outs[4] == 0xFF).all().item() and all(np.isnan(o).all() for o in houts[:4]) and (houts[4] == 0xFF).all()
    rd, md, rh, mh = call(cfg(flat_ground=1, ground_z=nan), n, 22)   # (ground given: cfg's plane is not read; these arguments, accepted, do write)
    torch.cuda.synchronize()
    assert rd == OK and rh == OK and not torch.isnan(outs[1]).any().item() and not np.isnan(houts[3]).any() and (houts[4] <= 1).all() and (outs[4] <= 1).all().item(), (md, mh)


# ---- the sensors
def _sensor_cases(scen):
    """257 random robots as tick records with a commanded velocity and a touch byte (0, 1 or 200) on every leg, and the restatement in float64 and 80 bits, with and
    without the wrench: computed once, never changed"""
    if "sens" not in _SHARED:
        rng = np.random.default_rng(8500)
        sc = SR.random_robots(scen, rng, NMAX, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1))
        sc["vel"] = rng.normal(0, 1.0, (NMAX, 12))
        sc["touch"] = rng.choice(np.array([0, 1, 200], np.uint8), (NMAX, 4))
        refs = {}
        for ext in (False, True):
            for dt in (np.float64, np.longdouble):
                r = GR.sensors(sc["mass"], sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["vel"], sc["touch"], GL.TOUCH_FORCE, sc["ext"] if ext else None,
                               rho_opt=sc["rho_opt"], dtype=dt)
                for v in r.values():
                    v.setflags(write=False)
                refs[(ext, dt)] = r
        _SHARED["sens"] = (sc, refs)
    return _SHARED["sens"]


def _poisoned(rows, skip=()):
    return {k: None if k in skip else (_ff(rows, w) if k == "reach" else _nan(rows, w)) for k, w in WIDTHS.items()}


def _device_sensors(eng, sc, n, ext, touch="touch", force=GL.TOUCH_FORCE, stride=22, stream=None, sl=None, skip=(), walk_entry=False):
    """the device entry (walk_entry: a1mpc_walk_sensors_batch_device instead) on the first n robots (or the slice sl) -> numpy dict of n + TAIL rows, poisoned beforehand"""
    import torch
    sl = slice(0, n) if sl is None else sl
    ins = [_t(sc["tick"][sl, :stride]), _t(sc["R"][sl]), _t(sc["foot"][sl]), _t(sc["grf"][sl]), _t(sc["contacts"][sl])]
    ew = _t(sc["ext"][sl]) if ext else None
    out = _poisoned(n + TAIL, skip)
    o = [out[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force", "reach", "foot_pos_rel", "foot_vel_rel")]
    torch.cuda.synchronize()
    if walk_entry:
        eng.walk_sensors_device(n, ins[0], stride, *ins[1:], *o, d_ext_wrench=ew, d_foot_vel_body=_t(sc["vel"][sl]), rho_opt=sc["rho_opt"], stream=stream)
    else:
        eng.walk_sensors_touch_device(n, ins[0], stride, *ins[1:], *o, d_ext_wrench=ew, d_foot_vel_body=_t(sc["vel"][sl]), d_touch=None if touch is None else _t(sc[touch][sl]),
                                      touch_force=force, rho_opt=sc["rho_opt"], stream=stream)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _tail_untouched(out, n):
    return all(v is None or ((v[n:] == 0xFF).all() if k == "reach" else np.isnan(v[n:]).all()) for k, v in out.items())


def _same(a, b, rows=slice(None), skip=()):
    return all(SR.bits_equal(a[k][rows], b[k][rows]) for k in SR.OUTPUTS if k != "reach" and k not in skip and a[k] is not None and b[k] is not None) \
        and np.array_equal(a["reach"][rows], b["reach"][rows])


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sensors_device_and_host_entries_equal_the_restatement(eng, scen, n, ext):
    """the first n of 257 robots with a touch byte on every leg and touch_force = 60: BITS bit for bit (foot_force: touch_force exactly on a touched swing leg, +0 on an
    untouched one), NOISY within 4 E of the 80-bit evaluation, nothing beyond row n; the host entry returns the device entry's bits"""
    sc, refs = _sensor_cases(scen)
    r64, r80 = refs[(ext, np.float64)], refs[(ext, np.longdouble)]
    out = _device_sensors(eng, sc, n, ext)
    assert _tail_untouched(out, n) and not any(np.isnan(v[:n]).any() for k, v in out.items() if k != "reach")
    figs = SR.assert_is_ref(out, r64, r80, n, (n, ext))
    swing, hit = sc["contacts"][:n] == 0, sc["touch"][:n] != 0
    ff = out["foot_force"][:n]
    assert (ff[swing & hit] == GL.TOUCH_FORCE).all() and np.array_equal(ff[swing & ~hit].view(np.uint64), np.zeros((swing & ~hit).sum(), np.uint64))
    h = eng.walk_sensors_touch(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["vel"][:n], sc["touch"][:n], GL.TOUCH_FORCE,
                               sc["ext"][:n] if ext else None, rho_opt=sc["rho_opt"])
    assert _same(h, out, slice(0, n))
    print(f"n {n} wrench {ext}: " + ", ".join(f"{k} {e:.1e} (E {E:.1e})" for k, (e, E) in figs.items()))


def test_sensors_reduce_to_the_walk_sensors_and_structure(eng, scen):
    """touch NULL or touch_force 0: every output is a1mpc_walk_sensors_batch_device's bit for bit; with a force every output but foot_force is, and a stance leg's touch
    byte changes no bit; strides 12 / 13, the optional outputs NULL and a side stream give the same bits; robot i alone has the bits of robot i of the 257"""
    import torch
    sc, refs = _sensor_cases(scen)
    n = 65
    walk = _device_sensors(eng, sc, NMAX, True, walk_entry=True)
    assert _same(_device_sensors(eng, sc, NMAX, True, touch=None), walk) and _same(_device_sensors(eng, sc, NMAX, True, force=0.0), walk)
    full = _device_sensors(eng, sc, NMAX, True)
    assert not _same(full, walk) and _same(full, walk, skip=("foot_force",))
    stance = sc["contacts"] != 0
    flipped = sc["touch"].copy(); flipped[stance] = np.where(flipped[stance] != 0, 0, 1)
    assert _same(_device_sensors(eng, dict(sc, flipped=flipped), NMAX, True, touch="flipped"), full)
    for stride in (12, 13):
        o = _device_sensors(eng, sc, n, True, stride=stride)
        assert _same(o, full, slice(0, n)) and _tail_untouched(o, n)
    lean = _device_sensors(eng, sc, n, True, skip=("foot_pos_rel", "foot_vel_rel"))
    assert lean["foot_pos_rel"] is None and _same(lean, full, slice(0, n)) and _tail_untouched(lean, n)
    stream = torch.cuda.Stream()
    assert _same(_device_sensors(eng, sc, n, True, stream=stream.cuda_stream), full, slice(0, n))
    for i in (0, 63, 64, 200, 256):
        one = _device_sensors(eng, sc, 1, True, sl=slice(i, i + 1))
        assert all(SR.bits_equal(one[k][:1], full[k][i:i + 1]) for k in SR.OUTPUTS if k != "reach") and _tail_untouched(one, 1), i


def test_sensors_refusals_leave_the_outputs_untouched(eng, scen):
    """the walk sensors' refusals and a touch_force that is negative or not finite, from both entries, the argument named, before any launch; n == 0 is OK and writes
    nothing"""
    import torch
    sc, _ = _sensor_cases(scen)
    n = 16
    L = eng.lib
    keys = ("tick", "R", "foot", "grf", "contacts")
    ins = [_t(sc[k][:n]) for k in keys]
    vel, hvel, tc, htc = _t(sc["vel"][:n]), np.ascontiguousarray(sc["vel"][:n]), _t(sc["touch"][:n]), np.ascontiguousarray(sc["touch"][:n])
    outs = list(_poisoned(n).values())
    hins = [np.ascontiguousarray(sc[k][:n]) for k in keys]
    houts = [np.full((n, w), 0xFF, np.uint8) if k == "reach" else np.full((n, w), np.nan) for k, w in WIDTHS.items()]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))
    fix0, opt0 = np.ascontiguousarray(SR.A1_RHO_FIX).reshape(20), np.ascontiguousarray(sc["rho_opt"]).reshape(12)

    def call(n_, stride, ins_=ins, outs_=outs, hins_=hins, houts_=houts, fix=fix0, opt=opt0, h=eng._h, force=GL.TOUCH_FORCE):
        fp, op = (None if fix is None else hp(np.ascontiguousarray(fix, dtype=np.float64))), (None if opt is None else hp(np.ascontiguousarray(opt, dtype=np.float64)))
        rd = L.a1mpc_touch_sensors_batch_device(h, n_, ptr(ins_[0]), stride, *[ptr(t) for t in ins_[1:]], None, ptr(vel), ptr(tc), force, fp, op, *[ptr(t) for t in outs_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_touch_sensors_batch(h, n_, hp(hins_[0]), stride, *[hp(a) for a in hins_[1:]], None, hp(hvel), hp(htc), force, fp, op, *[hp(a) for a in houts_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    nanfix = fix0.copy(); nanfix[11] = np.nan
    nolen = fix0.copy(); nolen[8] = 0.0
    bad = [(dict(stride=14), "state_stride"), (dict(n_=-1), "negative n"), (dict(fix=None), "null rho_fix"), (dict(opt=None), "null rho_opt"), (dict(fix=nanfix), "rho_fix"),
           (dict(fix=nolen), "upper leg"), (dict(h=None), "null handle"), (dict(force=-1.0), "touch_force"), (dict(force=float("nan")), "touch_force"),
           (dict(force=float("inf")), "touch_force")]
    for kw, word in bad:
        kw = dict(kw); n_ = kw.pop("n_", n); stride = kw.pop("stride", 22)
        rd, md, rh, mh = call(n_, stride, **kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    rd, md, rh, mh = call(513, 22)
    assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    for k, name in enumerate(["state", "R_world", "foot_abs", "grf_body", "contacts"]):
        rd, md, rh, mh = call(n, 22, ins_=[None if j == k else t for j, t in enumerate(ins)], hins_=[None if j == k else t for j, t in enumerate(hins)])
        assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for k, name in enumerate(["quat_out", "imu_acc_raw_out", "imu_gyro_raw_out", "joint_pos_out", "joint_vel_out", "foot_force_out", "reach_out"]):
        rd, md, rh, mh = call(n, 22, outs_=[None if j == k else t for j, t in enumerate(outs)], houts_=[None if j == k else t for j, t in enumerate(houts)])
        assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    rd, _, rh, _ = call(0, 22)
    assert rd == OK and rh == OK
    torch.cuda.synchronize()
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a
    untouched = lambda a: bool((host(a) == 0xFF).all()) if host(a).dtype == np.uint8 else bool(np.isnan(host(a)).all())
    assert all(untouched(o) for o in outs) and all(untouched(o) for o in houts)
    rd, _, rh, _ = call(n, 22)   # (the same arguments, accepted, do write)
    torch.cuda.synchronize()
    assert rd == OK and rh == OK and not any(untouched(o) for o in outs) and not any(untouched(o) for o in houts)


# ---- the closed loops on the device
LOOPS = dict(ramp=(True, 0.0), touch=(False, GL.TOUCH_FORCE), ramp_touch=(True, GL.TOUCH_FORCE))   # (a plane per robot?, touch_force)


def _loop_planes(sc, n, sloped):
    """robots 0 .. 3 are the CPU loop's ((+s, 0), (-s, 0), (0, +s), flat); robot b >= 4 stands on the pattern of robot b % 4 with a slope between 0.2 s and 0.5 s.
    (The slope s was chosen on robots 0 .. 3.  Robot 12 wobbles most when the walk starts -- tilt 0.122 on flat ground, the others 0.10 at most -- and on 0.77 s the CPU
    loop of all 17 has it at 0.196, next to the bar of 0.2; on these planes the CPU loop keeps every robot at or under 0.16.)"""
    g = np.zeros((n, 3))
    if sloped:
        g[:4] = GL.ramp_planes(sc, GL.RAMP_SLOPE)
        scale = np.random.default_rng(8600).uniform(0.2, 0.5, n)
        for b in range(4, n):
            g[b, 1:] = g[b % 4, 1:] * scale[b]
        pos = sc["state"][:n, 3:5]
        g[4:, 0] = -(g[4:, 1] * pos[4:, 0] + g[4:, 2] * pos[4:, 1])
    return g


@pytest.mark.parametrize("which", list(LOOPS))
def test_closed_loop_touch_sensors_tick_ground_step_on_the_device(eng, pkg, oracle, scen, which):
    """17 perturbed standing robots, h = 10, cold solves, the schedule of tests/walk_loop.py: a1mpc_touch_sensors_batch_device -> a1mpc_control_tick_sensors_device ->
    a1mpc_ground_step_batch_device (in place, fed the tick's grf, contacts, R_z and foot_pos_target_last_time, writing the touch bytes the next tick's sensors read), all
    on one stream without a host synchronisation between the first launch and the last; every tick's plant state, sensors, contacts and plan are copied into a history on
    that stream.  ramp: the planes of _loop_planes, touch_force 0; touch: flat, touch_force 60; ramp_touch: both.  conditions_hold (height above the robot's own plane)
    stays empty on every tick, every touchdown is on the robot's own plane within 1e-12, and against the same loop on the CPU (robots 0 .. 3): the end state's pos, v and
    angles within 1e-4, omega within 1e-3, and the early-contact ticks identical"""
    import torch
    E = pkg.engine
    sloped, force = LOOPS[which]
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
    planes = _loop_planes(sc, n, sloped)
    assert eng.horizon == SL.H and eng.cfg.warm_start == 0 and eng.cfg.mass == sc["params"]["mass"]
    L = eng.lib
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm))
    assert prm.control_dt == SL.CONTROL_DT and prm.contact.use_terrain_adapt == 1 and prm.contact.foot_force_low == 30.0
    state, R, foot = _t(sc["state"]), _t(sc["R"]), _t(sc["foot"])
    grf_eq, ct_all = _t(sc["grf_eq"]), _t(sc["contact"])
    ground = _t(planes)
    w = tick_world(n, dev, WL.COUNTERS)
    Z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    syn = dict(quat=Z(n, 4), imu_acc_raw=Z(n, 3), imu_gyro_raw=Z(n, 3), joint_pos=Z(n, 12), joint_vel=Z(n, 12), foot_force=Z(n, 4), reach=Z(n, 4, dt=torch.uint8))
    front = dict(R_world=Z(n, 9), R_z=Z(n, 9), root_euler=Z(n, 3), root_ang_vel=Z(n, 3), imu_acc=Z(n, 3), imu_ang_vel=Z(n, 3), root_lin_vel_d=Z(n, 3), root_ang_vel_d=Z(n, 3),
                 root_pos_d_z=Z(n), movement_mode=Z(n, dt=torch.uint8), mpc_active=Z(n, dt=torch.uint8))
    cs = {k: _t(v) for k, v in E.Engine.command_state(n).items() if k != "root_euler_d"}   # (root_euler_d is the tick world's)
    inp = dict(joint_pos=syn["joint_pos"], joint_vel=syn["joint_vel"], foot_force=syn["foot_force"], gait_counter_speed=_t(np.full((n, 4), WL.COUNTER_SPEED)),
               torques_gravity=Z(n, 12), **front)
    stick = dict(cmd=Z(n, 6), mode_toggle=Z(n, dt=torch.uint8))   # (held here: a TickSensors keeps addresses, not tensors)
    walk_cmd = Z(n, 6); walk_cmd[:, 0] = WL.SPEED
    one, zero = torch.ones(n, dtype=torch.uint8, device=dev), Z(n, dt=torch.uint8)
    ts = eng.tick_sensors(sensor=eng.sensor_config(imu_window=SL.IMU_WINDOW), quat=syn["quat"], imu_acc_raw=syn["imu_acc_raw"], imu_gyro_raw=syn["imu_gyro_raw"], **stick, **cs)
    bf = tick_buffers(E, inp, w)
    fvb = Z(n, 12)
    touch = torch.ones((n, 4), dtype=torch.uint8, device=dev)   # (the unstepped plant stands on all four feet)
    T = WL.PRIME + WL.STAND + WL.WALK
    hist = dict(state=Z(T, n, 12), R=Z(T, n, 9), foot=Z(T, n, 12), status=Z(T, n, dt=torch.int32), reach=Z(T, n, 4, dt=torch.uint8), grf=Z(T, n, 12),
                contacts=Z(T, n, 4, dt=torch.uint8), plan=Z(T, n, 4, dt=torch.uint8), mode=Z(T, n, dt=torch.uint8), sensors=Z(T, n, 38))
    stream = torch.cuda.Stream()
    wc = eng.walk_config(dt=SL.CONTROL_DT, swing_track=1.0)
    torch.cuda.synchronize()
    for t in range(T):
        first = t <= WL.PRIME     # the priming ticks and the first closed tick read the equilibrium forces, all legs in stance
        if t in (WL.PRIME + WL.STAND, WL.PRIME + WL.STAND + 1):
            with torch.cuda.stream(stream):
                stick["mode_toggle"].copy_(one if t == WL.PRIME + WL.STAND else zero); stick["cmd"].copy_(walk_cmd)
        eng.walk_sensors_touch_device(n, state, 12, R, foot, grf_eq if first else w["outs"]["grf"], ct_all if first else w["u8"]["contacts"], syn["quat"], syn["imu_acc_raw"],
                                      syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], syn["reach"], d_foot_vel_body=fvb, d_touch=touch,
                                      touch_force=force, stream=stream.cuda_stream)
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=stream.cuda_stream)
        if t >= WL.PRIME:
            eng.walk_step_ground_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], front["R_z"], w["state"]["foot_pos_target_last_time"], fvb, touch,
                                        d_ground=ground, walk=wc, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            hist["state"][t].copy_(state); hist["R"][t].copy_(R); hist["foot"][t].copy_(foot); hist["status"][t].copy_(w["i32"]["status"]); hist["reach"][t].copy_(syn["reach"])
            hist["grf"][t].copy_(w["outs"]["grf"]); hist["contacts"][t].copy_(w["u8"]["contacts"]); hist["plan"][t].copy_(w["u8"]["plan_contacts"])
            hist["mode"][t].copy_(front["movement_mode"])
            hist["sensors"][t].copy_(torch.cat([syn[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")], 1))
    torch.cuda.synchronize()
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    H = {k: v.cpu().numpy() for k, v in hist.items()}
    assert np.array_equal(H["state"][WL.PRIME - 1], sc["state"])   # (the plant was not stepped while the EKF was primed)
    w0 = WL.PRIME + WL.STAND
    assert not H["mode"][:w0].any() and (H["mode"][w0:] == 1).all()
    for t in range(WL.PRIME, T):
        finite = np.isfinite(H["sensors"][t]).all() and np.isfinite(H["grf"][t]).all() and np.isfinite(H["state"][t]).all()
        bad = SL.conditions_hold(GL.above_plane(planes, H["state"][t]), H["reach"][t], H["status"][t], finite)
        assert not bad, (t, bad)
    walk = {k: H[k][w0:] for k in ("contacts", "plan", "foot", "state", "R")}
    td, h = GL.touchdown_heights(walk, planes)
    early = GL.early_contacts(walk)
    print(f"{which} on the device, {WL.WALK} ticks, {n} robots: {len(td)} touchdowns off their planes by {np.abs(td).max():.1e} at most, lowest foot {h.min():.1e}; "
          f"{len(early)} early-contact ticks")
    assert len(td) >= 12 * n and np.abs(td).max() <= GL.TOUCHDOWN and h.min() >= -GL.TOUCHDOWN
    if force == 0.0:
        assert not early and len(td) == 12 * n
    else:
        assert min(sum(1 for e in early if e[1] == b) for b in range(n)) >= 1
    # the same loop on the CPU, the first 4 robots
    if which not in _SHARED:
        cpu = GL.GroundLoop(oracle, scen, sc, 4, ground=planes[:4], touch_force=force)
        _SHARED[which] = (GL.run(cpu, 4), cpu.x.copy())
    (chist, failed), x = _SHARED[which]
    assert not failed, failed[:3]
    d = lambda a, b: float(np.abs(a - b).max())
    end = H["state"][-1]
    figs = dict(pos=d(end[:4, 3:6], x[:, 3:6]), v=d(end[:4, 9:12], x[:, 9:12]), angles=d(end[:4, 0:3], x[:, 0:3]), omega=d(end[:4, 6:9], x[:, 6:9]))
    print(f"GPU loop against the CPU loop after {T - WL.PRIME} closed ticks:", ", ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert [e for e in early if e[1] < 4] == GL.early_contacts(chist)
    assert figs["pos"] <= 1e-4 and figs["v"] <= 1e-4 and figs["angles"] <= 1e-4 and figs["omega"] <= 1e-3
