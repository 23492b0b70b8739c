"""GPU: a1mpc_walk_step_batch(_device) and a1mpc_walk_sensors_batch(_device) -- the plant step with swing feet that move and a flat ground, and the sensors that know it.
Yardsticks: the elementwise numpy restatements of tests/walk_ref.py (the step's pos, R, v, omega, feet and foot_vel_body BIT FOR BIT, its angles within 1e-12; the sensors
by the rule of tests/sensor_synthesis_ref.py); the existing device entries, which the new ones must reduce to bit for bit; the device's own leg stage; and the trot
walk sensors -> tick -> walk step on one stream against the same loop on the CPU (tests/walk_loop.py).  One handle of 512 robots, gazebo parameter set, h = 10, cold solves."""
import ctypes as C
import itertools

import numpy as np
import pytest

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
STEP_CONFIGS = list(itertools.product((0.0, 0.5, 1.0), (0, 1), (1, 4)))   # swing_track, flat_ground, substeps
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


@pytest.fixture(scope="module")
def eng(pkg, scen):
    e = _engine(pkg, scen.scenario_stand(), 512, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


def _walkers(scen):
    """257 random walkers as tick records and the restatement of every step configuration (a wrench where the sub-steps are 4): computed once, never changed"""
    if "walk" not in _SHARED:
        rng = np.random.default_rng(7400)
        sc = WR.random_walkers(scen, rng, NMAX)
        sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1))
        refs = {}
        for track, ground, sub in STEP_CONFIGS:
            refs[(track, ground, sub)] = WR.step(sc["params"], sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], sc["ext"] if sub == 4 else None,
                                                 0.0025, sub, swing_track=track, flat_ground=ground, ground_z=GROUND_Z)
            for a in refs[(track, ground, sub)]:
                a.setflags(write=False)
        _SHARED["walk"] = (sc, refs)
    return _SHARED["walk"]


def _walk_cfg(eng, track, ground, sub):
    return eng.walk_config(substeps=sub, swing_track=track, flat_ground=ground, ground_z=GROUND_Z)


def _device_step(eng, sc, n, track, ground, sub, stride=22, stream=None, in_place=False, sl=None, with_targets=True):
    """the device entry on the first n robots (or the slice sl) -> numpy (state (n + TAIL, stride), R, foot, foot_vel_body): NaN-poisoned outputs, or in place"""
    import torch
    sl = slice(0, n) if sl is None else sl
    st = _t(sc["tick"][sl, :stride]); R = _t(sc["R"][sl]); foot = _t(sc["foot"][sl]); grf = _t(sc["grf"][sl]); ct = _t(sc["contacts"][sl])
    Rz, tg = (_t(sc["Rz"][sl]), _t(sc["target"][sl])) if with_targets else (None, None)
    ew = _t(sc["ext"][sl]) if sub == 4 else None
    so, Ro, fo = (None, None, None) if in_place else (_nan(n + TAIL, stride), _nan(n + TAIL, 9), _nan(n + TAIL, 12))
    vo = _nan(n + TAIL, 12)
    torch.cuda.synchronize()
    eng.walk_step_device(n, st, stride, R, foot, grf, ct, Rz, tg, vo, ew, so, Ro, fo, walk=_walk_cfg(eng, track, ground, sub), stream=stream)
    torch.cuda.synchronize()
    if in_place:
        so, Ro, fo = st, R, foot
    return so.cpu().numpy(), Ro.cpu().numpy(), fo.cpu().numpy(), vo.cpu().numpy()


def _assert_is_ref(out, ref, n, rows=slice(None)):
    so, Ro, fo, vo = out
    assert PR.bits_equal(so[:n, 3:12], ref[0][rows][:n, 3:12]) and PR.bits_equal(Ro[:n], ref[1][rows][:n]) and PR.bits_equal(fo[:n], ref[2][rows][:n])
    assert PR.bits_equal(vo[:n], ref[3][rows][:n])
    worst = float(np.abs(so[:n, :3] - ref[0][rows][:n, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_step_device_and_host_entries_equal_the_restatement_bit_for_bit(eng, scen, n):
    """the first n of 257 robots, swing_track 0 / 0.5 / 1, the ground off and on, 1 sub-step without a wrench and 4 with one: the device entry writes the restatement's
    bits, nothing beyond row n and nothing into words [12:22) of the tick records; the host entry returns the device entry's bits"""
    sc, refs = _walkers(scen)
    worst = 0.0
    for track, ground, sub in STEP_CONFIGS:
        out = _device_step(eng, sc, n, track, ground, sub)
        assert all(np.isnan(a[n:]).all() for a in out) and np.isnan(out[0][:n, 12:]).all() and not any(np.isnan(a[:n, :w]).any() for a, w in zip(out, (12, 9, 12, 12)))
        worst = max(worst, _assert_is_ref(out, refs[(track, ground, sub)], n))
        h = eng.walk_step(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n], sc["target"][:n], sc["ext"][:n] if sub == 4 else None,
                          walk=_walk_cfg(eng, track, ground, sub))
        assert PR.bits_equal(h["state"][:, :12], out[0][:n, :12]) and PR.bits_equal(h["R"], out[1][:n]) and PR.bits_equal(h["foot"], out[2][:n])
        assert PR.bits_equal(h["foot_vel_body"], out[3][:n]) and np.array_equal(h["state"][:, 12:], sc["tick"][:n, 12:])
    print(f"n {n}: {len(STEP_CONFIGS)} configurations, device and host entries carry the restatement's bits; angles within {worst:.1e}")


def test_step_in_place_strides_streams_and_a_robot_alone(eng, scen):
    """in place == out of place, the command half of the tick records surviving; strides 12 and 13 give the same bits; a side stream; robot i alone has the bits of robot
    i of the 257; a NaN target on every stance leg and a NaN force on every swing leg change no bit; a NaN pos stays with its robot"""
    import torch
    sc, refs = _walkers(scen)
    cfg = (1.0, 1, 4)
    ref = refs[cfg]
    n = 65
    ip = _device_step(eng, sc, n, *cfg, in_place=True)
    _assert_is_ref(ip, ref, n)
    assert np.array_equal(ip[0][:, 12:], sc["tick"][:n, 12:])
    for stride in (12, 13):
        out = _device_step(eng, sc, n, *cfg, stride=stride)
        _assert_is_ref(out, ref, n)
        assert np.isnan(out[0][:n, 12:]).all() and all(np.isnan(a[n:]).all() for a in out)
    stream = torch.cuda.Stream()
    _assert_is_ref(_device_step(eng, sc, n, *cfg, stream=stream.cuda_stream), ref, n)
    for i in (0, 63, 64, 200, 256):
        _assert_is_ref(_device_step(eng, sc, 1, *cfg, sl=slice(i, i + 1)), ref, 1, rows=slice(i, i + 1))
    target, grf = sc["target"].copy(), sc["grf"].copy()
    for i, l in np.argwhere(sc["contacts"][:n] != 0):
        target[i, 3 * l + (i + l) % 3] = np.nan
    for i, l in np.argwhere(sc["contacts"][:n] == 0):
        grf[i, 3 * l + (i + l) % 3] = np.nan
    _assert_is_ref(_device_step(eng, dict(sc, target=target, grf=grf), n, *cfg), ref, n)
    tick = sc["tick"].copy(); tick[37, 5] = np.nan
    so, Ro, fo, vo = _device_step(eng, dict(sc, tick=tick), n, *cfg)
    keep = np.arange(n) != 37
    assert PR.bits_equal(so[:n][keep, 3:12], ref[0][:n][keep, 3:12]) and PR.bits_equal(Ro[:n], ref[1][:n]) and PR.bits_equal(fo[:n][keep], ref[2][:n][keep])
    assert PR.bits_equal(vo[:n], ref[3][:n]) and np.isnan(so[37, 5]) and np.isfinite(np.delete(so[37, :12], 5)).all()
    stance = sc["contacts"][37] != 0
    assert np.isnan(fo[37, 2::3][stance]).all() and np.isfinite(fo[37, 2::3][~stance]).all()


def test_the_walk_step_reduces_to_the_plant_step_on_the_device(eng, scen):
    """swing_track = 0, flat_ground = 0, R_z and foot_target NULL: state, R and the feet are a1mpc_plant_step_batch_device's bit for bit at 1 and 4 sub-steps;
    foot_vel_body is all +0 bits"""
    import torch
    sc, _ = _walkers(scen)
    n = NMAX
    for sub in (1, 4):
        w = _device_step(eng, sc, n, 0.0, 0, sub, with_targets=False)
        st = _t(sc["tick"]); so, Ro, fo = _nan(n, 22), _nan(n, 9), _nan(n, 12)
        eng.plant_step_device(n, st, 22, _t(sc["R"]), _t(sc["foot"]), _t(sc["grf"]), _t(sc["contacts"]), _t(sc["ext"]) if sub == 4 else None, so, Ro, fo,
                              plant=eng.plant_config(substeps=sub))
        torch.cuda.synchronize()
        assert PR.bits_equal(w[0][:n], so.cpu().numpy()) and PR.bits_equal(w[1][:n], Ro.cpu().numpy()) and PR.bits_equal(w[2][:n], fo.cpu().numpy())
        assert np.array_equal(w[3][:n].view(np.uint64), np.zeros((n, 12), np.uint64))


def test_step_refusals_leave_the_outputs_untouched(eng, scen):
    """every refusal of the header: A1MPC_ERR_INVALID_ARGUMENT (1) from both entries, the field named in a1mpc_last_error, before any launch; n == 0 is OK and writes
    nothing; swing_track == 0 with NULL R_z and foot_target is accepted"""
    import torch
    sc, _ = _walkers(scen)
    n = 16
    L = eng.lib
    names = ["state_in", "R_world", "foot_abs", "grf_body", "contacts", "R_z", "foot_target"]
    ins = [_t(sc[k][:n]) for k in ("tick", "R", "foot", "grf", "contacts", "Rz", "target")]
    outs = [_nan(n, 22), _nan(n, 9), _nan(n, 12), _nan(n, 12)]
    hins = [np.ascontiguousarray(sc[k][:n]) for k in ("tick", "R", "foot", "grf", "contacts", "Rz", "target")]
    houts = [np.full((n, 22), np.nan), np.full((n, 9), np.nan), np.full((n, 12), np.nan), np.full((n, 12), np.nan)]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))

    def call(wc, n_, stride, ins_=ins, outs_=outs, hins_=hins, houts_=houts):
        wp = None if wc is None else C.byref(wc)
        rd = L.a1mpc_walk_step_batch_device(eng._h, wp, n_, ptr(ins_[0]), stride, *[ptr(t) for t in ins_[1:5]], None, ptr(ins_[5]), ptr(ins_[6]), *[ptr(t) for t in outs_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_walk_step_batch(eng._h, wp, n_, hp(hins_[0]), stride, *[hp(a) for a in hins_[1:5]], None, hp(hins_[5]), hp(hins_[6]), *[hp(a) for a in houts_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    cfg = lambda **kw: eng.walk_config(**kw)
    nan, inf = float("nan"), float("inf")
    bad = [(cfg(substeps=0), n, 22, "substeps"), (cfg(substeps=65), n, 22, "substeps"), (cfg(dt=0.0), n, 22, "dt"), (cfg(dt=nan), n, 22, "dt"),
           (cfg(gravity_z=inf), n, 22, "gravity_z"), (cfg(), n, 14, "state_stride"), (cfg(), n, 0, "state_stride"), (cfg(), -1, 22, "negative n"), (cfg(), 513, 22, "max_batch"),
           (None, n, 22, "a1mpc_walk_config"), (cfg(swing_track=-0.1), n, 22, "swing_track"), (cfg(swing_track=1.5), n, 22, "swing_track"),
           (cfg(swing_track=nan), n, 22, "swing_track"), (cfg(swing_track=inf), n, 22, "swing_track"), (cfg(flat_ground=1, ground_z=nan), n, 22, "ground_z"),
           (cfg(flat_ground=1, ground_z=-inf), n, 22, "ground_z")]
    for wc, n_, stride, word in bad:
        rd, md, rh, mh = call(wc, n_, stride)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    for k, name in enumerate(names):
        for track in ((1.0, 0.25) if k >= 5 else (1.0,)):
            rd, md, rh, mh = call(cfg(swing_track=track), n, 22, ins_=[None if j == k else t for j, t in enumerate(ins)], hins_=[None if j == k else t for j, t in enumerate(hins)])
            assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for k, name in enumerate(["state_out", "R_world_out", "foot_abs_out", "foot_vel_body_out"]):
        rd, md, rh, mh = call(cfg(), n, 22, outs_=[None if j == k else t for j, t in enumerate(outs)], houts_=[None if j == k else t for j, t in enumerate(houts)])
        assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    rd, _, rh, _ = call(cfg(), 0, 22)
    assert rd == OK and rh == OK
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all().item() for o in outs) and all(np.isnan(o).all() for o in houts)
    rd, md, rh, mh = call(cfg(flat_ground=0, ground_z=nan), n, 22)   # (the ground off: ground_z is not looked at; these arguments, accepted, do write)
    torch.cuda.synchronize()
    assert rd == OK and rh == OK and not torch.isnan(outs[1]).any().item() and not np.isnan(houts[3]).any(), (md, mh)
    rd, md, rh, mh = call(cfg(swing_track=0.0), n, 22, ins_=ins[:5] + [None, None], hins_=hins[:5] + [None, None])
    assert rd == OK and rh == OK, (md, mh)
    torch.cuda.synchronize()


# ---- the sensors
def _sensor_cases(scen):
    """257 random robots as tick records (all four quaternion branches and all 16 contact patterns in every 16, reachable feet) with a commanded velocity on every leg, and
    the restatement in float64 and 80 bits, with and without the wrench: computed once, never changed"""
    if "sens" not in _SHARED:
        rng = np.random.default_rng(7500)
        sc = SR.random_robots(scen, rng, NMAX, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1))
        sc["vel"] = rng.normal(0, 1.0, (NMAX, 12))
        refs = {}
        for ext in (False, True):
            for dt in (np.float64, np.longdouble):
                r = WR.sensors(sc["mass"], sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["vel"], sc["ext"] if ext else None, rho_opt=sc["rho_opt"], dtype=dt)
                for v in r.values():
                    v.setflags(write=False)
                refs[(ext, dt)] = r
        _SHARED["sens"] = (sc, refs)
    return _SHARED["sens"]


def _poisoned(rows, skip=()):
    import torch
    return {k: None if k in skip else (torch.full((rows, w), 0xFF, dtype=torch.uint8, device=_dev()) if k == "reach" else _nan(rows, w)) for k, w in WIDTHS.items()}


def _device_sensors(eng, sc, n, ext, vel="vel", stride=22, stream=None, sl=None, skip=(), synthesis=False):
    """the device entry (synthesis: a1mpc_sensor_synthesis_batch_device instead) on the first n robots (or the slice sl) -> numpy dict of n + TAIL rows, poisoned beforehand"""
    import torch
    sl = slice(0, n) if sl is None else sl
    ins = [_t(sc["tick"][sl, :stride]), _t(sc["R"][sl]), _t(sc["foot"][sl]), _t(sc["grf"][sl]), _t(sc["contacts"][sl])]
    ew = _t(sc["ext"][sl]) if ext else None
    out = _poisoned(n + TAIL, skip)
    o = [out[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force", "reach", "foot_pos_rel", "foot_vel_rel")]
    torch.cuda.synchronize()
    if synthesis:
        eng.sensor_synthesis_device(n, ins[0], stride, *ins[1:], *o, d_ext_wrench=ew, rho_opt=sc["rho_opt"], stream=stream)
    else:
        eng.walk_sensors_device(n, ins[0], stride, *ins[1:], *o, d_ext_wrench=ew, d_foot_vel_body=None if vel is None else _t(sc[vel][sl]), rho_opt=sc["rho_opt"], stream=stream)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _tail_untouched(out, n):
    return all(v is None or ((v[n:] == 0xFF).all() if k == "reach" else np.isnan(v[n:]).all()) for k, v in out.items())


def _same(a, b, rows=slice(None)):
    return all(SR.bits_equal(a[k][rows], b[k][rows]) for k in SR.OUTPUTS if k != "reach" and a[k] is not None and b[k] is not None) and np.array_equal(a["reach"][rows], b["reach"][rows])


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sensors_device_and_host_entries_equal_the_restatement(eng, scen, n, ext):
    """the first n of 257 robots with a commanded velocity on every leg: BITS bit for bit (a swing leg's foot_vel_rel IS the command), NOISY within 4 E of the 80-bit
    evaluation, reach == 0, nothing beyond row n; the host entry returns the device entry's bits"""
    sc, refs = _sensor_cases(scen)
    r64, r80 = refs[(ext, np.float64)], refs[(ext, np.longdouble)]
    out = _device_sensors(eng, sc, n, ext)
    assert _tail_untouched(out, n) and not any(np.isnan(v[:n]).any() for k, v in out.items() if k != "reach")
    figs = SR.assert_is_ref(out, r64, r80, n, (n, ext))
    swing = np.repeat(sc["contacts"][:n] == 0, 3, axis=1)
    assert SR.bits_equal(out["foot_vel_rel"][:n][swing], sc["vel"][:n][swing])
    h = eng.walk_sensors(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["vel"][:n], sc["ext"][:n] if ext else None, rho_opt=sc["rho_opt"])
    assert _same(h, out, slice(0, n))
    print(f"n {n} wrench {ext}: " + ", ".join(f"{k} {e:.1e} (E {E:.1e})" for k, (e, E) in figs.items()))


def test_sensors_reduce_to_the_synthesis_and_structure(eng, scen):
    """foot_vel_body NULL or all +0: every output is a1mpc_sensor_synthesis_batch_device's bit for bit; a NaN command on every stance leg changes no bit; strides 12 / 13,
    the optional outputs NULL and a side stream give the same bits; robot i alone has the bits of robot i of the 257"""
    import torch
    sc, refs = _sensor_cases(scen)
    n = 65
    syn = _device_sensors(eng, sc, NMAX, True, synthesis=True)
    assert _same(_device_sensors(eng, sc, NMAX, True, vel=None), syn) and _same(_device_sensors(eng, dict(sc, zero=np.zeros((NMAX, 12))), NMAX, True, vel="zero"), syn)
    full = _device_sensors(eng, sc, NMAX, True)
    assert not _same(full, syn)
    vel = sc["vel"].copy(); vel[np.repeat(sc["contacts"] != 0, 3, axis=1)] = np.nan
    assert _same(_device_sensors(eng, dict(sc, vel=vel), NMAX, True), full)
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
    """the synthesis's refusals from both entries, the argument named, before any launch; n == 0 is OK and writes nothing"""
    import torch
    sc, _ = _sensor_cases(scen)
    n = 16
    L = eng.lib
    ins = [_t(sc["tick"][:n]), _t(sc["R"][:n]), _t(sc["foot"][:n]), _t(sc["grf"][:n]), _t(sc["contacts"][:n])]
    vel, hvel = _t(sc["vel"][:n]), np.ascontiguousarray(sc["vel"][:n])
    outs = list(_poisoned(n).values())
    hins = [np.ascontiguousarray(sc[k][:n]) for k in ("tick", "R", "foot", "grf", "contacts")]
    houts = [np.full((n, w), 0xFF, np.uint8) if k == "reach" else np.full((n, w), np.nan) for k, w in WIDTHS.items()]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))
    fix0, opt0 = np.ascontiguousarray(SR.A1_RHO_FIX).reshape(20), np.ascontiguousarray(sc["rho_opt"]).reshape(12)

    def call(n_, stride, ins_=ins, outs_=outs, hins_=hins, houts_=houts, fix=fix0, opt=opt0, h=eng._h):
        fp, op = (None if fix is None else hp(np.ascontiguousarray(fix, dtype=np.float64))), (None if opt is None else hp(np.ascontiguousarray(opt, dtype=np.float64)))
        rd = L.a1mpc_walk_sensors_batch_device(h, n_, ptr(ins_[0]), stride, *[ptr(t) for t in ins_[1:]], None, ptr(vel), fp, op, *[ptr(t) for t in outs_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_walk_sensors_batch(h, n_, hp(hins_[0]), stride, *[hp(a) for a in hins_[1:]], None, hp(hvel), fp, op, *[hp(a) for a in houts_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    nanfix = fix0.copy(); nanfix[11] = np.nan
    nolen = fix0.copy(); nolen[8] = 0.0
    bad = [(dict(stride=14), "state_stride"), (dict(n_=-1), "negative n"), (dict(fix=None), "null rho_fix"), (dict(opt=None), "null rho_opt"), (dict(fix=nanfix), "rho_fix"),
           (dict(fix=nolen), "upper leg"), (dict(h=None), "null handle")]
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


def test_leg_stage_gives_the_commanded_velocity_back(eng, scen):
    """the synthesised joint_pos and joint_vel through a1mpc_leg_state_batch_device: on the swing legs foot_vel_rel is foot_vel_body within 4 E of the restated round
    trip's 80-bit evaluation (J(q) joint_vel, itself the command to 1e-13)"""
    import torch
    sc, refs = _sensor_cases(scen)
    n = NMAX
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
    ins = [_t(sc["tick"]), _t(sc["R"]), _t(sc["foot"]), _t(sc["grf"]), _t(sc["contacts"])]
    syn = _poisoned(n)
    z3 = torch.zeros((n, 3), dtype=torch.float64, device=_dev())
    leg = {k: _nan(n, w) for k, w in (("rel", 12), ("Jb", 36), ("vrel", 12), ("abs", 12))}
    stream = torch.cuda.Stream()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dp_ = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    torch.cuda.synchronize()
    eng.walk_sensors_device(n, ins[0], 22, *ins[1:], syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], syn["reach"],
                            d_foot_vel_body=_t(sc["vel"]), rho_opt=sc["rho_opt"], stream=stream.cuda_stream)
    fix, opt = np.ascontiguousarray(SR.A1_RHO_FIX), np.ascontiguousarray(sc["rho_opt"])
    rc = eng.lib.a1mpc_leg_state_batch_device(eng._h, n, ptr(syn["joint_pos"]), ptr(syn["joint_vel"]), ptr(ins[1]), ptr(z3), ptr(z3), dp_(fix), dp_(opt), ptr(leg["rel"]),
                                              ptr(leg["Jb"]), ptr(leg["vrel"]), ptr(leg["abs"]), None, None, None, C.c_void_p(stream.cuda_stream))
    assert rc == 0, eng.lib.a1mpc_last_error()
    torch.cuda.synchronize()
    got = leg["vrel"].cpu().numpy()
    E = float(np.abs(trip[np.float64].astype(np.longdouble) - trip[np.longdouble])[swing].max())
    err = float(np.abs(got.astype(np.longdouble) - trip[np.longdouble])[swing].max())
    print(f"the leg stage's foot_vel_rel on the swing legs against the commanded velocity: {err:.1e} (E {E:.1e})")
    assert err <= SR.FACTOR * E


# ---- the trot on the device
def test_trot_walk_sensors_tick_walk_step_on_the_device(eng, pkg, oracle, scen):
    """17 perturbed standing robots (sensor_loop.perturbed_standing_robots), h = 10, cold solves, the schedule of tests/walk_loop.py: 10 priming ticks of
    a1mpc_walk_sensors_batch_device -> a1mpc_control_tick_sensors_device on the unstepped plant, 100 closed ticks standing, 360 with the mode toggle on the first and a
    stick command of 0.2 m/s; a closed tick ends with a1mpc_walk_step_batch_device (swing_track 1, the ground on at 0) in place, fed the tick's grf, contacts, R_z and
    foot_pos_target_last_time.  All on one stream, enqueued without a host synchronisation; the stick and the toggle change by copies on that stream; each tick's plant
    state, sensors and status are copied into a history on the same stream and looked at afterwards.  Every per-tick and whole-walk condition of the CPU trot
    (tests/test_walk_host.py) on all 17 robots; the end state of the first 4 is the CPU loop's: pos, v, angles within 1e-4, omega within 1e-3"""
    import torch
    E = pkg.engine
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
    assert eng.horizon == SL.H and eng.cfg.warm_start == 0 and eng.cfg.mass == sc["params"]["mass"]
    L = eng.lib
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm))
    assert prm.control_dt == SL.CONTROL_DT and np.array_equal(np.array(prm.gait.default_foot_pos), SL.DEFAULT_FOOT_POS)
    state, R, foot = _t(sc["state"]), _t(sc["R"]), _t(sc["foot"])
    grf_eq, ct_all = _t(sc["grf_eq"]), _t(sc["contact"])
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
    T = WL.PRIME + WL.STAND + WL.WALK
    hist = dict(state=Z(T, n, 12), R=Z(T, n, 9), foot=Z(T, n, 12), status=Z(T, n, dt=torch.int32), reach=Z(T, n, 4, dt=torch.uint8), root_pos=Z(T, n, 3), grf=Z(T, n, 12),
                contacts=Z(T, n, 4, dt=torch.uint8), mode=Z(T, n, dt=torch.uint8), sensors=Z(T, n, 38))
    stream = torch.cuda.Stream()
    wc = eng.walk_config(dt=SL.CONTROL_DT, swing_track=1.0, flat_ground=1, ground_z=0.0)
    torch.cuda.synchronize()
    for t in range(T):
        first = t <= WL.PRIME     # the priming ticks and the first closed tick read the equilibrium forces, all legs in stance
        if t in (WL.PRIME + WL.STAND, WL.PRIME + WL.STAND + 1):
            with torch.cuda.stream(stream):
                stick["mode_toggle"].copy_(one if t == WL.PRIME + WL.STAND else zero); stick["cmd"].copy_(walk_cmd)
        eng.walk_sensors_device(n, state, 12, R, foot, grf_eq if first else w["outs"]["grf"], ct_all if first else w["u8"]["contacts"], syn["quat"], syn["imu_acc_raw"],
                                syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], syn["reach"], d_foot_vel_body=fvb, stream=stream.cuda_stream)
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=stream.cuda_stream)
        if t >= WL.PRIME:
            eng.walk_step_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], front["R_z"], w["state"]["foot_pos_target_last_time"], fvb, walk=wc,
                                 stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            hist["state"][t].copy_(state); hist["R"][t].copy_(R); hist["foot"][t].copy_(foot); hist["status"][t].copy_(w["i32"]["status"]); hist["reach"][t].copy_(syn["reach"])
            hist["root_pos"][t].copy_(w["state"]["root_pos"]); hist["grf"][t].copy_(w["outs"]["grf"]); hist["contacts"][t].copy_(w["u8"]["contacts"])
            hist["mode"][t].copy_(front["movement_mode"])
            hist["sensors"][t].copy_(torch.cat([syn[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")], 1))
    torch.cuda.synchronize()
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    H = {k: v.cpu().numpy() for k, v in hist.items()}
    assert np.array_equal(H["state"][WL.PRIME - 1], sc["state"])   # (the plant was not stepped while the EKF was primed)
    w0 = WL.PRIME + WL.STAND
    assert not H["mode"][:w0].any() and (H["mode"][w0:] == 1).all()
    herr = 0.0
    for t in range(WL.PRIME, T):
        finite = np.isfinite(H["sensors"][t]).all() and np.isfinite(H["grf"][t]).all() and np.isfinite(H["state"][t]).all() and np.isfinite(H["root_pos"][t]).all()
        bad = SL.conditions_hold(H["state"][t], H["reach"][t], H["status"][t], finite)
        assert not bad, (t, bad)
        e = float(np.abs(H["root_pos"][t][:, 2] - H["state"][t][:, 5]).max())
        assert e <= WL.HEIGHT_ESTIMATE, (t, e)
        herr = max(herr, e)
    assert (H["contacts"][:w0] == 1).all()
    bad, walk = WL.walk_conditions({k: H[k][w0:] for k in ("contacts", "foot", "state", "R")}, n)
    closed = H["state"][WL.PRIME:]
    print(f"trot on the device, {WL.WALK} ticks, {n} robots: height estimate off by {herr:.1e} at most, |roll, pitch| <= {np.abs(closed[:, :, :2]).max():.3f}, height "
          f"{closed[:, :, 5].min():.3f} .. {closed[:, :, 5].max():.3f}; {walk['touchdowns']} touchdowns at z {walk['touchdown_z'][0]:.1e} .. {walk['touchdown_z'][1]:.1e}, swings "
          f"rise {walk['swing_rise']:.3f} at least, heading speed {walk['heading_speed'].min():.3f} .. {walk['heading_speed'].max():.3f}")
    assert not bad, bad
    assert walk["touchdowns"] == 12 * n and max(abs(z) for z in walk["touchdown_z"]) <= 1e-12 and walk["below_plane"] >= -1e-12
    assert walk["swing_rise"] >= WL.SWING_RISE
    assert (walk["heading_speed"] >= WL.HEADING_SPEED[0]).all() and (walk["heading_speed"] <= WL.HEADING_SPEED[1]).all()
    # the same loop on the CPU, the first 4 robots
    cpu = WL.WalkLoop(oracle, scen, sc, 4)
    for t, (stepped, cmd, toggle) in enumerate(WL.schedule(4)):
        cpu.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
        assert (cpu.status == 1).all(), t
    d = lambda a, b: float(np.abs(a - b).max())
    end, x = H["state"][-1], cpu.x
    figs = dict(pos=d(end[:4, 3:6], x[:, 3:6]), v=d(end[:4, 9:12], x[:, 9:12]), angles=d(end[:4, 0:3], x[:, 0:3]), omega=d(end[:4, 6:9], x[:, 6:9]))
    print(f"GPU loop against the CPU loop after {T - WL.PRIME} closed ticks:", ", ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert figs["pos"] <= 1e-4 and figs["v"] <= 1e-4 and figs["angles"] <= 1e-4 and figs["omega"] <= 1e-3
