"""GPU: a1mpc_sensor_synthesis_batch(_device) -- joint, IMU and pose sensors synthesised from the plant's outputs.
Yardsticks: the elementwise numpy restatement of tests/sensor_synthesis_ref.py (gyro, accelerometer, foot force, foot_pos_rel, foot_vel_rel BIT FOR BIT; the quaternion,
joint angles and joint rates within 4 E of the restatement's 80-bit evaluation, E = the float64 noise floor on the test's own inputs); the stages the synthesis inverts,
on the device (a1mpc_leg_state_batch_device gives the feet and the body's velocity back, a1mpc_sensor_frontend_batch_device the attitude and omega, one plant step the
accelerometer); and the closed loop sensors -> tick -> plant -> sensors on one stream against the same loop on the CPU (tests/sensor_loop.py).
One handle of 512 robots, gazebo parameter set, h = 10, cold solves."""
import ctypes as C

import numpy as np
import pytest

import plant_ref as PR
import sensor_loop as SL
import sensor_synthesis_ref as SR
from gpu_common import _engine, tick_buffers, tick_world

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 64, 65, 257]
NMAX = max(SIZES)
TAIL = 3
WIDTHS = dict(quat=4, imu_acc_raw=3, imu_gyro_raw=3, joint_pos=12, joint_vel=12, foot_force=4, reach=4, foot_pos_rel=12, foot_vel_rel=12)
OK, INVALID, TOO_LARGE = 0, 1, 5
_SHARED = {}


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _poisoned(rows, skip=()):
    import torch
    return {k: None if k in skip else (torch.full((rows, w), 0xFF, dtype=torch.uint8, device=_dev()) if k == "reach" else
                                       torch.full((rows, w), float("nan"), dtype=torch.float64, device=_dev())) for k, w in WIDTHS.items()}


@pytest.fixture(scope="module")
def eng(pkg, scen):
    e = _engine(pkg, scen.scenario_stand(), 512, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


def _cases(scen):
    """257 random robots as tick records (all four quaternion branches and all 16 contact patterns in every 16, rho_opt within +-0.01) and the restatement in float64 and
    in 80 bits, with and without the wrench: computed once, never changed"""
    if not _SHARED:
        rng = np.random.default_rng(6300)
        sc = SR.random_robots(scen, rng, NMAX, rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1))
        _SHARED["sc"] = sc
        for ext in (False, True):
            for dt in (np.float64, np.longdouble):
                r = SR.synthesise(sc["mass"], sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"] if ext else None, rho_opt=sc["rho_opt"], dtype=dt)
                for v in r.values():
                    v.setflags(write=False)
                _SHARED[(ext, dt)] = r
    return _SHARED["sc"], _SHARED


def _device_call(eng, sc, n, ext, stride=22, stream=None, rows=None, skip=(), sl=None):
    """the device entry on the first n robots (or the slice sl) -> numpy dict of n + TAIL rows, poisoned beforehand"""
    import torch
    sl = slice(0, n) if sl is None else sl
    ins = [_t(sc["tick"][sl, :stride]), _t(sc["R"][sl]), _t(sc["foot"][sl]), _t(sc["grf"][sl]), _t(sc["contacts"][sl])]
    ew = _t(sc["ext"][sl]) if ext else None
    out = _poisoned(n + TAIL if rows is None else rows, skip)
    torch.cuda.synchronize()
    eng.sensor_synthesis_device(n, ins[0], stride, ins[1], ins[2], ins[3], ins[4], out["quat"], out["imu_acc_raw"], out["imu_gyro_raw"], out["joint_pos"], out["joint_vel"],
                                out["foot_force"], out["reach"], out["foot_pos_rel"], out["foot_vel_rel"], d_ext_wrench=ew, rho_opt=sc["rho_opt"], stream=stream)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _tail_untouched(out, n):
    return all(v is None or ((v[n:] == 0xFF).all() if k == "reach" else np.isnan(v[n:]).all()) for k, v in out.items())


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_device_and_host_entries_equal_the_restatement(eng, scen, n, ext):
    """the first n of 257 robots: the device entry writes the restatement's bits where the arithmetic is + - * / alone, stays within 4 E of the 80-bit evaluation elsewhere,
    writes reach == 0 and nothing beyond row n; the host entry returns the device entry's bits"""
    sc, refs = _cases(scen)
    r64, r80 = refs[(ext, np.float64)], refs[(ext, np.longdouble)]
    out = _device_call(eng, sc, n, ext)
    assert _tail_untouched(out, n) and not any(np.isnan(v[:n]).any() for k, v in out.items() if k != "reach")
    figs = SR.assert_is_ref(out, r64, r80, n, (n, ext))
    h = eng.sensor_synthesis(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["ext"][:n] if ext else None, rho_opt=sc["rho_opt"])
    assert all(SR.bits_equal(h[k], out[k][:n]) for k in SR.OUTPUTS if k != "reach") and np.array_equal(h["reach"], out["reach"][:n])
    print(f"n {n} wrench {ext}: " + ", ".join(f"{k} {e:.1e} (E {E:.1e})" for k, (e, E) in figs.items()))


def test_strides_optional_outputs_streams_and_a_robot_alone(eng, scen):
    """strides 12 and 13 give the bits of 22; the optional outputs NULL change nothing else, on both entries; a side stream gives the null stream's bits; robot i alone has
    the bits of robot i of the 257"""
    import torch
    sc, refs = _cases(scen)
    r64, r80 = refs[(True, np.float64)], refs[(True, np.longdouble)]
    n = 65
    base = _device_call(eng, sc, n, True)
    same = lambda a, b, rows=slice(0, n): all(SR.bits_equal(a[k][rows], b[k][rows]) for k in SR.OUTPUTS if k != "reach" and a[k] is not None and b[k] is not None) and \
        np.array_equal(a["reach"][rows], b["reach"][rows])
    for stride in (12, 13):
        o = _device_call(eng, sc, n, True, stride=stride)
        assert same(o, base) and _tail_untouched(o, n)
    lean = _device_call(eng, sc, n, True, skip=("foot_pos_rel", "foot_vel_rel"))
    assert lean["foot_pos_rel"] is None and same(lean, base) and _tail_untouched(lean, n)
    SR.assert_is_ref(lean, r64, r80, n)
    hl = eng.sensor_synthesis(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["ext"][:n], rho_opt=sc["rho_opt"], want_foot_rel=False)
    assert hl["foot_pos_rel"] is None and hl["foot_vel_rel"] is None and same(hl, base)
    stream = torch.cuda.Stream()
    assert same(_device_call(eng, sc, n, True, stream=stream.cuda_stream), base)
    full = _device_call(eng, sc, NMAX, True)
    for i in (0, 63, 64, 200, 256):
        one = _device_call(eng, sc, 1, True, sl=slice(i, i + 1))
        assert all(SR.bits_equal(one[k][:1], full[k][i:i + 1]) for k in SR.OUTPUTS if k != "reach") and _tail_untouched(one, 1), i


def test_non_finite_inputs_stay_with_their_robot(eng, scen):
    """a NaN force on every swing leg changes no bit; a NaN omega poisons the gyro, the foot velocities and the joint rates of that robot and nothing else; an infinite foot
    raises that robot's own outputs alone"""
    sc, refs = _cases(scen)
    n = 65
    base = _device_call(eng, sc, n, True)
    keys = [k for k in SR.OUTPUTS if k != "reach"]
    swing = np.argwhere(sc["contacts"][:n] == 0)
    grf = sc["grf"].copy()
    for i, l in swing:
        grf[i, 3 * l + (i + l) % 3] = np.nan
    assert len(swing) > n
    out = _device_call(eng, dict(sc, grf=grf), n, True)
    assert all(SR.bits_equal(out[k], base[k]) for k in keys) and np.array_equal(out["reach"], base["reach"])
    tick = sc["tick"].copy(); tick[37, 7] = np.nan
    out = _device_call(eng, dict(sc, tick=tick), n, True)
    keep = np.arange(n) != 37
    assert all(SR.bits_equal(out[k][:n][keep], base[k][:n][keep]) for k in keys) and np.array_equal(out["reach"], base["reach"])
    assert np.isnan(out["imu_gyro_raw"][37]).all() and all(SR.bits_equal(out[k][37], base[k][37]) for k in ("quat", "joint_pos", "imu_acc_raw", "foot_force", "foot_pos_rel"))
    foot = sc["foot"].copy(); foot[21, 4] = np.inf
    out = _device_call(eng, dict(sc, foot=foot), n, True)
    keep = np.arange(n) != 21
    assert all(SR.bits_equal(out[k][:n][keep], base[k][:n][keep]) for k in keys) and np.array_equal(out["reach"][:n][keep], base["reach"][:n][keep])
    assert not np.isfinite(out["foot_pos_rel"][21, 3:6]).all() and _tail_untouched(out, n)


def test_refusals_leave_the_outputs_untouched(eng, scen):
    """every refusal of the header from both entries, the argument named in a1mpc_last_error, before any launch; n == 0 is OK and writes nothing"""
    import torch
    sc, _ = _cases(scen)
    n = 16
    L = eng.lib
    in_names = ["state", "R_world", "foot_abs", "grf_body", "contacts"]
    out_names = ["quat_out", "imu_acc_raw_out", "imu_gyro_raw_out", "joint_pos_out", "joint_vel_out", "foot_force_out", "reach_out"]
    ins = [_t(sc["tick"][:n]), _t(sc["R"][:n]), _t(sc["foot"][:n]), _t(sc["grf"][:n]), _t(sc["contacts"][:n])]
    outs = list(_poisoned(n).values())
    hins = [np.ascontiguousarray(sc[k][:n]) for k in ("tick", "R", "foot", "grf", "contacts")]
    houts = [np.full((n, w), 0xFF, np.uint8) if k == "reach" else np.full((n, w), np.nan) for k, w in WIDTHS.items()]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))
    fix0, opt0 = np.ascontiguousarray(SR.A1_RHO_FIX).reshape(20), np.ascontiguousarray(sc["rho_opt"]).reshape(12)

    def call(n_, stride, ins_=ins, outs_=outs, hins_=hins, houts_=houts, fix=fix0, opt=opt0, h=eng._h):
        fp, op = (None if fix is None else hp(np.ascontiguousarray(fix, dtype=np.float64))), (None if opt is None else hp(np.ascontiguousarray(opt, dtype=np.float64)))
        rd = L.a1mpc_sensor_synthesis_batch_device(h, n_, ptr(ins_[0]), stride, *[ptr(t) for t in ins_[1:]], None, fp, op, *[ptr(t) for t in outs_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_sensor_synthesis_batch(h, n_, hp(hins_[0]), stride, *[hp(a) for a in hins_[1:]], None, fp, op, *[hp(a) for a in houts_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    def geometry(changes=()):
        f, o = fix0.copy().reshape(4, 5), opt0.copy().reshape(4, 3)
        for arr, l, k, v in changes:
            (f if arr == "fix" else o)[l, k] = v
        return dict(fix=f.reshape(20), opt=o.reshape(12))

    g = lambda arr, l, k, v: geometry([(arr, l, k, v)])
    bad = [(dict(stride=14), "state_stride"), (dict(stride=0), "state_stride"), (dict(n_=-1), "negative n"), (dict(fix=None), "null rho_fix"), (dict(opt=None), "null rho_opt"),
           (g("fix", 2, 1, np.nan), "rho_fix"), (g("fix", 0, 4, np.inf), "rho_fix"), (g("opt", 3, 0, np.nan), "rho_opt"), (g("fix", 1, 3, 0.0), "upper leg"),
           (g("fix", 1, 3, -0.21), "upper leg")]
    zero_len = geometry(); zero_len["fix"][5 * 2 + 4] = 0.05; zero_len["opt"][3 * 2 + 2] = 0.05; zero_len["opt"][3 * 2] = 0.0
    bad.append((zero_len, "lower leg"))
    for kw, word in bad:
        kw = dict(kw); n_ = kw.pop("n_", n); stride = kw.pop("stride", 22)
        rd, md, rh, mh = call(n_, stride, **kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    rd, md, rh, mh = call(513, 22)
    assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    rd, md, rh, mh = call(n, 22, h=None)
    assert rd == INVALID and rh == INVALID and "null handle" in md and "null handle" in mh
    for k, name in enumerate(in_names):
        rd, md, rh, mh = call(n, 22, ins_=[None if j == k else t for j, t in enumerate(ins)], hins_=[None if j == k else t for j, t in enumerate(hins)])
        assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for k, name in enumerate(out_names):
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


# ---- independent of the restatement: the stages the synthesis inverts, on the device
def _within(got, r64, r80, label):
    """the tolerance rule on a round trip: |device - 80-bit| <= 4 E, E = |float64 - 80-bit| of the restated round trip on these inputs"""
    E = float(np.abs(r64.astype(np.longdouble) - r80).max())
    err = float(np.abs(got.astype(np.longdouble) - r80).max())
    assert err <= SR.FACTOR * E, (label, err, E)
    return err, E


def test_leg_stage_and_sensor_stage_give_the_plant_back(eng, scen):
    """the synthesised joint_pos, joint_vel and R through a1mpc_leg_state_batch_device reproduce foot_abs, and -R (foot_vel_rel + gyro x foot_pos_rel) is v on the stance
    legs; the synthesised quaternion and gyro through a1mpc_sensor_frontend_batch_device (imu_window = 1, fresh filters) reproduce R_world and omega.  Each within 4 E of
    the restated round trip's 80-bit evaluation -- which itself is the plant's value to 1e-14 (R is orthogonal to 2e-16)"""
    import torch
    sc, refs = _cases(scen)
    n = NMAX
    s64, s80 = refs[(False, np.float64)], refs[(False, np.longdouble)]
    t64, t80 = SR.round_trips(s64, sc["R"], rho_opt=sc["rho_opt"]), SR.round_trips(s80, sc["R"], rho_opt=sc["rho_opt"], dtype=np.longdouble)
    stance = np.repeat(sc["contacts"] != 0, 3, axis=1)
    truth = dict(foot_abs=sc["foot"], v_stance=np.tile(sc["tick"][:, 9:12], (1, 4)), R_world=sc["R"], omega=sc["tick"][:, 6:9])
    for k in SR.ROUND_TRIPS:
        m = stance if k == "v_stance" else np.ones_like(truth[k], bool)
        assert np.abs(t80[k] - truth[k])[m].max() <= 1e-14, k   # the restated round trip closes (R R' - I is 2e-16: R is a float64 matrix)
    ins = [_t(sc["tick"]), _t(sc["R"]), _t(sc["foot"]), _t(sc["grf"]), _t(sc["contacts"])]
    syn = _poisoned(n)
    z3 = torch.zeros((n, 3), dtype=torch.float64, device=_dev())
    leg = {k: torch.full((n, w), float("nan"), dtype=torch.float64, device=_dev()) for k, w in (("rel", 12), ("Jb", 36), ("vrel", 12), ("abs", 12))}
    front = {k: torch.full((n, w), float("nan"), dtype=torch.float64, device=_dev()) for k, w in (("R_world", 9), ("R_z", 9), ("root_euler", 3), ("imu_acc", 3), ("imu_ang_vel", 3),
                                                                                                  ("root_ang_vel", 3))}
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dp_ = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    eng.reset_sensor_state()
    torch.cuda.synchronize()
    eng.sensor_synthesis_device(n, ins[0], 22, ins[1], ins[2], ins[3], ins[4], syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"],
                                syn["foot_force"], syn["reach"], syn["foot_pos_rel"], syn["foot_vel_rel"], rho_opt=sc["rho_opt"], stream=stream.cuda_stream)
    fix, opt = np.ascontiguousarray(SR.A1_RHO_FIX), np.ascontiguousarray(sc["rho_opt"])
    rc = eng.lib.a1mpc_leg_state_batch_device(eng._h, n, ptr(syn["joint_pos"]), ptr(syn["joint_vel"]), ptr(ins[1]), ptr(z3), ptr(z3), dp_(fix), dp_(opt), ptr(leg["rel"]),
                                              ptr(leg["Jb"]), ptr(leg["vrel"]), ptr(leg["abs"]), None, None, None, sp)
    assert rc == 0, eng.lib.a1mpc_last_error()
    eng.sensor_frontend_device(n, syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], *front.values(), cfg=eng.sensor_config(imu_window=1), stream=stream.cuda_stream)
    torch.cuda.synchronize()
    eng.reset_sensor_state()
    N = lambda t: t.cpu().numpy()
    got = dict(foot_abs=N(leg["abs"]), v_stance=SR.stance_velocity(sc["R"], N(leg["vrel"]), N(syn["imu_gyro_raw"]), N(leg["rel"])), R_world=N(front["R_world"]),
               omega=N(front["root_ang_vel"]))
    figs = {}
    for k in SR.ROUND_TRIPS:
        m = stance if k == "v_stance" else np.ones_like(truth[k], bool)
        figs[k] = _within(np.where(m, got[k], 0.0), np.where(m, t64[k], 0.0), np.where(m, t80[k], 0.0), k)
    print("round trips through the leg stage and the sensor stage: " + ", ".join(f"{k} {e:.1e} (E {E:.1e})" for k, (e, E) in figs.items()))
    assert np.array_equal(N(front["imu_ang_vel"]), N(syn["imu_gyro_raw"]))   # a window of one sample is the sample


def test_accelerometer_is_the_specific_force_of_the_plant_step(eng, scen):
    """one a1mpc_plant_step_batch with substeps = 1: R_pre imu_acc_raw = (v' - v) / dt - g e_z within 1e-12 max(1, |a|), the rounding of v divided by dt (about 4e-14
    for |v| <= 1), with and without the wrench"""
    sc, refs = _cases(scen)
    n, dt = NMAX, 0.0025
    for ext in (False, True):
        ew = sc["ext"] if ext else None
        syn = eng.sensor_synthesis(sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], ew, rho_opt=sc["rho_opt"])
        st = eng.plant_step(sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], ew, plant=eng.plant_config(dt=dt, substeps=1))["state"]
        a = (st[:, 9:12] - sc["tick"][:, 9:12]) / dt - np.array([0.0, 0.0, PR.GRAVITY])
        got = np.einsum("bij,bj->bi", sc["R"].reshape(n, 3, 3), syn["imu_acc_raw"])
        err = np.abs(got - a).max(axis=1) / np.maximum(1.0, np.abs(a).max(axis=1))
        print(f"wrench {ext}: R imu_acc_raw against (v' - v) / dt - g e_z: {err.max():.1e} relative to max(1, |a|)")
        assert err.max() <= 1e-12 and np.abs(a).max() > 5.0


# ---- the closed loop on the device
def test_closed_loop_sensors_tick_plant_on_the_device(eng, pkg, oracle, scen):
    """17 perturbed standing robots (sensor_loop.perturbed_standing_robots), h = 10, cold solves.  PRIME ticks of a1mpc_sensor_synthesis_batch_device ->
    a1mpc_control_tick_sensors_device on the unstepped plant under the equilibrium forces prime the EKF; then 100 x (synthesis -> tick -> a1mpc_plant_step_batch_device with
    the tick's grf and contacts, in place), all on one stream, enqueued without a host synchronisation; each tick's plant state, sensors and status are copied into a
    history on the same stream and looked at afterwards.  On every tick: return codes 0, every output finite, status 1, reach == 0, |roll|, |pitch| <= 0.2, the height
    within 0.3 +- 0.05.  The end state of the first 4 robots is that of the same loop on the CPU (sensor_loop.OracleLoop): pos, v, angles within 1e-4, omega within 1e-3
    (the bounds of tests/test_gpu_plant.py's closed loop: a 1e-5 N force parity accumulating, over a quarter of its ticks)."""
    import torch
    E = pkg.engine
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
    assert eng.horizon == SL.H and eng.cfg.warm_start == 0 and eng.cfg.mass == sc["params"]["mass"]
    L = eng.lib
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm))
    assert prm.control_dt == SL.CONTROL_DT and np.array_equal(np.array(prm.rho_fix).reshape(4, 5), SR.A1_RHO_FIX) and not np.array(prm.rho_opt).any()
    assert np.array_equal(np.array(prm.gait.default_foot_pos), SL.DEFAULT_FOOT_POS)
    state, R, foot = _t(sc["state"]), _t(sc["R"]), _t(sc["foot"])
    grf_eq, ct_all = _t(sc["grf_eq"]), _t(sc["contact"])
    w = tick_world(n, dev, [0.0, 120.0, 120.0, 0.0])
    Z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    syn = dict(quat=Z(n, 4), imu_acc_raw=Z(n, 3), imu_gyro_raw=Z(n, 3), joint_pos=Z(n, 12), joint_vel=Z(n, 12), foot_force=Z(n, 4), reach=Z(n, 4, dt=torch.uint8))
    front = dict(R_world=Z(n, 9), R_z=Z(n, 9), root_euler=Z(n, 3), root_ang_vel=Z(n, 3), imu_acc=Z(n, 3), imu_ang_vel=Z(n, 3), root_lin_vel_d=Z(n, 3), root_ang_vel_d=Z(n, 3),
                 root_pos_d_z=Z(n), movement_mode=Z(n, dt=torch.uint8), mpc_active=Z(n, dt=torch.uint8))
    cs = {k: _t(v) for k, v in E.Engine.command_state(n).items() if k != "root_euler_d"}   # (root_euler_d is the tick world's)
    inp = dict(joint_pos=syn["joint_pos"], joint_vel=syn["joint_vel"], foot_force=syn["foot_force"], gait_counter_speed=_t(np.full((n, 4), 2.0)), torques_gravity=Z(n, 12), **front)
    stick = dict(cmd=Z(n, 6), mode_toggle=Z(n, dt=torch.uint8))   # no command, no toggle: the robots stand.  (Held here: a TickSensors keeps addresses, not tensors)
    ts = eng.tick_sensors(sensor=eng.sensor_config(imu_window=SL.IMU_WINDOW), quat=syn["quat"], imu_acc_raw=syn["imu_acc_raw"], imu_gyro_raw=syn["imu_gyro_raw"], **stick, **cs)
    bf = tick_buffers(E, inp, w)
    T = SL.PRIME + SL.TICKS
    hist = dict(state=Z(T, n, 12), status=Z(T, n, dt=torch.int32), reach=Z(T, n, 4, dt=torch.uint8), root_pos=Z(T, n, 3), grf=Z(T, n, 12), contacts=Z(T, n, 4, dt=torch.uint8),
                sensors=Z(T, n, 38))
    stream = torch.cuda.Stream()
    pc = eng.plant_config(dt=SL.CONTROL_DT)
    torch.cuda.synchronize()
    for t in range(T):
        first = t <= SL.PRIME     # the priming ticks and the first closed tick read the equilibrium forces, all legs in stance
        eng.sensor_synthesis_device(n, state, 12, R, foot, grf_eq if first else w["outs"]["grf"], ct_all if first else w["u8"]["contacts"], syn["quat"], syn["imu_acc_raw"],
                                    syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], syn["reach"], stream=stream.cuda_stream)
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=stream.cuda_stream)
        if t >= SL.PRIME:
            eng.plant_step_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], plant=pc, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            hist["state"][t].copy_(state); hist["status"][t].copy_(w["i32"]["status"]); hist["reach"][t].copy_(syn["reach"]); hist["root_pos"][t].copy_(w["state"]["root_pos"])
            hist["grf"][t].copy_(w["outs"]["grf"]); hist["contacts"][t].copy_(w["u8"]["contacts"])
            hist["sensors"][t].copy_(torch.cat([syn[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")], 1))
    torch.cuda.synchronize()
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    H = {k: v.cpu().numpy() for k, v in hist.items()}
    herr = np.abs(H["root_pos"][:SL.PRIME, :, 2] - H["state"][:SL.PRIME, :, 5]).max(axis=1)
    print(f"height estimate against the plant's over the {SL.PRIME} priming ticks: " + " ".join(f"{e:.1e}" for e in herr))
    assert herr[-1] <= 1e-3
    assert np.array_equal(H["state"][SL.PRIME - 1], sc["state"])   # (the plant was not stepped while the EKF was primed)
    for t in range(T):
        finite = np.isfinite(H["sensors"][t]).all() and np.isfinite(H["grf"][t]).all() and np.isfinite(H["state"][t]).all() and np.isfinite(H["root_pos"][t]).all()
        bad = SL.conditions_hold(H["state"][t], H["reach"][t], H["status"][t], finite)
        assert not bad, (t, bad)
    assert (H["contacts"] == 1).all()
    end = H["state"][-1]
    tilt = lambda x: float(np.abs(x[:, 0:2]).max()); spin = lambda x: float(np.abs(x[:, 6:9]).max())
    print(f"closed loop, {SL.TICKS} ticks: |roll, pitch| {tilt(sc['state']):.4f} -> {tilt(end):.4f}, |omega| {spin(sc['state']):.3f} -> {spin(end):.3f}, height "
          f"{end[:, 5].min():.4f} .. {end[:, 5].max():.4f}, estimate off by {np.abs(H['root_pos'][-1][:, 2] - end[:, 5]).max():.1e}")
    assert tilt(end) < 0.5 * tilt(sc["state"])
    # the same loop on the CPU, the first 4 robots
    cpu = SL.OracleLoop(oracle, scen, sc, 4)
    for t in range(T):
        cpu.tick(step_plant=t >= SL.PRIME)
        assert (cpu.status == 1).all(), t
    d = lambda a, b: float(np.abs(a - b).max())
    x = cpu.x
    figs = dict(pos=d(end[:4, 3:6], x[:, 3:6]), v=d(end[:4, 9:12], x[:, 9:12]), angles=d(end[:4, 0:3], x[:, 0:3]), omega=d(end[:4, 6:9], x[:, 6:9]))
    print(f"GPU loop against the CPU loop after {SL.TICKS} ticks:", ", ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert figs["pos"] <= 1e-4 and figs["v"] <= 1e-4 and figs["angles"] <= 1e-4 and figs["omega"] <= 1e-3
