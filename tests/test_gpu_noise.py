"""GPU: a1mpc_sensor_noise_batch(_device) -- counter-based Gaussian noise on the synthesised sensors and a random-walk IMU bias, in place.  Yardsticks: the numpy
restatement of tests/noise_ref.py (z within the device bar, every array within sigma times it plus one ulp); what must hold bit for bit on the device itself (a repeated
call, a robot alone, a split batch, the reductions, a side stream, a NaN row, the host entry against the device entry); every refusal of the header with poisoned arrays;
and the noisy trot  walk sensors -> sensor noise -> tick -> walk step  on one stream against the same loop on the CPU (tests/noise_loop.py).  One handle of 512 robots,
gazebo parameter set, h = 10, cold solves."""
import ctypes as C

import numpy as np
import pytest

import noise_loop as NL
import noise_ref as NR
import sensor_loop as SL
import walk_loop as WL
from gpu_common import _engine, tick_buffers, tick_world

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 65, 257]
NMAX = max(SIZES)
TAIL = 3
CASES = [(0, 7, 2026), (2 ** 32 - NMAX, 2 ** 33, 0x9E3779B97F4A7C15), (1000, 0, 2026)]   # robot0, tick, seed
KEYS = NR.SENSORS + ("imu_bias",)
OK, INVALID, TOO_LARGE = 0, 1, 5
_SHARED = {}


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(_dev())   # (a copy: the shared inputs are read-only)


@pytest.fixture(scope="module")
def eng(pkg, scen):
    e = _engine(pkg, scen.scenario_stand(), 512, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


def _sensors():
    """260 rows of sensor values and a bias: computed once, never changed"""
    if "s" not in _SHARED:
        _SHARED["s"] = NR.random_sensors(NMAX + TAIL, seed=8300)
    return _SHARED["s"]


def _config(eng, cfg):
    return eng.noise_config(**cfg)


def _device(eng, cfg, robot0, tick, n, src=None, skip=(), sl=None, stream=None, want_z=True):
    """the device entry on copies of rows sl (default: all 260, the first n worked on) -> (dict of the arrays of KEYS not skipped, z (n + TAIL, 44) NaN-poisoned or None)"""
    import torch
    src = _sensors() if src is None else src
    sl = slice(None) if sl is None else sl
    d = {k: (None if k in skip else _t(src[k][sl])) for k in KEYS}
    z = torch.full((n + TAIL, 44), float("nan"), dtype=torch.float64, device=_dev()) if want_z else None
    torch.cuda.synchronize()
    eng.sensor_noise_device(_config(eng, cfg), n, tick, *[d[k] for k in KEYS], d_z=z, robot0=robot0, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items() if v is not None}, None if z is None else z.cpu().numpy()


def _host(eng, cfg, robot0, tick, n, src=None):
    src = _sensors() if src is None else src
    a = {k: np.array(src[k][:n]) for k in KEYS}
    z = eng.sensor_noise(_config(eng, cfg), tick, **a, robot0=robot0, want_z=True)
    return a, z


def _same(a, b, rows=slice(None), rows_b=None):
    rows_b = rows if rows_b is None else rows_b
    return all(NR.bits_equal(a[k][rows], b[k][rows_b]) for k in a)


@pytest.mark.parametrize("n", SIZES)
def test_device_and_host_entries_equal_the_restatement(eng, n):
    """the first n of 260 rows, every channel on at levels of order one; robot0 0, 1000 and 2^32 - 257, ticks 0, 7 and 2^33, both seeds: z within the device bar, every
    array within sigma times the bar plus one ulp, nothing beyond row n; the host entry returns the device entry's bits"""
    src = _sensors()
    worst = 0.0
    for robot0, tick, seed in CASES:
        cfg = dict(NR.LOUD, seed=seed)
        ref, rbias, rz = NR.apply(cfg, robot0, tick, {k: src[k][:n] for k in NR.SENSORS}, src["imu_bias"][:n])
        out, z = _device(eng, cfg, robot0, tick, n)
        e = float(np.abs(z[:n] - rz).max())
        print(f"n {n} robot0 {robot0} tick {tick} seed {seed:#x}: worst |z - z_ref| {e:.3e}")
        worst = max(worst, e)
        assert e <= NR.CEILING, e
        assert e <= NR.DEVICE_BAR, (e, NR.DEVICE_BAR)
        excess, figs = NR.worst_excess(out, dict(ref, imu_bias=rbias), cfg, NR.DEVICE_BAR, True, n)
        assert excess <= 0.0, (excess, figs)
        assert np.isnan(z[n:]).all() and all(NR.bits_equal(out[k][n:], src[k][n:]) for k in KEYS) and not any(NR.bits_equal(out[k][:n], src[k][:n]) for k in KEYS)
        h, hz = _host(eng, cfg, robot0, tick, n)
        assert _same(h, out, slice(0, n)) and NR.bits_equal(hz, z[:n])
    print(f"n {n}: worst |z - z_ref| {worst:.3e} (device bar {NR.DEVICE_BAR})")


def test_determinism_split_and_a_side_stream(eng):
    """a repeated call; a side stream; robot g alone (robot0 = g, n = 1) against its row of the 257; the 257 split at 100 with robot0 offset against the whole; another
    tick, robot or seed gives other normals, and a robot's normals do not depend on its row"""
    import torch
    cfg, robot0, tick, n = NR.LOUD, 1000, 7, NMAX
    src = _sensors()
    whole, z = _device(eng, cfg, robot0, tick, n)
    again, z2 = _device(eng, cfg, robot0, tick, n)
    assert _same(again, whole) and NR.bits_equal(z2, z)
    side, z3 = _device(eng, cfg, robot0, tick, n, stream=torch.cuda.Stream().cuda_stream)
    assert _same(side, whole) and NR.bits_equal(z3, z)
    for i in (0, 63, 64, 200, 256):
        one, z1 = _device(eng, cfg, robot0 + i, tick, 1, sl=slice(i, i + 1 + TAIL))
        assert _same(one, whole, slice(0, 1), slice(i, i + 1)) and NR.bits_equal(z1[:1], z[i:i + 1]), i
    lo, zlo = _device(eng, cfg, robot0, tick, 100, sl=slice(0, 100))
    hi, zhi = _device(eng, cfg, robot0 + 100, tick, n - 100, sl=slice(100, n))
    assert _same(lo, whole, slice(0, 100)) and _same(hi, whole, slice(0, n - 100), slice(100, n)) and NR.bits_equal(zlo[:100], z[:100]) and NR.bits_equal(zhi[:n - 100], z[100:n])
    assert not NR.bits_equal(_device(eng, cfg, robot0, tick + 1, n)[1], z) and not NR.bits_equal(_device(eng, dict(cfg, seed=2027), robot0, tick, n)[1], z)
    assert NR.bits_equal(_device(eng, cfg, robot0 + 1, tick, n)[1][:n - 1], z[1:n])


def test_reductions_and_a_nan_row(eng):
    """all sigmas 0 with the bias NULL leaves every array unchanged, -0 and NaN rows included; with the bias given and both walks 0 the bias keeps its bits and is still
    applied; one sigma on changes only its array, with and without z_out; z_out is the same whatever the sigmas; a NULL array is left alone and changes nothing else; a NaN
    row stays with its robot"""
    src = {k: np.array(v) for k, v in _sensors().items()}
    for k in NR.SENSORS:
        src[k][3] = -0.0; src[k][20] = np.nan
        src[k][21].view(np.uint64)[:] = 0x7FF8DEADBEEF0001
    n = 65
    off = NR.config(seed=2026)
    loud, lz = _device(eng, NR.LOUD, 0, 7, n, src)
    out, z = _device(eng, off, 0, 7, n, src, skip=("imu_bias",))
    assert all(NR.bits_equal(out[k], src[k]) for k in NR.SENSORS) and NR.bits_equal(z, lz)
    out, z = _device(eng, off, 0, 7, n, src)
    ref, _, _ = NR.apply(off, 0, 7, {k: src[k] for k in NR.SENSORS}, src["imu_bias"])
    assert NR.bits_equal(out["imu_bias"], src["imu_bias"]) and NR.bits_equal(z, lz) and all(NR.bits_equal(out[k][:n], ref[k][:n]) for k in NR.SENSORS)
    assert not NR.bits_equal(out["imu_gyro_raw"], src["imu_gyro_raw"])
    owner = dict(gyro_sigma="imu_gyro_raw", acc_sigma="imu_acc_raw", att_sigma="quat", joint_pos_sigma="joint_pos", joint_vel_sigma="joint_vel", foot_force_sigma="foot_force")
    quiet = dict(NR.LOUD, gyro_bias_walk=0.0, acc_bias_walk=0.0)
    full, _ = _device(eng, quiet, 0, 7, n, src, skip=("imu_bias",))
    for level, key in owner.items():
        for want_z in (True, False):
            out, z = _device(eng, NR.config(seed=2026, **{level: NR.LOUD[level]}), 0, 7, n, src, skip=("imu_bias",), want_z=want_z)
            assert [k for k in NR.SENSORS if not NR.bits_equal(out[k], src[k])] == [key], (level, want_z)
            assert NR.bits_equal(out[key], full[key]) and (z is None or NR.bits_equal(z, lz)), (level, want_z)
    for key in NR.SENSORS:
        out, z = _device(eng, NR.LOUD, 0, 7, n, src, skip=(key,))
        assert key not in out and _same(out, loud) and NR.bits_equal(z, lz)
    bad = 37
    s2 = {k: np.array(v) for k, v in _sensors().items()}
    base, bz = _device(eng, NR.LOUD, 0, 7, n, s2)
    for v in s2.values():
        v[bad] = np.nan
    out, z = _device(eng, NR.LOUD, 0, 7, n, s2)
    keep = np.arange(NMAX + TAIL) != bad
    assert all(NR.bits_equal(out[k][keep], base[k][keep]) and np.isnan(out[k][bad]).all() for k in KEYS) and NR.bits_equal(z, bz)


def test_refusals_leave_the_arrays_untouched(eng):
    """every refusal of the header: A1MPC_ERR_INVALID_ARGUMENT (1) from both entries, the field named in a1mpc_last_error, before any launch; n > max_batch is
    A1MPC_ERR_BATCH_TOO_LARGE; n == 0 is OK and writes nothing; the same arguments, accepted, do write"""
    import torch
    n = 16
    L = eng.lib
    names = list(KEYS) + ["z_out"]
    widths = [NR.WIDTHS[k] for k in KEYS] + [44]
    dev = [torch.full((n, w), float("nan"), dtype=torch.float64, device=_dev()) for w in widths]
    hst = [np.full((n, w), np.nan) for w in widths]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(cfg, n_=n, robot0=0, dev_=dev, hst_=hst, h=eng._h):
        nc = None if cfg is None else C.byref(_config(eng, cfg))
        rd = L.a1mpc_sensor_noise_batch_device(h, nc, n_, robot0, 7, *[ptr(t) for t in dev_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_sensor_noise_batch(h, nc, n_, robot0, 7, *[hp(a) for a in hst_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    nan, inf = float("nan"), float("inf")
    bad = [(dict(h=None), "null handle"), (dict(cfg=None), "a1mpc_noise_config"), (dict(n_=-1), "negative n"), (dict(robot0=2 ** 32 - n + 1), "2^32"),
           (dict(robot0=2 ** 64 - 1), "2^32")]
    for level in NR.LEVELS:
        bad += [(dict(cfg=dict(NR.LOUD, **{level: v})), level) for v in (-1e-9, nan, inf, -inf)]
    swap = lambda lst, i, v: [v if j == i else x for j, x in enumerate(lst)]
    bad += [(dict(cfg=dict(NR.OFF, gyro_bias_walk=1e-5), dev_=swap(dev, 6, None), hst_=swap(hst, 6, None)), "imu_bias"),
            (dict(cfg=dict(NR.OFF, acc_bias_walk=1e-4), dev_=swap(dev, 6, None), hst_=swap(hst, 6, None)), "imu_bias"),
            (dict(dev_=swap(dev, 4, dev[3]), hst_=swap(hst, 4, hst[3])), "overlap"), (dict(dev_=swap(dev, 7, dev[0]), hst_=swap(hst, 7, hst[0])), "overlap"),
            (dict(dev_=swap(dev, 2, dev[1][1:]), hst_=swap(hst, 2, hst[1][1:])), "overlap")]
    for kw, word in bad:
        kw = dict(kw); cfg = kw.pop("cfg", NR.LOUD)
        rd, md, rh, mh = call(cfg, **kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    big_dev = [torch.full((513, w), float("nan"), dtype=torch.float64, device=_dev()) for w in widths]   # (513 rows each: 513 rows of the small ones would overlap)
    big_hst = [np.full((513, w), np.nan) for w in widths]
    rd, md, rh, mh = call(NR.LOUD, n_=513, dev_=big_dev, hst_=big_hst)
    assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all().item() for t in big_dev) and all(np.isnan(a).all() for a in big_hst)
    rd, _, rh, _ = call(NR.LOUD, n_=0)
    assert rd == OK and rh == OK
    rd, md, rh, mh = call(NR.LOUD, n_=0, robot0=2 ** 32)   # (the last index is 2^32 - 1: an empty batch may start behind it)
    assert rd == OK and rh == OK, (md, mh)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all().item() for t in dev) and all(np.isnan(a).all() for a in hst), names
    for t, a in zip(dev[:7], hst[:7]):
        t.zero_(); a[:] = 0.0
    rd, md, rh, mh = call(dict(NR.LOUD, gyro_sigma=-0.0), robot0=2 ** 32 - n)   # (the same arrays, accepted, are written; -0 is 0: off)
    torch.cuda.synchronize()
    assert rd == OK and rh == OK, (md, mh)
    assert not torch.isnan(dev[7]).any().item() and not np.isnan(hst[7]).any() and all(bool((t != 0).any().item()) for t in dev[3:7]) and all((a != 0).any() for a in hst[3:7])
    assert all(NR.bits_equal(t.cpu().numpy(), a) for t, a in zip(dev, hst))


# ---- the noisy trot on the device
def test_noisy_trot_on_the_device(eng, pkg, oracle, scen):
    """the trot of tests/test_gpu_walk.py with a1mpc_sensor_noise_batch_device between the walk sensors and the tick: 17 perturbed standing robots, NOMINAL levels, seed
    2026, robot0 0, the noise's tick = the loop's tick, the bias carried on the device from zero.  All on one stream, enqueued without a host synchronisation between the
    first launch and the last.  Every per-tick and whole-walk condition of the CPU trot on all 17 robots, and the end state against the CPU NoisyWalkLoop of 17 within
    the end-state bars of tests/test_gpu_walk.py: pos, v, angles within 1e-4, omega within 1e-3"""
    import torch
    E = pkg.engine
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
    assert eng.horizon == SL.H and eng.cfg.warm_start == 0 and eng.cfg.mass == sc["params"]["mass"]
    L = eng.lib
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm))
    state, R, foot = _t(sc["state"]), _t(sc["R"]), _t(sc["foot"])
    grf_eq, ct_all = _t(sc["grf_eq"]), _t(sc["contact"])
    w = tick_world(n, dev, WL.COUNTERS)
    Z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    syn = dict(quat=Z(n, 4), imu_acc_raw=Z(n, 3), imu_gyro_raw=Z(n, 3), joint_pos=Z(n, 12), joint_vel=Z(n, 12), foot_force=Z(n, 4), reach=Z(n, 4, dt=torch.uint8))
    front = dict(R_world=Z(n, 9), R_z=Z(n, 9), root_euler=Z(n, 3), root_ang_vel=Z(n, 3), imu_acc=Z(n, 3), imu_ang_vel=Z(n, 3), root_lin_vel_d=Z(n, 3), root_ang_vel_d=Z(n, 3),
                 root_pos_d_z=Z(n), movement_mode=Z(n, dt=torch.uint8), mpc_active=Z(n, dt=torch.uint8))
    cs = {k: _t(v) for k, v in E.Engine.command_state(n).items() if k != "root_euler_d"}
    inp = dict(joint_pos=syn["joint_pos"], joint_vel=syn["joint_vel"], foot_force=syn["foot_force"], gait_counter_speed=_t(np.full((n, 4), WL.COUNTER_SPEED)),
               torques_gravity=Z(n, 12), **front)
    stick = dict(cmd=Z(n, 6), mode_toggle=Z(n, dt=torch.uint8))
    walk_cmd = Z(n, 6); walk_cmd[:, 0] = WL.SPEED
    one, zero = torch.ones(n, dtype=torch.uint8, device=dev), Z(n, dt=torch.uint8)
    ts = eng.tick_sensors(sensor=eng.sensor_config(imu_window=SL.IMU_WINDOW), quat=syn["quat"], imu_acc_raw=syn["imu_acc_raw"], imu_gyro_raw=syn["imu_gyro_raw"], **stick, **cs)
    bf = tick_buffers(E, inp, w)
    fvb, bias = Z(n, 12), Z(n, 6)
    nc = eng.noise_config(**NR.NOMINAL)
    T = WL.PRIME + WL.STAND + WL.WALK
    hist = dict(state=Z(T, n, 12), R=Z(T, n, 9), foot=Z(T, n, 12), status=Z(T, n, dt=torch.int32), reach=Z(T, n, 4, dt=torch.uint8), root_pos=Z(T, n, 3), grf=Z(T, n, 12),
                contacts=Z(T, n, 4, dt=torch.uint8), sensors=Z(T, n, 38), root_vel=Z(T, n, 3))
    stream = torch.cuda.Stream()
    wc = eng.walk_config(dt=SL.CONTROL_DT, swing_track=1.0, flat_ground=1, ground_z=0.0)
    torch.cuda.synchronize()
    for t in range(T):
        first = t <= WL.PRIME
        if t in (WL.PRIME + WL.STAND, WL.PRIME + WL.STAND + 1):
            with torch.cuda.stream(stream):
                stick["mode_toggle"].copy_(one if t == WL.PRIME + WL.STAND else zero); stick["cmd"].copy_(walk_cmd)
        eng.walk_sensors_device(n, state, 12, R, foot, grf_eq if first else w["outs"]["grf"], ct_all if first else w["u8"]["contacts"], syn["quat"], syn["imu_acc_raw"],
                                syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], syn["reach"], d_foot_vel_body=fvb, stream=stream.cuda_stream)
        eng.sensor_noise_device(nc, n, t, syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], bias,
                                stream=stream.cuda_stream)
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=stream.cuda_stream)
        if t >= WL.PRIME:
            eng.walk_step_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], front["R_z"], w["state"]["foot_pos_target_last_time"], fvb, walk=wc,
                                 stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            hist["state"][t].copy_(state); hist["R"][t].copy_(R); hist["foot"][t].copy_(foot); hist["status"][t].copy_(w["i32"]["status"]); hist["reach"][t].copy_(syn["reach"])
            hist["root_pos"][t].copy_(w["state"]["root_pos"]); hist["grf"][t].copy_(w["outs"]["grf"]); hist["contacts"][t].copy_(w["u8"]["contacts"])
            hist["root_vel"][t].copy_(w["state"]["root_lin_vel"])
            hist["sensors"][t].copy_(torch.cat([syn[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")], 1))
    torch.cuda.synchronize()
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    H = {k: v.cpu().numpy() for k, v in hist.items()}
    assert np.array_equal(H["state"][WL.PRIME - 1], sc["state"])
    w0 = WL.PRIME + WL.STAND
    herr = 0.0
    for t in range(WL.PRIME, T):
        finite = np.isfinite(H["sensors"][t]).all() and np.isfinite(H["grf"][t]).all() and np.isfinite(H["state"][t]).all() and np.isfinite(H["root_pos"][t]).all()
        bad = SL.conditions_hold(H["state"][t], H["reach"][t], H["status"][t], finite)
        assert not bad, (t, bad)
        e = float(np.abs(H["root_pos"][t][:, 2] - H["state"][t][:, 5]).max())
        assert e <= WL.HEIGHT_ESTIMATE, (t, e)
        herr = max(herr, e)
    bad, walk = WL.walk_conditions({k: H[k][w0:] for k in ("contacts", "foot", "state", "R")}, n)
    closed = H["state"][WL.PRIME:]
    verr = float(np.abs(H["root_vel"][WL.PRIME:] - closed[:, :, 9:12]).max())
    print(f"noisy trot on the device, {WL.WALK} ticks, {n} robots: height estimate off by {herr:.2e} at most, |roll, pitch| <= {np.abs(closed[:, :, :2]).max():.3f}, swings "
          f"rise {walk['swing_rise']:.3f} at least, heading speed {walk['heading_speed'].min():.3f} .. {walk['heading_speed'].max():.3f}, the EKF's velocity off by {verr:.3f} "
          f"m/s at most, bias up to {float(bias.abs().max()):.1e}")
    assert not bad, bad
    assert walk["swing_rise"] >= WL.SWING_RISE
    assert (walk["heading_speed"] >= WL.HEADING_SPEED[0]).all() and (walk["heading_speed"] <= WL.HEADING_SPEED[1]).all()
    # the same loop on the CPU, all 17 robots
    cpu = NL.NoisyWalkLoop(oracle, scen, sc, n, noise=NR.NOMINAL)
    for t, (stepped, cmd, toggle) in enumerate(WL.schedule(n)):
        cpu.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
        assert (cpu.status == 1).all(), t
    d = lambda a, b: float(np.abs(a - b).max())
    end, x = H["state"][-1], cpu.x
    figs = dict(pos=d(end[:, 3:6], x[:, 3:6]), v=d(end[:, 9:12], x[:, 9:12]), angles=d(end[:, 0:3], x[:, 0:3]), omega=d(end[:, 6:9], x[:, 6:9]),
                bias=d(bias.cpu().numpy(), cpu.bias))
    print(f"GPU loop against the CPU loop after {T - WL.PRIME} closed ticks:", ", ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert figs["pos"] <= 1e-4 and figs["v"] <= 1e-4 and figs["angles"] <= 1e-4 and figs["omega"] <= 1e-3
    # the bias is a sum of T terms walk z: each may be off by walk times the z bar, and each sum may round the other way
    assert figs["bias"] <= T * (max(NR.NOMINAL["gyro_bias_walk"], NR.NOMINAL["acc_bias_walk"]) * NR.DEVICE_BAR + np.spacing(np.abs(cpu.bias).max()))
