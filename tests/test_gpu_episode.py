"""GPU: a1mpc_episode_update_batch(_device) and a1mpc_episode_summary_batch(_device) -- the per-robot episode record and its deterministic batch summary.  Yardstick:
the numpy restatement of tests/episode_ref.py, bit for bit (neither kernel calls a library function: there is no bar in this file); what must hold on the device itself
(a repeated call, a side stream, the host entry against the device entry, rows beyond n); every refusal of the header with poisoned arrays; and one closed loop, the
noisy trot of tests/test_gpu_noise.py with robot 5 pushed over (tests/episode_loop.py), whose records are read with ONE copy at the end and held to what numpy makes of
per-tick copies of a second run.  One handle of 4224 robots, gazebo parameter set, h = 10, cold solves."""
import ctypes as C

import numpy as np
import pytest

import episode_loop as EL
import episode_ref as ER
import noise_ref as NR
import sensor_loop as SL
import walk_loop as WL
from gpu_common import _engine, tick_buffers, tick_world

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 65, 257]
SUMMARY_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]
MAX_BATCH = 4224
TAIL = 3
POISON = 0x7FF8DEADBEEF0001
NAMES = ("root_pos", "root_lin_vel", "root_lin_vel_d", "root_pos_d_z", "ground", "grf_body", "contacts", "status", "reach")
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
    e = _engine(pkg, scen.scenario_stand(), MAX_BATCH, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


def _inputs(stride):
    """three ticks of inputs for 260 robots per stride: computed once, never changed"""
    if stride not in _SHARED:
        _SHARED[stride] = ER.random_inputs(max(SIZES) + TAIL, seed=9100 + stride, stride=stride, ticks=3)
    return _SHARED[stride]


def _device(eng, ep, tick, d, n, skip=(), stream=None, cfg=None):
    """the device entry on a copy of `ep` (all its rows on the device, the first n worked on) -> the copy"""
    import torch
    t = {k: _t(v) for k, v in d.items() if v is not None and k not in skip}
    e = _t(ep)
    torch.cuda.synchronize()
    eng.episode_update_device(n, tick, e, t["state"], d["state"].shape[1], t["R"], **{"d_" + k: t.get(k) for k in NAMES}, config=cfg, stream=stream)
    torch.cuda.synchronize()
    return e.cpu().numpy()


def _host(eng, ep, tick, d, n):
    e = np.array(ep[:n])
    return eng.episode_update(e, tick, d["state"][:n], d["R"][:n], **{k: d[k][:n] for k in NAMES})


def _summary_device(eng, ep, n, stream=None):
    import torch
    e = _t(ep); out = torch.full((20 + TAIL,), float("nan"), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    eng.episode_summary_device(n, e, out, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_update_entries_equal_the_restatement(eng, n):
    """the first n of 260 rows, every input given, the three strides, three consecutive ticks from the all-zero record: every bit of every record from the device entry
    and from the host entry, and the rows beyond n keep their poison"""
    for stride in (12, 13, 22):
        ref = np.zeros((n, ER.WORDS))
        dev = np.zeros((n + TAIL, ER.WORDS)); dev[n:].view(np.uint64)[:] = POISON
        hst = np.zeros((n, ER.WORDS))
        for t, d in enumerate(_inputs(stride)):
            ref = ER.update(ref, 2 ** 40 + t, **{k: v[:n] for k, v in d.items()})
            dev = _device(eng, dev, 2 ** 40 + t, d, n)
            hst = _host(eng, hst, 2 ** 40 + t, d, n)
            assert ER.bits_equal(dev[:n], ref) and ER.bits_equal(hst, ref), (stride, t)
            assert (dev[n:].view(np.uint64) == POISON).all()
        assert (ref[:, 0] == 3).all()


def test_update_structure_on_the_device(eng):
    """a repeated call on a copy; a side stream; each optional input NULL keeps its words' payload; a NaN row ends its own episode alone; a frozen record keeps every
    bit; tilt before height; the last valid tick"""
    import torch
    n = 257
    ins = _inputs(12)
    d = ins[0]
    start = ER.update(np.zeros((n, ER.WORDS)), 0, **{k: v[:n] for k, v in ins[1].items()})
    once = _device(eng, start, 1, d, n)
    assert ER.bits_equal(once, ER.update(start, 1, **{k: v[:n] for k, v in d.items()}))
    assert ER.bits_equal(_device(eng, start, 1, d, n), once)
    assert ER.bits_equal(_device(eng, start, 1, d, n, stream=torch.cuda.Stream().cuda_stream), once)
    for key in ER.OPTIONAL:
        p = np.array(start); p.view(np.uint64)[:, list(ER.WORDS_OF[key])] = POISON
        less = ER.without({k: v[:n] for k, v in d.items()}, key)
        out = _device(eng, p, 1, less, n)
        assert ER.bits_equal(out, ER.update(p, 1, **less)) and (out[:, list(ER.WORDS_OF[key])].view(np.uint64) == POISON).all(), key
    bad = {k: np.array(v[:n]) for k, v in d.items()}
    bad["state"][37, 3] = np.nan; bad["R"][38, 8] = 0.4; bad["state"][38, 5] = 0.01; bad["state"][39, 5] = 0.01
    bad["contacts"][40] = (0, 1, 1, 1); bad["grf_body"][40, 0:3] = np.nan   # (a swing leg's force: not read)
    out = _device(eng, start, 2 ** 53 - 2, bad, n)
    assert ER.bits_equal(out, ER.update(start, 2 ** 53 - 2, **bad))
    assert list(out[37:41, 2]) == [1, 2, 3, 0] and (out[37:40, 1] == 2.0 ** 53 - 1).all()
    keep = np.ones(n, bool); keep[37:41] = False
    assert ER.bits_equal(out[keep], once[keep])
    nan = {k: (np.full(v.shape, np.nan) if v.dtype == np.float64 else v) for k, v in bad.items()}
    again = _device(eng, out, 9, nan, n)
    assert ER.bits_equal(again[37:40], out[37:40]) and (again[keep, 2] == 1).all()


@pytest.mark.parametrize("n", SUMMARY_SIZES)
def test_summary_entries_equal_the_restatement(eng, n):
    """one, two and three launch levels, either side of every edge: all 20 words from both entries, row n poisoned and nothing written behind the 20 words"""
    ep = np.vstack([ER.random_records(n, seed=9200 + n), np.full((1, ER.WORDS), np.nan)])
    ref = ER.summary(ep[:n])
    out = _summary_device(eng, ep, n)
    assert ER.bits_equal(out[:20], ref), (out, ref)
    assert np.isnan(out[20:]).all()
    assert ER.bits_equal(eng.episode_summary(ep[:n]), ref)


def test_summary_structure_on_the_device(eng):
    """a repeated call and a side stream give the same bits; the lowest row wins a tie across workgroups and levels; -1 when nobody ended"""
    import torch
    n = 4200
    ep = ER.random_records(n, seed=9900)
    ep[:, 5] = np.minimum(ep[:, 5], 0.4)
    for g in (4150, 77, 2000):
        ep[g, 5] = 0.45
    out = _summary_device(eng, ep, n)
    assert ER.bits_equal(out[:20], ER.summary(ep)) and out[10] == 77
    assert ER.bits_equal(_summary_device(eng, ep, n), out) and ER.bits_equal(_summary_device(eng, ep, n, stream=torch.cuda.Stream().cuda_stream), out)
    ep[:, 1:3] = 0
    out = _summary_device(eng, ep, n)
    assert out[5] == -1 and out[1] == n and ER.bits_equal(out[:20], ER.summary(ep))


def test_refusals_leave_the_arrays_untouched(eng):
    """every refusal of the header: A1MPC_ERR_INVALID_ARGUMENT (1) from both entries of both calls, the field named in a1mpc_last_error, before any launch; n > max_batch
    is A1MPC_ERR_BATCH_TOO_LARGE; n == 0 is OK and writes nothing; the same arguments, accepted, do write"""
    import torch
    n = 16
    L = eng.lib
    d = {k: np.array(v[:n]) for k, v in _inputs(12)[0].items()}
    order = ("state", "R") + NAMES
    dev = {k: _t(d[k]) for k in order}
    dev["episode"] = torch.full((n, 16), float("nan"), dtype=torch.float64, device=_dev()); dev["summary"] = torch.full((20,), float("nan"), dtype=torch.float64, device=_dev())
    hst = dict(d, episode=np.full((n, 16), np.nan), summary=np.full(20, np.nan))
    ctype = {np.dtype("float64"): C.c_double, np.dtype("uint8"): C.c_uint8, np.dtype("int32"): C.c_int32}
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(ctype[a.dtype]))

    def update(cfg=ER.DEFAULT, n_=n, tick=7, stride=12, h=eng._h, **swap):
        ec = None if cfg is None else C.byref(eng.episode_config(**cfg))
        dv, hs = dict(dev), dict(hst)
        for k, (a, b) in swap.items():
            dv[k], hs[k] = a, b
        rd = L.a1mpc_episode_update_batch_device(h, ec, n_, tick, ptr(dv["state"]), stride, ptr(dv["R"]), *[ptr(dv[k]) for k in NAMES], ptr(dv["episode"]), None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_episode_update_batch(h, ec, n_, tick, hp(hs["state"]), stride, hp(hs["R"]), *[hp(hs[k]) for k in NAMES], hp(hs["episode"]))
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    def summary(n_=n, h=eng._h, **swap):
        dv, hs = dict(dev), dict(hst)
        for k, (a, b) in swap.items():
            dv[k], hs[k] = a, b
        rd = L.a1mpc_episode_summary_batch_device(h, n_, ptr(dv["episode"]), ptr(dv["summary"]), None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_episode_summary_batch(h, n_, hp(hs["episode"]), hp(hs["summary"]))
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    nan, inf, none = float("nan"), float("inf"), (None, None)
    bad = [(dict(h=None), "null handle"), (dict(h=None, n_=-1, stride=5, cfg=None), "null handle"), (dict(cfg=None), "a1mpc_episode_config"), (dict(state=none), "state"),
           (dict(R=none), "R_world"), (dict(episode=none), "episode"), (dict(n_=-1), "negative n"), (dict(tick=2 ** 53 - 1), "tick"), (dict(tick=2 ** 64 - 1), "tick"),
           (dict(root_pos=none), "together"), (dict(root_lin_vel=none), "together"), (dict(grf_body=none), "together"), (dict(contacts=none), "together"),
           (dict(episode=(dev["grf_body"], hst["grf_body"])), "overlaps"), (dict(state=(dev["episode"], hst["episode"])), "overlaps"),
           (dict(reach=(dev["episode"].view(torch.uint8)[8:], hst["episode"].view(np.uint8)[8:])), "overlaps")]
    bad += [(dict(stride=s), "state_stride") for s in (0, 11, 14, 21, -12)]
    bad += [(dict(cfg=dict(ER.DEFAULT, min_up=v)), "min_up") for v in (nan, inf, -inf, 1.0000001, -1.5)]
    bad += [(dict(cfg=dict(ER.DEFAULT, min_height=v)), "min_height") for v in (nan, inf, -inf)]
    for kw, word in bad:
        rd, md, rh, mh = update(**kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    for kw, word in [(dict(h=None), "null handle"), (dict(h=None, n_=-1), "null handle"), (dict(episode=none), "episode"), (dict(summary=none), "summary_out"),
                     (dict(n_=-1), "negative n"), (dict(summary=(dev["episode"][3], hst["episode"][3])), "overlaps")]:
        rd, md, rh, mh = summary(**kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    big = MAX_BATCH + 1
    big_dev = {k: torch.zeros((big,) + tuple(d[k].shape[1:]), dtype=dev[k].dtype, device=_dev()) for k in order}
    big_hst = {k: np.zeros((big,) + d[k].shape[1:], d[k].dtype) for k in order}
    big_dev["episode"] = torch.full((big, 16), float("nan"), dtype=torch.float64, device=_dev()); big_hst["episode"] = np.full((big, 16), np.nan)
    rd, md, rh, mh = update(n_=big, **{k: (big_dev[k], big_hst[k]) for k in big_dev})
    assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    rd, md, rh, mh = summary(n_=big, episode=(big_dev["episode"], big_hst["episode"]))
    assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    for f in (update, summary):
        rd, md, rh, mh = f(n_=0)
        assert rd == OK and rh == OK, (md, mh)
    torch.cuda.synchronize()
    assert torch.isnan(big_dev["episode"]).all().item() and np.isnan(big_hst["episode"]).all()
    assert torch.isnan(dev["episode"]).all().item() and torch.isnan(dev["summary"]).all().item() and np.isnan(hst["episode"]).all() and np.isnan(hst["summary"]).all()
    assert all(ER.bits_equal(dev[k].cpu().numpy().astype(np.float64), d[k].astype(np.float64)) and ER.bits_equal(hst[k].astype(np.float64), d[k].astype(np.float64)) for k in order)
    dev["episode"].zero_(); hst["episode"][:] = 0.0
    rd, md, rh, mh = update(cfg=dict(min_up=-1.0, min_height=-0.0), tick=2 ** 53 - 2)   # (the same arrays, accepted, are written; the ends of the ranges)
    assert rd == OK and rh == OK, (md, mh)
    rd, md, rh, mh = summary()
    assert rd == OK and rh == OK, (md, mh)
    torch.cuda.synchronize()
    e = dev["episode"].cpu().numpy()
    assert (e[:, 0] == 1).all() and ER.bits_equal(e, hst["episode"]) and ER.bits_equal(e, ER.update(np.zeros((n, 16)), 2 ** 53 - 2, cfg=dict(min_up=-1.0, min_height=-0.0), **d))
    assert ER.bits_equal(dev["summary"].cpu().numpy(), hst["summary"]) and ER.bits_equal(hst["summary"], ER.summary(e))


# ---- the pushed trot on the device
def _pushed_trot(eng, pkg, scen, copying):
    """the noisy trot of tests/test_gpu_noise.py under episode_loop.wrench, a1mpc_episode_update_batch_device behind every walk step on the loop's stream.  copying False:
    nothing is copied until the end -> (records, summary, None); copying True: the truth and the estimate are copied to the host after every closed tick ->
    (records, summary, the copies)"""
    import torch
    E = pkg.engine
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
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
    pushes = [_t(EL.wrench(n, EL.PUSH_FIRST - 1)), _t(EL.wrench(n, EL.PUSH_FIRST))]   # (no push, the push)
    assert not pushes[0].any().item() and pushes[1][EL.ROBOT, 3].item() == EL.TORQUE
    episode, summary = Z(n, ER.WORDS), Z(ER.SUMMARY)
    nc = eng.noise_config(**NR.NOMINAL)
    ec = eng.episode_config()
    wc = eng.walk_config(dt=SL.CONTROL_DT, swing_track=1.0, flat_ground=1, ground_z=0.0)
    T = WL.PRIME + WL.STAND + WL.WALK
    stream = torch.cuda.Stream()
    copies = dict(state=[], R=[], vel=[]) if copying else None
    torch.cuda.synchronize()
    for t in range(T):
        first = t <= WL.PRIME
        ext = pushes[1 if EL.PUSH_FIRST <= t < EL.PUSH_FIRST + EL.PUSH_TICKS else 0]
        if t in (WL.PRIME + WL.STAND, WL.PRIME + WL.STAND + 1):
            with torch.cuda.stream(stream):
                stick["mode_toggle"].copy_(one if t == WL.PRIME + WL.STAND else zero); stick["cmd"].copy_(walk_cmd)
        eng.walk_sensors_device(n, state, 12, R, foot, grf_eq if first else w["outs"]["grf"], ct_all if first else w["u8"]["contacts"], syn["quat"], syn["imu_acc_raw"],
                                syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], syn["reach"], d_ext_wrench=ext, d_foot_vel_body=fvb,
                                stream=stream.cuda_stream)
        eng.sensor_noise_device(nc, n, t, syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], bias,
                                stream=stream.cuda_stream)
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=stream.cuda_stream)
        if t >= WL.PRIME:
            eng.walk_step_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], front["R_z"], w["state"]["foot_pos_target_last_time"], fvb, d_ext_wrench=ext,
                                 walk=wc, stream=stream.cuda_stream)
            eng.episode_update_device(n, t, episode, state, 12, R, d_root_pos=w["state"]["root_pos"], d_root_lin_vel=w["state"]["root_lin_vel"],
                                      d_root_lin_vel_d=front["root_lin_vel_d"], d_root_pos_d_z=front["root_pos_d_z"], d_grf_body=w["outs"]["grf"],
                                      d_contacts=w["u8"]["contacts"], d_status=w["i32"]["status"], d_reach=syn["reach"], config=ec, stream=stream.cuda_stream)
            if copying:
                stream.synchronize()
                copies["state"].append(state.cpu().numpy()); copies["R"].append(R.cpu().numpy()); copies["vel"].append(w["state"]["root_lin_vel"].cpu().numpy())
    eng.episode_summary_device(n, episode, summary, stream=stream.cuda_stream)
    stream.synchronize()
    out = torch.cat([episode.reshape(-1), summary]).cpu().numpy()   # the run's ONE copy: 17 x 16 + 20 doubles
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    return out[:n * ER.WORDS].reshape(n, ER.WORDS), out[n * ER.WORDS:], copies


def test_pushed_trot_on_the_device(eng, pkg, scen):
    """17 robots, robot 5 takes a roll torque of 150 N m for 60 ticks of the walk (no leg force can hold it: a physical fall).  From the run's one copy: the pushed robot
    ended by tilt or height inside the push window, the other 16 alive with all 460 closed ticks; the summary is the restatement's of those records; and the alive
    robots' tilt_max, est_vel_err_max, x0 / y0 and dist2 are, bit for bit, what numpy makes of the per-tick copies of a second run of the same seeded loop"""
    n = 17
    ep, summ, _ = _pushed_trot(eng, pkg, scen, copying=False)
    others = np.arange(n) != EL.ROBOT
    print("the pushed robot:", dict(zip(ER.FIELDS, ep[EL.ROBOT])))
    print("summary:", dict(zip(ER.SUMMARY_FIELDS, summ)))
    assert ep[EL.ROBOT, 2] in (2, 3) and EL.PUSH_FIRST <= ep[EL.ROBOT, 1] - 1 < EL.PUSH_FIRST + EL.PUSH_TICKS
    assert ep[EL.ROBOT, 0] == ep[EL.ROBOT, 1] - 1 - WL.PRIME
    assert (ep[others, 2] == 0).all() and (ep[others, 1] == 0).all() and (ep[others, 0] == EL.CLOSED).all()
    assert np.isfinite(ep).all() and (ep[others, 11] == 0).all() and (ep[others, 12] == 0).all()
    assert ER.bits_equal(summ, ER.summary(ep))
    assert list(summ[:5]) == [n, n - 1, 0, ep[EL.ROBOT, 2] == 2, ep[EL.ROBOT, 2] == 3] and summ[5] == ep[EL.ROBOT, 1] - 1
    ep2, summ2, cp = _pushed_trot(eng, pkg, scen, copying=True)
    assert ER.bits_equal(ep2, ep) and ER.bits_equal(summ2, summ)   # (the loop is reproducible)
    st, R, vel = np.stack(cp["state"]), np.stack(cp["R"]), np.stack(cp["vel"])
    assert st.shape[0] == EL.CLOSED
    d = vel - st[:, :, 9:12]
    verr = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).max(0)
    tilt = np.maximum((1.0 - R[:, :, 8]).max(0), 0.0)
    dx, dy = st[-1, :, 3] - st[0, :, 3], st[-1, :, 4] - st[0, :, 4]
    assert ER.bits_equal(ep[others, 5], tilt[others]) and ER.bits_equal(ep[others, 8], verr[others])
    assert ER.bits_equal(ep[others, 13:15], st[0][others, 3:5]) and ER.bits_equal(ep[others, 15], (dx * dx + dy * dy)[others])
