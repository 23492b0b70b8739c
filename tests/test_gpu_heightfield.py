"""GPU: a1mpc_heightfield_step_batch(_device) and a1mpc_heightfield_sample_batch(_device) -- the walk step over ONE gridded height field with an origin row per robot, a
touch byte per leg and the ground_out row of the episode record, and the sampling rule on its own.  Yardsticks: the elementwise numpy restatement of
tests/heightfield_ref.py (pos, R, v, omega, feet, foot_vel_body, touch and ground_out BIT FOR BIT, the angles within the walk tests' bar; the heights bit for bit);
a1mpc_ground_step_batch_device, which a constant field must reduce to bit for bit; and the closed loops  touch sensors -> tick -> height-field step  on one stream
against the same loops on the CPU (tests/heightfield_loop.py), with ground_out chained into the episode record.  One handle of 512 robots, gazebo parameter set, h = 10,
cold solves."""
import ctypes as C

import numpy as np
import pytest

import episode_ref as ER
import ground_loop as GL
import heightfield_cases as HC
import heightfield_loop as HL
import heightfield_ref as HR
import plant_ref as PR
import sensor_loop as SL
import walk_loop as WL
from gpu_common import _engine, tick_buffers, tick_world

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 65, 257]
NMAX = HC.NMAX
TAIL = 3
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
    _SHARED.clear()
    e.close()


def _on_device(eng, f):
    """the Field on the engine's device (Engine.heightfield), made once per field"""
    if ("dev", id(f)) not in _SHARED:
        _SHARED[("dev", id(f))] = (f, eng.heightfield(f.H, f.x0, f.y0, f.dx, f.dy, f.interp))   # (the Field is kept with it: its id stays its own)
    return _SHARED[("dev", id(f))][1]


def _device_step(eng, pkg, sc, n, k, stride=22, stream=None, sl=None, flags=None, field=None, ground_entry=None):
    """the device entry on the first n robots (or the slice sl) in configuration k of heightfield_cases.CONFIGS -> numpy (state (n + TAIL, stride), R, foot, foot_vel_body,
    touch, ground_out or None): poisoned outputs, or in place.  ground_entry (n, 3): a1mpc_ground_step_batch_device on those planes instead"""
    import torch
    sl = slice(0, n) if sl is None else sl
    sub, track, name = HC.CONFIGS[k]
    with_origin, with_out, in_place = HC.flags(k) if flags is None else flags
    f = _on_device(eng, HC.fields(pkg)[name] if field is None else field)
    st = _t(sc["wide"][sl, :stride]); R = _t(sc["R"][sl]); foot = _t(sc["foot"][sl]); grf = _t(sc["grf"][sl]); ct = _t(sc["contacts"][sl])
    Rz, tg = _t(sc["Rz"][sl]), _t(sc["target"][sl])
    og = _t(sc["origin"][sl]) if with_origin else None
    ew = _t(sc["ext"][sl]) if sub == 3 else None
    so, Ro, fo = (None, None, None) if in_place else (_nan(n + TAIL, stride), _nan(n + TAIL, 9), _nan(n + TAIL, 12))
    vo, to, go = _nan(n + TAIL, 12), _ff(n + TAIL), _nan(n + TAIL, 3) if with_out else None
    wc = eng.walk_config(substeps=sub, swing_track=track)
    torch.cuda.synchronize()
    if ground_entry is not None:
        eng.walk_step_ground_device(n, st, stride, R, foot, grf, ct, Rz, tg, vo, to, _t(ground_entry[sl]), ew, so, Ro, fo, walk=wc, stream=stream)
    else:
        eng.walk_step_heightfield_device(n, st, stride, R, foot, grf, ct, Rz, tg, vo, to, f, og, ew, so, Ro, fo, walk=wc, stream=stream, d_ground_out=go)
    torch.cuda.synchronize()
    if in_place:
        so, Ro, fo = st, R, foot
    return so.cpu().numpy(), Ro.cpu().numpy(), fo.cpu().numpy(), vo.cpu().numpy(), to.cpu().numpy(), None if go is None else go.cpu().numpy()


def _assert_is_ref(out, ref, n, rows=slice(None)):
    so, Ro, fo, vo, to, go = out
    assert PR.bits_equal(so[:n, 3:12], ref[0][rows][:n, 3:12]) and PR.bits_equal(Ro[:n], ref[1][rows][:n]) and PR.bits_equal(fo[:n], ref[2][rows][:n])
    assert PR.bits_equal(vo[:n], ref[3][rows][:n]) and np.array_equal(to[:n], ref[4][rows][:n])
    if go is not None:
        assert PR.bits_equal(go[:n], ref[5][rows][:n]) and np.isnan(go[n:]).all()
    worst = float(np.abs(so[:n, :3] - ref[0][rows][:n, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_step_device_and_host_entries_equal_the_restatement_bit_for_bit(eng, pkg, scen, n):
    """the first n of 257 robots in the 48 configurations of the CPU test (sub-steps 1 and 3 with a wrench, swing_track 0 / 0.5 / 1, the eight fields, with and without
    origin and ground_out, in place and out of place), on a side stream: the device entry writes the restatement's bits, nothing beyond row n and nothing into words
    [12:22) of the tick records; the host entry returns the device entry's bits"""
    import torch
    sc = HC.walkers(scen)
    stream = torch.cuda.Stream()
    worst = 0.0
    for k, (sub, track, name) in enumerate(HC.CONFIGS):
        with_origin, with_out, in_place = HC.flags(k)
        out = _device_step(eng, pkg, sc, n, k, stream=stream.cuda_stream)
        assert np.isnan(out[3][n:]).all() and (out[4][n:] == 0xFF).all() and (out[5] is None) == (not with_out)
        if in_place:
            assert np.array_equal(out[0][:, 12:], sc["wide"][:n, 12:])
        else:
            assert all(np.isnan(a[n:]).all() for a in out[:3]) and np.isnan(out[0][:n, 12:]).all()
        assert not any(np.isnan(a[:n, :w]).any() for a, w in zip(out[:4], (12, 9, 12, 12)))
        worst = max(worst, _assert_is_ref(out, HC.ref(pkg, scen, k), n))
        h = eng.walk_step_heightfield(sc["wide"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n], sc["target"][:n],
                                      _on_device(eng, HC.fields(pkg)[name]), sc["origin"][:n] if with_origin else None, sc["ext"][:n] if sub == 3 else None,
                                      walk=eng.walk_config(substeps=sub, swing_track=track), ground_out=with_out)
        assert PR.bits_equal(h["state"][:, :12], out[0][:n, :12]) and PR.bits_equal(h["R"], out[1][:n]) and PR.bits_equal(h["foot"], out[2][:n])
        assert PR.bits_equal(h["foot_vel_body"], out[3][:n]) and np.array_equal(h["state"][:, 12:], sc["wide"][:n, 12:]) and np.array_equal(h["touch"], out[4][:n])
        assert (h["ground"] is None) if not with_out else PR.bits_equal(h["ground"], out[5][:n])
    print(f"n {n}: {len(HC.CONFIGS)} configurations, device and host entries carry the restatement's bits; angles within {worst:.1e}")


@pytest.mark.parametrize("with_origin", [False, True])
def test_sample_entries_on_the_edge_cases(eng, pkg, with_origin):
    """every field, and the two at the world's origin where X = -1e-300 and X = -0.0 reach the rule as such, on the edge points of the CPU test (nodes, the last node of each axis, beyond every side and corner, -1e-300, -0.0, +-inf, NaN in X only and in Y only),
    with and without an origin row: the device entry (side stream) and the host entry write the restatement's bits, a NaN exactly where X or Y is one, a finite height
    for +-inf, and nothing beyond the last point"""
    import torch
    rng = np.random.default_rng(9800)
    stream = torch.cuda.Stream()
    tiny = 0
    for name, f in HC.point_fields(pkg).items():
        pts = HC.edge_points_few(f)
        n = len(pts)
        assert n <= 512
        origin = None
        if with_origin:
            origin, pts = HC.point_origins(rng, pts)
        tiny += HC.tiny_points_reach_the_rule(f, pts, origin)   # (asserts ux = -1e-300 / dx and ux = -0.0 on the two fields at the world's origin)
        ref = HR.sample(f, pts[:, 0], pts[:, 1], origin)
        out = torch.full((n + TAIL,), -1e300, dtype=torch.float64, device=_dev())
        xy, og = _t(pts), _t(origin)
        torch.cuda.synchronize()
        eng.heightfield_sample_device(_on_device(eng, f), n, xy, out, og, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == -1e300).all() and HR.same_heights(got[:n], ref), name
        nan = np.isnan(pts).any(axis=1)
        assert nan.sum() == 4 and np.array_equal(np.isnan(got[:n]), nan) and np.isinf(pts[~nan]).any(axis=1).sum() == 6
        assert HR.same_heights(eng.heightfield_sample(_on_device(eng, f), pts, origin), ref), name
    assert tiny == 2


def test_step_reductions_a_robot_alone_and_strides(eng, pkg, scen):
    """a constant field of the value c (both interp), origin NULL: every other output is a1mpc_ground_step_batch_device's with ground = (c, 0, 0), run here, bit for bit,
    and ground_out is (c, 0, 0); robot i alone has the bits of robot i of the 257, whatever wavefront and lane it sat in, and so has a batch cut out of the middle;
    strides 12 and 13 give the same bits"""
    sc = HC.walkers(scen)
    c = 0.0375
    level = np.tile([c, 0.0, 0.0], (NMAX, 1))
    same = lambda g, w, n: all(PR.bits_equal(x[:n], y[:n]) for x, y in zip(g[:4], w[:4])) and np.array_equal(g[4][:n], w[4][:n])
    for interp, k in ((0, 0), (1, 17), (1, 40)):
        f = HR.Field(np.full((2, 3) if interp else (1, 1), c), -0.3, 0.2, 0.4, 0.7, interp)
        flags = (False, True, False)
        h = _device_step(eng, pkg, sc, NMAX, k, flags=flags, field=f)
        g = _device_step(eng, pkg, sc, NMAX, k, flags=flags, ground_entry=level)
        assert same(h, g, NMAX) and PR.bits_equal(h[5][:NMAX], level), (interp, k)
        assert (g[4][:NMAX][sc["contacts"] == 0] == 1).any() and (g[4][:NMAX][sc["contacts"] == 0] == 0).any()
    k = 47   # (3 sub-steps, swing_track 1, the 64 x 48 bilinear field)
    flags = (True, True, False)
    ref = HC.ref(pkg, scen, k) if HC.flags(k)[0] else HR.step(sc["params"], sc["wide"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"],
                                                              HC.fields(pkg)[HC.CONFIGS[k][2]], sc["origin"], sc["ext"], 0.0025, 3, swing_track=1.0)
    for i in (0, 63, 64, 200, 256):
        _assert_is_ref(_device_step(eng, pkg, sc, 1, k, sl=slice(i, i + 1), flags=flags), ref, 1, rows=slice(i, i + 1))
    _assert_is_ref(_device_step(eng, pkg, sc, 37, k, sl=slice(100, 137), flags=flags), ref, 37, rows=slice(100, 137))
    for stride in (12, 13):
        out = _device_step(eng, pkg, sc, 65, k, stride=stride, flags=flags)
        _assert_is_ref(out, ref, 65)
        assert np.isnan(out[0][:65, 12:]).all() and all(np.isnan(a[65:]).all() for a in out[:4]) and (out[4][65:] == 0xFF).all()


def test_refusals_leave_the_outputs_untouched(eng, pkg, scen):
    """every refusal of the field and of the ground step, from both step entries and both sample entries: A1MPC_ERR_INVALID_ARGUMENT (1) with the argument named, before any
    launch; a field of more than 2^20 nodes and n > max_batch are A1MPC_ERR_BATCH_TOO_LARGE (5), the former from the host-pointer entries alone; n == 0 is OK and writes
    nothing.  The poisoned outputs stay poisoned throughout; the same arguments, accepted, do write"""
    import torch
    sc = HC.walkers(scen)
    n = 16
    L = eng.lib
    keys = ("wide", "R", "foot", "grf", "contacts", "Rz", "target")
    names = ["state_in", "R_world", "foot_abs", "grf_body", "contacts", "R_z", "foot_target"]
    ins = [_t(sc[k][:n]) for k in keys]
    outs = [_nan(n, 22), _nan(n, 9), _nan(n, 12), _nan(n, 12), _ff(n), _nan(n, 3)]
    hins = [np.ascontiguousarray(sc[k][:n]) for k in keys]
    houts = [np.full((n, 22), np.nan), np.full((n, 9), np.nan), np.full((n, 12), np.nan), np.full((n, 12), np.nan), np.full((n, 4), 0xFF, np.uint8), np.full((n, 3), np.nan)]
    og, hog = _t(sc["origin"][:n]), np.ascontiguousarray(sc["origin"][:n])
    xy, hxy = _t(sc["wide"][:n, 3:5]), np.ascontiguousarray(sc["wide"][:n, 3:5])
    sout, hsout = _nan(n, 1), np.full(n, np.nan)
    good = _on_device(eng, HC.fields(pkg)["5x3/1"])
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))
    ref = lambda s: None if s is None else C.byref(s)

    def step(wc, n_, stride, dfield=good.struct, hfield=good.host, ins_=ins, outs_=outs, hins_=hins, houts_=houts):
        wp = None if wc is None else C.byref(wc)
        rd = L.a1mpc_heightfield_step_batch_device(eng._h, wp, n_, ptr(ins_[0]), stride, *[ptr(t) for t in ins_[1:5]], None, ptr(ins_[5]), ptr(ins_[6]), ref(dfield), ptr(og),
                                                   *[ptr(t) for t in outs_], None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_heightfield_step_batch(eng._h, wp, n_, hp(hins_[0]), stride, *[hp(a) for a in hins_[1:5]], None, hp(hins_[5]), hp(hins_[6]), ref(hfield), hp(hog),
                                            *[hp(a) for a in houts_])
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    def sample(n_, dfield=good.struct, hfield=good.host, xy_=True, out_=True, h=eng._h):
        rd = L.a1mpc_heightfield_sample_batch_device(h, ref(dfield), n_, ptr(xy) if xy_ else None, ptr(og), ptr(sout) if out_ else None, None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_heightfield_sample_batch(h, ref(hfield), n_, hp(hxy) if xy_ else None, hp(hog), hp(hsout) if out_ else None)
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    cfg = lambda **kw: eng.walk_config(**kw)
    nan, inf = float("nan"), float("inf")

    def variant(**kw):
        d, h = pkg.engine.Heightfield(), pkg.engine.Heightfield()
        C.memmove(C.byref(d), C.byref(good.struct), C.sizeof(d)); C.memmove(C.byref(h), C.byref(good.host), C.sizeof(h))
        for k, v in kw.items():
            setattr(d, k, v); setattr(h, k, v)
        return d, h

    fields_bad = [(dict(interp=2), "interp"), (dict(nx=1), "nx"), (dict(ny=0), "ny"), (dict(interp=0, nx=0), "nx"), (dict(nx=32769), "nx"), (dict(ny=40000), "ny"),
                  (dict(dx=0.0), "dx"), (dict(dx=nan), "dx"), (dict(dy=-1.0), "dy"), (dict(dy=inf), "dy"), (dict(x0=nan), "x0"), (dict(y0=-inf), "y0"), (dict(dx=1e-320), "1 / dx"),
                  (dict(dy=1e-320), "1 / dy"), (dict(height=None), "height")]
    for kw, word in fields_bad:
        d, h = variant(**kw)
        for rd, md, rh, mh in (step(cfg(), n, 22, d, h), sample(n, d, h)):
            assert rd == INVALID and rh == INVALID and "a1mpc_heightfield" in md and word in md and word in mh, (kw, rd, md, rh, mh)
    for rd, md, rh, mh in (step(cfg(), n, 22, None, None), sample(n, None, None)):
        assert rd == INVALID and rh == INVALID and "null a1mpc_heightfield" in md and "null a1mpc_heightfield" in mh
    # more than 2^20 nodes: the host-pointer entries refuse to stage it; the device entries take it (here with n = 0, so that nothing is launched on a field that is not there)
    d, h = variant(nx=1025, ny=1025)
    wc = cfg()
    rh = L.a1mpc_heightfield_step_batch(eng._h, C.byref(wc), n, hp(hins[0]), 22, *[hp(a) for a in hins[1:5]], None, hp(hins[5]), hp(hins[6]), C.byref(h), hp(hog), *[hp(a) for a in houts])
    assert rh == TOO_LARGE and "2^20" in L.a1mpc_last_error().decode()
    rh = L.a1mpc_heightfield_sample_batch(eng._h, C.byref(h), n, hp(hxy), hp(hog), hp(hsout))
    assert rh == TOO_LARGE and "2^20" in L.a1mpc_last_error().decode()
    assert L.a1mpc_heightfield_sample_batch_device(eng._h, C.byref(d), 0, ptr(xy), None, ptr(sout), None) == OK
    d, h = variant(nx=1024, ny=1024)   # (2^20 nodes exactly is within what is staged: refused for nothing; n = 0 again)
    assert L.a1mpc_heightfield_sample_batch(eng._h, C.byref(h), 0, hp(hxy), None, hp(hsout)) == OK
    bad = [(cfg(substeps=0), n, 22, "substeps"), (cfg(substeps=65), n, 22, "substeps"), (cfg(dt=0.0), n, 22, "dt"), (cfg(dt=nan), n, 22, "dt"),
           (cfg(gravity_z=inf), n, 22, "gravity_z"), (cfg(), n, 14, "state_stride"), (cfg(), n, 0, "state_stride"), (cfg(), -1, 22, "negative n"), (cfg(), 513, 22, "max_batch"),
           (None, n, 22, "a1mpc_walk_config"), (cfg(swing_track=-0.1), n, 22, "swing_track"), (cfg(swing_track=1.5), n, 22, "swing_track"), (cfg(swing_track=nan), n, 22, "swing_track")]
    for wc, n_, stride, word in bad:
        rd, md, rh, mh = step(wc, n_, stride)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    for k, name in enumerate(names):
        for track in ((1.0, 0.25) if k >= 5 else (1.0,)):
            rd, md, rh, mh = step(cfg(swing_track=track), n, 22, ins_=[None if j == k else t for j, t in enumerate(ins)], hins_=[None if j == k else t for j, t in enumerate(hins)])
            assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for k, name in enumerate(["state_out", "R_world_out", "foot_abs_out", "foot_vel_body_out", "touch_out"]):
        rd, md, rh, mh = step(cfg(), n, 22, outs_=[None if j == k else t for j, t in enumerate(outs)], houts_=[None if j == k else t for j, t in enumerate(houts)])
        assert rd == INVALID and rh == INVALID and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for kw, word in ((dict(n_=-1), "negative n"), (dict(xy_=False), "null xy"), (dict(out_=False), "null height_out"), (dict(h=None), "null handle")):
        kw = dict(kw); n_ = kw.pop("n_", n)
        rd, md, rh, mh = sample(n_, **kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, md, mh)
    rd, md, rh, mh = sample(513)
    assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    rd, _, rh, _ = step(cfg(), 0, 22)
    assert rd == OK and rh == OK
    rd, _, rh, _ = sample(0)
    assert rd == OK and rh == OK
    torch.cuda.synchronize()
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a
    untouched = lambda a: bool((host(a) == 0xFF).all()) if host(a).dtype == np.uint8 else bool(np.isnan(host(a)).all())
    assert all(untouched(o) for o in outs + houts + [sout, hsout])
    rd, md, rh, mh = step(cfg(flat_ground=1, ground_z=nan), n, 22)   # (cfg's plane is not read; these arguments, accepted, do write -- ground_out among them)
    assert rd == OK and rh == OK, (md, mh)
    rd, md, rh, mh = sample(n)
    torch.cuda.synchronize()
    assert rd == OK and rh == OK and not any(untouched(o) for o in outs[1:] + houts[1:] + [sout, hsout]), (md, mh)
    assert (host(outs[4]) <= 1).all() and (houts[4] <= 1).all() and not np.isnan(host(outs[5])).any() and not np.isnan(houts[5]).any()


# ---- the closed loops on the device
EPISODE_TICKS = 8   # ground_out is chained into the episode record over the last ticks


def _loop_terrain(pkg, sc, n, which):
    if which == "ramp":
        return HL.ramp_tiles(pkg.heightfields, sc, HL.loop_planes(sc, n)) + (0.0,)
    return HL.stairs_field(pkg.heightfields, sc, HL.STAIR_RISE, n) + (GL.TOUCH_FORCE,)


@pytest.mark.parametrize("which", ["ramp", "stairs"])
def test_closed_loop_touch_sensors_tick_heightfield_step_on_the_device(eng, pkg, oracle, scen, which):
    """17 perturbed standing robots, h = 10, cold solves, the schedule of tests/walk_loop.py: a1mpc_touch_sensors_batch_device -> a1mpc_control_tick_sensors_device ->
    a1mpc_heightfield_step_batch_device (in place, fed the tick's grf, contacts, R_z and foot_pos_target_last_time, writing the touch bytes the next tick's sensors read
    and ground_out), all on one stream without a host synchronisation between the first launch and the last; over the last 8 ticks ground_out goes straight into
    a1mpc_episode_update_batch_device on that stream.  ramp: a bilinear tile per robot of ONE field (heightfield_loop.loop_planes), touch_force 0; stairs: cell-constant
    stairs of rise HL.STAIR_RISE under every robot, touch_force 60.  conditions_hold (height above ground_out) stays empty on every tick, every touchdown is on the field
    within 1e-12, ground_out is the restatement's hf under the body bit for bit, the episode records are episode_ref's bit for bit, and against the same loop on the CPU
    (robots 0 .. 3): the end state's pos, v and angles within 1e-4, omega within 1e-3, and the early-contact ticks identical"""
    import torch
    E = pkg.engine
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
    field, origin, force = _loop_terrain(pkg, sc, n, which)
    assert eng.horizon == SL.H and eng.cfg.warm_start == 0 and eng.cfg.mass == sc["params"]["mass"]
    L = eng.lib
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm))
    assert prm.control_dt == SL.CONTROL_DT and prm.contact.use_terrain_adapt == 1 and prm.contact.foot_force_low == 30.0
    state, R, foot = _t(sc["state"]), _t(sc["R"]), _t(sc["foot"])
    grf_eq, ct_all = _t(sc["grf_eq"]), _t(sc["contact"])
    hf, og = eng.heightfield(field.H, field.x0, field.y0, field.dx, field.dy, field.interp), _t(origin)
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
    fvb, gout = Z(n, 12), Z(n, 3)
    touch = torch.ones((n, 4), dtype=torch.uint8, device=dev)   # (the unstepped plant stands on all four feet)
    episode = Z(n, ER.WORDS)
    T = WL.PRIME + WL.STAND + WL.WALK
    hist = dict(state=Z(T, n, 12), R=Z(T, n, 9), foot=Z(T, n, 12), status=Z(T, n, dt=torch.int32), reach=Z(T, n, 4, dt=torch.uint8), grf=Z(T, n, 12),
                contacts=Z(T, n, 4, dt=torch.uint8), plan=Z(T, n, 4, dt=torch.uint8), mode=Z(T, n, dt=torch.uint8), sensors=Z(T, n, 38), ground=Z(T, n, 3), pos_d_z=Z(T, n))
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
            eng.walk_step_heightfield_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], front["R_z"], w["state"]["foot_pos_target_last_time"], fvb, touch,
                                             hf, og, walk=wc, stream=stream.cuda_stream, d_ground_out=gout)
        if t >= T - EPISODE_TICKS:
            eng.episode_update_device(n, t, episode, state, 12, R, d_root_pos_d_z=front["root_pos_d_z"], d_ground=gout, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            hist["state"][t].copy_(state); hist["R"][t].copy_(R); hist["foot"][t].copy_(foot); hist["status"][t].copy_(w["i32"]["status"]); hist["reach"][t].copy_(syn["reach"])
            hist["grf"][t].copy_(w["outs"]["grf"]); hist["contacts"][t].copy_(w["u8"]["contacts"]); hist["plan"][t].copy_(w["u8"]["plan_contacts"])
            hist["mode"][t].copy_(front["movement_mode"]); hist["ground"][t].copy_(gout); hist["pos_d_z"][t].copy_(front["root_pos_d_z"])
            hist["sensors"][t].copy_(torch.cat([syn[k] for k in ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")], 1))
    torch.cuda.synchronize()
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state):
        assert reset(eng._h) == 0
    H = {k: v.cpu().numpy() for k, v in hist.items()}
    assert np.array_equal(H["state"][WL.PRIME - 1], sc["state"])   # (the plant was not stepped while the EKF was primed)
    w0 = WL.PRIME + WL.STAND
    assert not H["mode"][:w0].any() and (H["mode"][w0:] == 1).all()
    for t in range(WL.PRIME, T):
        under = HR.sample(field, H["state"][t][:, 3], H["state"][t][:, 4], origin)
        assert HR.same_heights(H["ground"][t][:, 0], under) and not H["ground"][t][:, 1:].any(), t   # ground_out: hf under the body as the restatement has it, (+0, +0)
        finite = np.isfinite(H["sensors"][t]).all() and np.isfinite(H["grf"][t]).all() and np.isfinite(H["state"][t]).all()
        bad = SL.conditions_hold(GL.above_plane(H["ground"][t], H["state"][t]), H["reach"][t], H["status"][t], finite)
        assert not bad, (t, bad)
    walk = {k: H[k][w0:] for k in ("contacts", "plan", "foot", "state", "R")}
    td, h = HL.heights_above_the_field(walk, field, origin)
    early = GL.early_contacts(walk)
    gain = H["ground"][-1][:, 0] - H["ground"][w0][:, 0]
    print(f"{which} on the device, {WL.WALK} ticks, {n} robots: {len(td)} touchdowns off the field by {np.abs(td).max():.1e} at most, lowest foot {h.min():.1e}; "
          f"{len(early)} early-contact ticks; ground_out gained {gain.min():.3f} .. {gain.max():.3f}")
    assert len(td) >= 12 * n and np.abs(td).max() <= GL.TOUCHDOWN and h.min() >= -GL.TOUCHDOWN
    if force == 0.0:
        assert not early and len(td) == 12 * n
    else:
        assert min(sum(1 for e in early if e[1] == b) for b in range(n)) >= 1 and gain.max() >= HL.STAIR_RISE - 1e-12
    # the episode record over the last ticks, fed ground_out on the stream: episode_ref's bits on the history
    ep = np.zeros((n, ER.WORDS))
    for t in range(T - EPISODE_TICKS, T):
        ep = ER.update(ep, t, H["state"][t], H["R"][t], root_pos_d_z=H["pos_d_z"][t], ground=H["ground"][t])
    assert ER.bits_equal(episode.cpu().numpy(), ep) and (ep[:, ER.W["ticks"]] == EPISODE_TICKS).all() and (ep[:, ER.W["height_err_sum"]] > 0).all()
    # the same loop on the CPU, the first 4 robots
    if which not in _SHARED:
        cpu = HL.HeightfieldLoop(oracle, scen, sc, 4, field, origin[:4], touch_force=force)
        _SHARED[which] = (HL.run(cpu, 4), cpu.x.copy())
    (chist, failed), x = _SHARED[which]
    assert not failed, failed[:3]
    d = lambda a, b: float(np.abs(a - b).max())
    end = H["state"][-1]
    figs = dict(pos=d(end[:4, 3:6], x[:, 3:6]), v=d(end[:4, 9:12], x[:, 9:12]), angles=d(end[:4, 0:3], x[:, 0:3]), omega=d(end[:4, 6:9], x[:, 6:9]))
    print(f"GPU loop against the CPU loop after {T - WL.PRIME} closed ticks:", ", ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert [e for e in early if e[1] < 4] == GL.early_contacts(chist)
    assert figs["pos"] <= 1e-4 and figs["v"] <= 1e-4 and figs["angles"] <= 1e-4 and figs["omega"] <= 1e-3
