"""GPU: a1mpc_plant_step_batch(_device) -- one control period of the nonlinear single rigid body under the forces of a solve.
Yardsticks: the elementwise numpy restatement of tests/plant_ref.py (pos, R, v, omega and the feet BIT FOR BIT, the angles within 1e-12: library atan2 / asin on
bit-identical arguments); physics that does not know the restatement (momentum, orthogonality, closed forms of free fall, equilibrium, the order of the scheme); the
reference's linear model at its linearisation point (a1mpc_horizon_states_batch); and the closed loop solve -> plant -> solve on the device against the same loop run with
the CPU oracle and the restatement.  One handle of 512 robots, gazebo parameter set."""
import ctypes as C

import numpy as np
import pytest

import plant_ref as PR
from gpu_common import _engine

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 64, 65, 257]   # one wavefront, its edges, several workgroups
NMAX = max(SIZES)
TAIL = 3


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(rows, w):
    import torch
    return torch.full((rows, w), float("nan"), dtype=torch.float64, device=_dev())


_SHARED = {}


@pytest.fixture(scope="module")
def eng(pkg, scen):
    e = _engine(pkg, scen.scenario_stand(), 512, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


def _cases(scen):
    """257 random robots as tick records, and the restatement's results for (1 sub-step, no wrench) and (4 sub-steps, a wrench): computed once, never changed"""
    if "sc" not in _SHARED:
        rng = np.random.default_rng(5100)
        sc = PR.random_robots(scen, rng, NMAX)
        sc["tick"] = np.ascontiguousarray(np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1))
        _SHARED["sc"] = sc
        _SHARED["ref"] = {(sub, ext): PR.step(sc["params"], sc["tick"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"] if ext else None, 0.0025, sub)
                          for sub, ext in ((1, False), (4, True))}
        for r in _SHARED["ref"].values():
            for a in r:
                a.setflags(write=False)
    return _SHARED["sc"], _SHARED["ref"]


def _device_step(eng, sc, n, sub, ext, stride=22, stream=None, in_place=False):
    """the device entry on the first n robots -> numpy (state (n + TAIL, stride), R, foot): NaN-poisoned outputs, or in place on copies of the inputs"""
    import torch
    st = _t(sc["tick"][:n, :stride]); R = _t(sc["R"][:n]); foot = _t(sc["foot"][:n]); grf = _t(sc["grf"][:n]); ct = _t(sc["contacts"][:n])
    ew = _t(sc["ext"][:n]) if ext else None
    so, Ro, fo = (None, None, None) if in_place else (_nan(n + TAIL, stride), _nan(n + TAIL, 9), _nan(n + TAIL, 12))
    torch.cuda.synchronize()
    eng.plant_step_device(n, st, stride, R, foot, grf, ct, ew, so, Ro, fo, plant=eng.plant_config(substeps=sub), stream=stream)
    torch.cuda.synchronize()
    if in_place:
        so, Ro, fo = st, R, foot
    return so.cpu().numpy(), Ro.cpu().numpy(), fo.cpu().numpy()


def _assert_is_ref(out, ref, n, stride):
    so, Ro, fo = out
    assert PR.bits_equal(so[:n, 3:12], ref[0][:n, 3:12]) and PR.bits_equal(Ro[:n], ref[1][:n]) and PR.bits_equal(fo[:n], ref[2][:n])
    worst = float(np.abs(so[:n, :3] - ref[0][:n, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("sub,ext", [(1, False), (4, True)])
@pytest.mark.parametrize("n", SIZES)
def test_device_and_host_entries_equal_the_restatement_bit_for_bit(eng, scen, n, sub, ext):
    """the first n of 257 robots (all 16 contact patterns from n = 16 on): the device entry writes the restatement's bits, nothing beyond row n and nothing into words
    [12:22) of the tick records; the host entry returns the device entry's bits"""
    sc, refs = _cases(scen)
    ref = refs[(sub, ext)]
    out = _device_step(eng, sc, n, sub, ext)
    assert all(np.isnan(a[n:]).all() for a in out) and np.isnan(out[0][:n, 12:]).all() and not any(np.isnan(a[:n, :w]).any() for a, w in zip(out, (12, 9, 12)))
    worst = _assert_is_ref(out, ref, n, 22)
    h = eng.plant_step(sc["tick"][:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["ext"][:n] if ext else None, plant=eng.plant_config(substeps=sub))
    assert PR.bits_equal(h["state"][:, :12], out[0][:n, :12]) and PR.bits_equal(h["R"], out[1][:n]) and PR.bits_equal(h["foot"], out[2][:n])
    assert np.array_equal(h["state"][:, 12:], sc["tick"][:n, 12:])
    print(f"n {n} substeps {sub} wrench {ext}: device and host entries carry the restatement's bits; angles within {worst:.1e}")


def test_in_place_strides_streams_and_a_robot_alone(eng, scen):
    """in place == out of place; strides 12 and 13 give the same bits and leave word 12 alone; a non-default stream; robot i alone has the bits of robot i of the 257"""
    import torch
    sc, refs = _cases(scen)
    ref = refs[(4, True)]
    n = 65
    si, Ri, fi = _device_step(eng, sc, n, 4, True, in_place=True)
    _assert_is_ref((si, Ri, fi), ref, n, 22)
    assert np.array_equal(si[:, 12:], sc["tick"][:n, 12:])   # the command half of the tick records survives the step in place
    for stride in (12, 13):
        out = _device_step(eng, sc, n, 4, True, stride=stride)
        _assert_is_ref(out, ref, n, stride)
        assert np.isnan(out[0][:n, 12:]).all() and all(np.isnan(a[n:]).all() for a in out)
        ip = _device_step(eng, sc, n, 4, True, stride=stride, in_place=True)
        _assert_is_ref(ip, ref, n, stride)
        assert np.array_equal(ip[0][:, 12:], sc["tick"][:n, 12:stride])
    stream = torch.cuda.Stream()
    out = _device_step(eng, sc, n, 4, True, stream=stream.cuda_stream)
    _assert_is_ref(out, ref, n, 22)
    for i in (0, 63, 64, 200, 256):
        one = {k: sc[k][i:i + 1] for k in ("tick", "R", "foot", "grf", "contacts", "ext")}
        o = _device_step(eng, one, 1, 4, True)
        assert PR.bits_equal(o[0][:1, 3:12], ref[0][i:i + 1, 3:12]) and PR.bits_equal(o[1][:1], ref[1][i:i + 1]) and PR.bits_equal(o[2][:1], ref[2][i:i + 1])


def test_non_finite_inputs_stay_with_their_robot(eng, scen):
    """a NaN force on every swing leg changes no bit; a NaN pos poisons pos of that robot and nothing else"""
    sc, refs = _cases(scen)
    ref = refs[(4, True)]
    n = 65
    swing = np.argwhere(sc["contacts"][:n] == 0)
    grf = sc["grf"].copy()
    for i, l in swing:
        grf[i, 3 * l + (i + l) % 3] = np.nan
    assert len(swing) > n
    out = _device_step(eng, dict(sc, grf=grf), n, 4, True)
    _assert_is_ref(out, ref, n, 22)
    tick = sc["tick"].copy(); tick[37, 4] = np.nan
    so, Ro, fo = _device_step(eng, dict(sc, tick=tick), n, 4, True)
    keep = np.arange(n) != 37
    assert PR.bits_equal(so[:n][keep, 3:12], ref[0][:n][keep, 3:12]) and PR.bits_equal(Ro[:n], ref[1][:n]) and PR.bits_equal(fo[:n][keep], ref[2][:n][keep])
    assert np.isnan(so[37, 4]) and np.isfinite(np.delete(so[37, :12], 4)).all()


def test_refusals_leave_the_outputs_untouched(eng, scen):
    """every refusal of the header: A1MPC_ERR_INVALID_ARGUMENT (1) from both entries, the field named in a1mpc_last_error, before any launch; n == 0 is OK and writes nothing"""
    import torch
    sc, _ = _cases(scen)
    n = 16
    L = eng.lib
    ins = [_t(sc["tick"][:n]), _t(sc["R"][:n]), _t(sc["foot"][:n]), _t(sc["grf"][:n]), _t(sc["contacts"][:n])]
    outs = [_nan(n, 22), _nan(n, 9), _nan(n, 12)]
    hins = [np.ascontiguousarray(sc[k][:n]) for k in ("tick", "R", "foot", "grf", "contacts")]
    houts = [np.full((n, 22), np.nan), np.full((n, 9), np.nan), np.full((n, 12), np.nan)]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_double))

    def call(pc, n_, stride, ins_=ins, outs_=outs, hins_=hins, houts_=houts):
        pcp = None if pc is None else C.byref(pc)
        rd = L.a1mpc_plant_step_batch_device(eng._h, pcp, n_, ptr(ins_[0]), stride, ptr(ins_[1]), ptr(ins_[2]), ptr(ins_[3]), ptr(ins_[4]), None, ptr(outs_[0]), ptr(outs_[1]),
                                             ptr(outs_[2]), None)
        md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_plant_step_batch(eng._h, pcp, n_, hp(hins_[0]), stride, hp(hins_[1]), hp(hins_[2]), hp(hins_[3]), hp(hins_[4]), None, hp(houts_[0]), hp(houts_[1]),
                                      hp(houts_[2]))
        mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    cfg = lambda **kw: eng.plant_config(**kw)
    bad = [(cfg(substeps=0), n, 22, "substeps"), (cfg(substeps=65), n, 22, "substeps"), (cfg(substeps=-3), n, 22, "substeps"), (cfg(dt=0.0), n, 22, "dt"),
           (cfg(dt=-0.0025), n, 22, "dt"), (cfg(dt=float("nan")), n, 22, "dt"), (cfg(dt=float("inf")), n, 22, "dt"), (cfg(gravity_z=float("nan")), n, 22, "gravity_z"),
           (cfg(gravity_z=float("-inf")), n, 22, "gravity_z"), (cfg(), n, 14, "state_stride"), (cfg(), n, 0, "state_stride"), (cfg(), -1, 22, "negative n"),
           (cfg(), 513, 22, "max_batch"), (None, n, 22, "a1mpc_plant_config")]
    for pc, n_, stride, word in bad:
        rd, md, rh, mh = call(pc, n_, stride)
        assert rd == 1 and rh == 1 and word in md and word in mh, (word, rd, md, rh, mh)
    for k, name in enumerate(["state_in", "R_world", "foot_abs", "grf_body", "contacts"]):
        rd, md, rh, mh = call(cfg(), n, 22, ins_=[None if j == k else t for j, t in enumerate(ins)], hins_=[None if j == k else t for j, t in enumerate(hins)])
        assert rd == 1 and rh == 1 and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    for k, name in enumerate(["state_out", "R_world_out", "foot_abs_out"]):
        rd, md, rh, mh = call(cfg(), n, 22, outs_=[None if j == k else t for j, t in enumerate(outs)], houts_=[None if j == k else t for j, t in enumerate(houts)])
        assert rd == 1 and rh == 1 and ("null " + name) in md and ("null " + name) in mh, (name, md, mh)
    rd, _, rh, _ = call(cfg(), 0, 22)
    assert rd == 0 and rh == 0
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all().item() for o in outs) and all(np.isnan(o).all() for o in houts)
    rd, _, rh, _ = call(cfg(), n, 22)   # (the same arguments, accepted, do write)
    torch.cuda.synchronize()
    assert rd == 0 and rh == 0 and not torch.isnan(outs[1]).any().item() and not np.isnan(houts[1]).any()


# ---- physics that does not know the restatement: 64 random robots, the host entry called 400 times
def _gpu_stepper(eng):
    def go(st, R, foot, grf, ct, ext, dt, substeps):
        o = eng.plant_step(st, R, foot, grf, ct, ext, plant=eng.plant_config(dt=dt, substeps=substeps))
        return o["state"], o["R"], o["foot"]
    return go


def test_torque_free_flight_keeps_orthogonality_and_the_swing_feet(eng, scen):
    dL, orth, feet = PR.torque_free_flight(_gpu_stepper(eng), scen)
    print(f"400 calls without contacts: |R R' - I| {orth:.1e}, swing feet in the body frame {feet:.1e} (|dL| / |L| {dL:.1e})")
    assert orth <= 1e-12 and feet <= 1e-10


def test_torque_free_flight_keeps_world_angular_momentum(eng, scen):
    """R I_b R' omega after 400 CALLS against before, relative, the worst of 64 robots; bar 1e-12 (7e-14 on the restatement, whose bits the kernel has; 1.8e-12 without
    step 0 of the scheme: see tests/test_plant_host.py)."""
    dL, _, _ = PR.torque_free_flight(_gpu_stepper(eng), scen)
    print(f"400 calls without contacts: |dL| / |L| {dL:.2e}")
    assert dL <= 1e-12


def test_free_fall_follows_the_closed_forms(eng, scen):
    dv, dz = PR.free_fall(_gpu_stepper(eng), scen)
    print(f"400 calls of free fall: v_z off by {dv:.1e}, pos_z by {dz:.1e}")
    assert dv <= 1e-10 and dz <= 1e-10


def test_a_standing_robot_does_not_move(eng, scen):
    moved = PR.standing(_gpu_stepper(eng), scen)
    print(f"400 calls standing on m g / 4 per leg: largest move {moved:.1e}")
    assert moved <= 1e-12


def test_the_scheme_is_first_order_in_h(eng, scen):
    r1, r2 = PR.rotation_order(_gpu_stepper(eng), scen)
    print(f"rotation error against 4096 sub-steps shrinks by {r1:.3f} (40 -> 80 steps) and {r2:.3f} (80 -> 160)")
    assert 1.7 <= r1 <= 2.4 and 1.7 <= r2 <= 2.4


def test_agrees_with_the_linear_model_at_its_linearisation_point(eng, scen):
    """omega0 = 0, any attitude, substeps 1, dt = cfg.dt, angles consistent with R: block 0 of a1mpc_horizon_states_batch with u = R f equals the plant's euler, omega and v
    within 1e-11 of the largest entry, and pos_plant - pos_linear = dt (v' - v) within the same bound"""
    n = 64
    rng = np.random.default_rng(5200)
    sc = PR.random_robots(scen, rng, n)
    h, dt = eng.horizon, sc["params"]["dt"]
    st = sc["state"].copy(); st[:, 6:9] = 0.0; st[:, 0:3] = PR.euler_of(sc["R"])
    ct = np.ones((n, 4), np.uint8)
    Rm = sc["R"].reshape(n, 3, 3)
    uw = np.einsum("bij,blj->bli", Rm, sc["grf"].reshape(n, 4, 3)).reshape(n, 12)
    u = np.concatenate([uw, np.zeros((n, 12 * (h - 1)))], 1)
    x0 = np.concatenate([st, np.full((n, 1), -9.8)], 1)
    lin = eng.horizon_states(x0, sc["R"], sc["foot"], u=u)["x_pred"][:, 0, :12]
    out = eng.plant_step(st, sc["R"], sc["foot"], sc["grf"], ct, plant=eng.plant_config(dt=dt))
    pl = out["state"]
    assert np.abs(out["R"] - sc["R"]).max() <= 2.3e-16   # (omega0 = 0: the Cayley factor is the identity, exactly; step 0 moves an orthogonal R by an ulp at most)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    figs = [rel(pl[:, 0:3], lin[:, 0:3]), rel(pl[:, 6:9], lin[:, 6:9]), rel(pl[:, 9:12], lin[:, 9:12])]
    dpos = float(np.abs((pl[:, 3:6] - lin[:, 3:6]) - dt * (pl[:, 9:12] - st[:, 9:12])).max() / np.abs(lin[:, 3:6]).max())
    print(f"plant against the linear model's first step: euler {figs[0]:.1e}, omega {figs[1]:.1e}, v {figs[2]:.1e}, pos - dt (v' - v) {dpos:.1e} (relative to the largest entry)")
    assert np.abs(lin[:, 6:9]).max() > 0.1   # (the forces do turn the body)
    assert max(figs) <= 1e-11 and dpos <= 1e-11


# ---- the closed loop on the device
def _perturbed_standing_robots(scen, nb=16, seed=5):
    rng = np.random.default_rng(seed)
    P = scen.PARAM_SETS["gazebo"]
    roll = rng.uniform(-.1, .1, nb); pit = rng.uniform(-.1, .1, nb); yaw = rng.uniform(-.5, .5, nb)
    R = scen.rot_zyx(roll, pit, yaw)
    pos = np.stack([rng.normal(0, 1, nb), rng.normal(0, 1, nb), 0.3 + rng.uniform(-.03, .03, nb)], 1)
    w = rng.normal(0, .2, (nb, 3)); v = rng.normal(0, .1, (nb, 3))
    footb = np.array(P["foot"], float)[None] + rng.uniform(-.02, .02, (nb, 4, 3)); footb[:, :, 2] = -0.3   # feet on the plane 0.3 below the nominal body
    foot = np.einsum("bij,blj->bli", R, footb).reshape(nb, 12)
    z3 = np.zeros((nb, 3))
    tick = scen.pack_tick(PR.euler_of(R.reshape(nb, 9)), pos, w, v, z3, z3, z3, np.full(nb, 0.3))
    return dict(params=dict(P, **scen.MPC_CONSTANTS), horizon=10, tick=tick, R=np.ascontiguousarray(R.reshape(nb, 9)), foot=np.ascontiguousarray(foot),
                contact=np.ones((nb, 4), np.uint8))


def test_closed_loop_solve_plant_solve_on_the_device(eng, oracle, scen):
    """16 perturbed standing robots, h = 10, cold solves: 400 x (a1mpc_solve_batch_ticks_device -> a1mpc_plant_step_batch_device in place on the tick records, R_world and
    the feet) on one stream, enqueued without a host synchronisation.  Every status solved on every tick; the robots settle (roll / pitch and omega to a tenth, the height
    error no larger); and the end state is that of the same loop run with the CPU oracle's cold solve and the restatement: pos, v, angles within 1e-4, omega within 1e-3
    (the 1e-5 N force parity accumulated in one direction over 400 ticks through dt / m and dt lever / I_xx)."""
    import torch
    sc = _perturbed_standing_robots(scen)
    n, h, ticks, dt = 16, 10, 400, sc["params"]["dt"]
    tick, R, foot, ct = _t(sc["tick"]), _t(sc["R"]), _t(sc["foot"]), _t(sc["contact"])
    grf = torch.zeros((n, 12), dtype=torch.float64, device=_dev()); iters = torch.zeros(n, dtype=torch.int32, device=_dev())
    status = torch.zeros((ticks, n), dtype=torch.int32, device=_dev())
    stream = torch.cuda.Stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    assert eng.horizon == h and eng.cfg.warm_start == 0 and eng.cfg.mass == sc["params"]["mass"]
    pc = eng.plant_config(dt=dt)
    for t in range(ticks):
        rc = eng.lib.a1mpc_solve_batch_ticks_device(eng._h, n, ptr(tick), ptr(R), ptr(foot), ptr(ct), ptr(grf), None, ptr(iters), ptr(status[t]), C.c_void_p(stream.cuda_stream))
        assert rc == 0, eng.lib.a1mpc_last_error()
        eng.plant_step_device(n, tick, 22, R, foot, grf, ct, plant=pc, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    end, Rg, sts = tick.cpu().numpy(), R.cpu().numpy(), status.cpu().numpy()
    assert (sts == 1).all(), np.unique(sts)
    assert np.array_equal(end[:, 12:], sc["tick"][:, 12:])
    tilt = lambda x: float(np.abs(x[:, 0:2]).max()); spin = lambda x: float(np.abs(x[:, 6:9]).max()); high = lambda x: float(np.abs(x[:, 5] - 0.3).max())
    print(f"closed loop, 400 ticks: |roll, pitch| {tilt(sc['tick']):.4f} -> {tilt(end):.4f}, |omega| {spin(sc['tick']):.3f} -> {spin(end):.4f}, height error "
          f"{high(sc['tick']):.4f} -> {high(end):.4f}")
    assert tilt(end) <= 0.1 * tilt(sc["tick"]) and spin(end) <= 0.1 * spin(sc["tick"]) and high(end) <= high(sc["tick"])
    # the same loop on the CPU: the oracle's cold solve and the restatement
    pr = oracle.mpc_params(h, dt, sc["params"]["mu"], sc["params"]["fz_min"], sc["params"]["fz_max"], sc["params"]["q"], sc["params"]["r"], sc["params"]["mass"],
                           sc["params"]["inertia"])
    st = oracle.default_settings()
    z3 = np.zeros((n, 3))
    x, Rc, fc = sc["tick"][:, :12].copy(), sc["R"], sc["foot"]
    for t in range(ticks):
        x0 = np.concatenate([x, np.full((n, 1), -9.8)], 1)
        xref = scen.build_reference(h, dt, x[:, 0:3], x[:, 3:6], Rc.reshape(n, 3, 3), z3, z3, z3, np.full(n, 0.3))
        o = oracle.mpc_solve_batch(pr, st, x0, xref, Rc, fc, sc["contact"])
        assert (o["status"] == 1).all()
        x, Rc, fc = PR.step(sc["params"], x, Rc, fc, o["grf"], sc["contact"], None, dt, 1)
    d = lambda a, b: float(np.abs(a - b).max())
    figs = dict(pos=d(end[:, 3:6], x[:, 3:6]), v=d(end[:, 9:12], x[:, 9:12]), angles=d(end[:, 0:3], x[:, 0:3]), omega=d(end[:, 6:9], x[:, 6:9]))
    print("GPU loop against the oracle's loop after 400 ticks:", ", ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert figs["pos"] <= 1e-4 and figs["v"] <= 1e-4 and figs["angles"] <= 1e-4 and figs["omega"] <= 1e-3
