"""The sensor-synthesis kernel on the CPU: the product's kernel text compiled for the host (tests/emu/sensor_synthesis_host.py: 64 host threads in lock step are one
wavefront) against the elementwise numpy restatement of tests/sensor_synthesis_ref.py -- gyro, accelerometer, foot force, foot_pos_rel and foot_vel_rel bit for bit, the
quaternion, the joint angles and the joint rates within 4 E of the restatement's 80-bit evaluation (E: the float64 noise floor of the computation on the test's own inputs,
sensor_synthesis_ref.noise_floor) -- the round trips that do not know the restatement, the table of unreachable feet, and the closed loop
sensors -> tick -> plant -> sensors on the CPU (tests/sensor_loop.py), held to the conditions the GPU loop of tests/test_gpu_sensor_synthesis.py is held to."""
import numpy as np
import pytest

import frontend_ref as FR
import sensor_loop as SL
import sensor_synthesis_host as host
import sensor_synthesis_ref as SR

SIZES = (1, 15, 16, 17, 65)
_SHARED = {}


def _cases(scen):
    """65 random robots (all four quaternion branches, all 16 contact patterns, rho_opt within +-0.01) and the restatement in float64 and 80 bits, with and without the
    wrench: computed once, never changed"""
    if not _SHARED:
        rng = np.random.default_rng(6100)
        sc = SR.random_robots(scen, rng, max(SIZES), rho_opt=rng.uniform(-0.01, 0.01, (4, 3)))
        a = (sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"])
        _SHARED["sc"] = sc
        for ext in (False, True):
            for dt in (np.float64, np.longdouble):
                r = SR.synthesise(*a, sc["ext"] if ext else None, rho_opt=sc["rho_opt"], dtype=dt)
                for v in r.values():
                    v.setflags(write=False)
                _SHARED[(ext, dt)] = r
    return _SHARED["sc"], _SHARED


def test_the_inputs_take_every_branch(scen):
    sc, refs = _cases(scen)
    br = SR.quaternion_branch(sc["R"])
    assert set(br[:16].tolist()) == {0, 1, 2, 3}, br[:16]
    tr = sc["R"][:, 0] + sc["R"][:, 4] + sc["R"][:, 8]
    turned = np.isin(np.arange(len(tr)) % 16, (1, 2, 3))
    assert (tr[turned] < -0.9).all() and np.array_equal(br[turned][:3], [0, 1, 2])   # rotations near pi about x, y, z take the three largest-diagonal branches
    assert len({tuple(c) for c in sc["contacts"]}) == 16
    assert not refs[(True, np.float64)]["reach"].any()         # reachable by construction: the feet came through the forward map
    assert np.abs(refs[(True, np.float64)]["joint_pos"] - sc["q"]).max() <= 1e-13   # and the inverse returns the angles they came from


@pytest.mark.parametrize("stride", [12, 13, 22])
@pytest.mark.parametrize("with_ext", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_text_on_the_host_equals_the_restatement(scen, n, stride, with_ext):
    """a lone robot, either side of a wavefront edge, several workgroups with a partly filled last one; the three row widths; the wrench null and given.  NaN-poisoned rows
    beyond n stay NaN"""
    sc, refs = _cases(scen)
    r64, r80 = refs[(with_ext, np.float64)], refs[(with_ext, np.longdouble)]
    state = np.concatenate([sc["state"], np.random.default_rng(stride).normal(0, 1, (max(SIZES), stride - 12))], 1)
    out = host.run(sc["mass"], state[:n], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["ext"][:n] if with_ext else None, rho_opt=sc["rho_opt"], rows=n + 3)
    figs = SR.assert_is_ref(out, r64, r80, n, (n, stride, with_ext))
    assert all((v[n:] == 0xFF).all() if k == "reach" else np.isnan(v[n:]).all() for k, v in out.items())
    assert not any(np.isnan(v[:n]).any() for k, v in out.items() if k != "reach")
    print(f"n {n} stride {stride} wrench {with_ext}: " + ", ".join(f"{k} {e:.1e} (E {E:.1e})" for k, (e, E) in figs.items()))
    if with_ext:
        assert not SR.bits_equal(refs[(False, np.float64)]["imu_acc_raw"], r64["imu_acc_raw"])


def test_optional_outputs_null_a_robot_alone_and_non_finite_inputs(scen):
    """foot_pos_rel_out / foot_vel_rel_out NULL change nothing else; robot i alone == robot i of the batch; a NaN force on a swing leg changes no bit; a NaN omega stays
    with its robot"""
    sc, refs = _cases(scen)
    n = 37
    r64, r80 = refs[(True, np.float64)], refs[(True, np.longdouble)]
    args = lambda s=slice(0, n), **kw: (sc["mass"], kw.get("state", sc["state"])[s], sc["R"][s], sc["foot"][s], kw.get("grf", sc["grf"])[s], sc["contacts"][s], sc["ext"][s])
    full = host.run(*args(), rho_opt=sc["rho_opt"])
    lean = host.run(*args(), rho_opt=sc["rho_opt"], want_foot_rel=False)
    assert lean["foot_pos_rel"] is None and lean["foot_vel_rel"] is None
    SR.assert_is_ref(lean, r64, r80, n)
    assert all(SR.bits_equal(lean[k], full[k]) for k in SR.OUTPUTS if lean[k] is not None and k != "reach") and np.array_equal(lean["reach"], full["reach"])
    for i in (0, 15, 16, 36):
        one = host.run(*args(slice(i, i + 1)), rho_opt=sc["rho_opt"])
        assert all(SR.bits_equal(one[k], full[k][i:i + 1]) for k in SR.OUTPUTS if k != "reach")
    grf = sc["grf"].copy(); swing = np.argwhere(sc["contacts"][:n] == 0)
    for i, l in swing:
        grf[i, 3 * l + (i + l) % 3] = np.nan
    nan_swing = host.run(*args(grf=grf), rho_opt=sc["rho_opt"])
    assert len(swing) > n and all(SR.bits_equal(nan_swing[k], full[k]) for k in SR.OUTPUTS if k != "reach")
    state = sc["state"].copy(); state[20, 7] = np.nan
    bad = host.run(*args(state=state), rho_opt=sc["rho_opt"])
    keep = np.arange(n) != 20
    assert all(SR.bits_equal(bad[k][keep], full[k][keep]) for k in SR.OUTPUTS if k != "reach") and np.isnan(bad["imu_gyro_raw"][20]).all()
    assert SR.bits_equal(bad["quat"][20], full["quat"][20]) and SR.bits_equal(bad["joint_pos"][20], full["joint_pos"][20])   # (omega reaches neither)


def test_round_trips_that_do_not_know_the_restatement(scen):
    """the synthesised angles through the forward map give the feet back; J(q) joint_vel is foot_vel_rel; the quaternion through Eigen's toRotationMatrix gives R back;
    R gyro is omega; -R (foot_vel_rel + gyro x p) is v on the stance legs.  Bars: 1e-13 on lengths of 0.4 m and rates of a few m/s (the float64 noise floor of these
    chains is 1e-15 .. 1e-14: see the E figures the parity test prints)"""
    sc, refs = _cases(scen)
    n = max(SIZES)
    out = host.run(sc["mass"], sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], None, rho_opt=sc["rho_opt"])
    Rm = sc["R"].reshape(n, 3, 3)
    pb = np.einsum("bji,blj->bli", Rm, sc["foot"].reshape(n, 4, 3)).reshape(n, 12)
    assert np.abs(SR.forward_feet(SR.A1_RHO_FIX, sc["rho_opt"], out["joint_pos"]) - pb).max() <= 1e-13
    assert np.abs(out["foot_pos_rel"] - pb).max() <= 1e-15
    for l in range(4):
        _, J = SR.forward_leg(SR.leg_geometry(SR.A1_RHO_FIX, sc["rho_opt"], l), [out["joint_pos"][:, 3 * l + k] for k in range(3)])
        v = np.stack([J[r] * out["joint_vel"][:, 3 * l] + J[3 + r] * out["joint_vel"][:, 3 * l + 1] + J[6 + r] * out["joint_vel"][:, 3 * l + 2] for r in range(3)], 1)
        assert np.abs(v - out["foot_vel_rel"][:, 3 * l:3 * l + 3]).max() <= 1e-13
        st = sc["contacts"][:, l] != 0
        vb = out["foot_vel_rel"][:, 3 * l:3 * l + 3] + np.cross(out["imu_gyro_raw"], out["foot_pos_rel"][:, 3 * l:3 * l + 3])
        assert np.abs(-np.einsum("bij,bj->bi", Rm, vb) - sc["state"][:, 9:12])[st].max() <= 1e-13
        assert not out["foot_vel_rel"][~st, 3 * l:3 * l + 3].any() and not out["joint_vel"][~st, 3 * l:3 * l + 3].any() and not out["foot_force"][~st, l].any()
    assert np.abs(FR.quat_to_rotation(out["quat"]) - sc["R"]).max() <= 1e-14 and np.abs(np.linalg.norm(out["quat"], axis=1) - 1.0).max() <= 1e-15
    assert np.abs(np.einsum("bij,bj->bi", Rm, out["imu_gyro_raw"]) - sc["state"][:, 6:9]).max() <= 1e-14


def test_accelerometer_is_the_specific_force_of_the_plant_step(scen):
    """R imu_acc_raw = (v' - v) / dt - g e_z of one plant step with substeps = 1 (tests/plant_ref.py), within 1e-12 max(1, |a|): the rounding of v divided by dt"""
    import plant_ref as PR
    sc, refs = _cases(scen)
    n, dt = max(SIZES), 0.0025
    P = dict(scen.PARAM_SETS["gazebo"], **scen.MPC_CONSTANTS)
    acc = refs[(True, np.float64)]["imu_acc_raw"]
    st, _, _ = PR.step(P, sc["state"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"], dt, 1)
    a = (st[:, 9:12] - sc["state"][:, 9:12]) / dt - np.array([0.0, 0.0, PR.GRAVITY])
    got = np.einsum("bij,bj->bi", sc["R"].reshape(n, 3, 3), acc)
    err = np.abs(got - a).max(axis=1) / np.maximum(1.0, np.abs(a).max(axis=1))
    print(f"R imu_acc_raw against (v' - v) / dt - g e_z: {err.max():.1e} relative to max(1, |a|)")
    assert err.max() <= 1e-12


def test_unreachable_feet_raise_their_flag_and_zero_the_joint_rates(scen):
    """sensor_synthesis_ref.unreachable_feet on leg 0 of six robots (level bodies, so foot_abs is the body-frame foot), the other legs reachable: the documented bits on
    leg 0 and none elsewhere, joint_vel of leg 0 exactly +0 although the body moves, the other legs' rates not zero, everything finite"""
    table = SR.unreachable_feet()
    n = len(table)
    rng = np.random.default_rng(6200)
    sc = SR.random_robots(scen, rng, n, rho_opt=SR.UNREACHABLE_OPT)
    R = np.tile(np.eye(3).reshape(9), (n, 1))
    foot = SR.forward_feet(SR.A1_RHO_FIX, SR.UNREACHABLE_OPT, sc["q"])
    foot[:, 0:3] = np.array([p for p, _ in table])
    ct = np.ones((n, 4), np.uint8)
    out = host.run(sc["mass"], sc["state"], R, foot, sc["grf"], ct, None, rho_opt=SR.UNREACHABLE_OPT)
    ref = SR.synthesise(sc["mass"], sc["state"], R, foot, sc["grf"], ct, None, rho_opt=SR.UNREACHABLE_OPT)
    want = np.zeros((n, 4), np.uint8); want[:, 0] = [bits for _, bits in table]
    assert np.array_equal(out["reach"], want), out["reach"][:, 0]
    assert np.array_equal(ref["reach"], want)
    assert {1, 2, 3} == set(want[:, 0].tolist())
    assert np.array_equal(out["joint_vel"][:, 0:3].view(np.uint64), np.zeros((n, 3), np.uint64))   # +0, the bits
    assert (np.abs(out["joint_vel"][:, 3:]) > 1e-6).any(axis=1).all() and (np.abs(out["foot_vel_rel"][:, 0:3]) > 1e-6).any(axis=1).all()
    assert all(np.isfinite(out[k]).all() for k in SR.OUTPUTS if k != "reach")
    assert all(SR.bits_equal(out[k], ref[k]) for k in SR.BITS) and np.abs(out["joint_pos"] - ref["joint_pos"]).max() <= 1e-14


def test_closed_loop_on_the_cpu(oracle, scen):
    """4 perturbed standing robots (sensor_loop.perturbed_standing_robots), the EKF primed with PRIME ticks of sensors from the unstepped plant -- after which the estimated
    height is within 1 mm of the plant's -- then 100 closed ticks sensors -> tick -> plant.  On every tick: every sensor finite, status 1, reach == 0, |roll|, |pitch| <= 0.2,
    the height within 0.3 +- 0.05.  The robots settle: the tilt halves, the legs stay in stance"""
    sc = SL.perturbed_standing_robots(scen)
    L = SL.OracleLoop(oracle, scen, sc, 4)
    herr = []
    for t in range(SL.PRIME):
        L.tick(step_plant=False)
        herr.append(float(np.abs(L.pos[:, 2] - L.x[:, 5]).max()))
    print(f"height estimate against the plant's over the {SL.PRIME} priming ticks: " + " ".join(f"{e:.1e}" for e in herr))
    assert herr[-1] <= 1e-3 and herr[0] > 0.1
    x0 = L.x.copy()
    for t in range(SL.TICKS):
        L.tick()
        finite = all(np.isfinite(np.asarray(v, float)).all() for v in L.sensors.values()) and np.isfinite(L.grf).all() and np.isfinite(L.x).all()
        bad = SL.conditions_hold(L.x, L.sensors["reach"], L.status, finite)
        assert not bad, (t, bad)
        assert np.abs(L.pos[:, 2] - L.x[:, 5]).max() <= 1e-3, t    # the estimate stays with the plant
    tilt = lambda x: float(np.abs(x[:, 0:2]).max()); spin = lambda x: float(np.abs(x[:, 6:9]).max())
    print(f"closed loop on the CPU, {SL.TICKS} ticks: |roll, pitch| {tilt(x0):.4f} -> {tilt(L.x):.4f}, |omega| {spin(x0):.3f} -> {spin(L.x):.3f}, height "
          f"{L.x[:, 5].min():.4f} .. {L.x[:, 5].max():.4f}, estimate off by {np.abs(L.pos[:, 2] - L.x[:, 5]).max():.1e}")
    assert tilt(L.x) < 0.5 * tilt(x0) and (L.ct == 1).all()
