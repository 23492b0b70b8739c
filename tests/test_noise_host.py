"""Sensor noise and IMU bias on the CPU: the product's kernel text compiled for the host (tests/emu/sensor_noise_host.py: 64 host threads in lock step are one wavefront)
against the numpy restatement of tests/noise_ref.py, within the host bar; what must hold bit for bit (a repeated call, a robot alone, a split batch, the reductions, a
NaN row); the quaternion's geometry; the generator's statistics on the restatement and on the kernel text; and the noisy trot of tests/noise_loop.py on the CPU, the
yardstick of the GPU loop of tests/test_gpu_noise.py."""
import numpy as np
import pytest

import noise_loop as NL
import noise_ref as NR
import sensor_loop as SL
import sensor_noise_host as host
import walk_loop as WL
from test_walk_host import run_trot

SIZES = (1, 15, 16, 17, 65)
ROBOT0 = (0, 2 ** 32 - 65)
TICKS = (0, 7, 2 ** 33)
SEEDS = (2026, 0x9E3779B97F4A7C15)
ROWS = max(SIZES) + 3
_SHARED = {}


def _sensors():
    if "s" not in _SHARED:
        _SHARED["s"] = NR.random_sensors(ROWS)
    return _SHARED["s"]


def _split(s):
    return {k: s[k] for k in NR.SENSORS}, s["imu_bias"]


def _same(a, b, rows=slice(None)):
    (sa, ba, za), (sb, bb, zb) = a, b
    return all(NR.bits_equal(sa[k][rows], sb[k][rows]) for k in sa) and (ba is None or NR.bits_equal(ba[rows], bb[rows])) and (za is None or NR.bits_equal(za[rows], zb[rows]))


@pytest.mark.parametrize("n", SIZES)
def test_kernel_text_on_the_host_is_the_restatement(n):
    """a lone robot, either side of a wavefront edge, several workgroups with a partly filled last one; robot0 0 and 2^32 - 65 (the last index a robot may have), ticks
    0, 7 and 2^33 (the high word of the counter), both seeds (one with a high word), every channel on at levels of order one: z within the host bar, every array within
    sigma times the bar plus one ulp; rows beyond n keep their bits"""
    sens, bias = _split(_sensors())
    worst = 0.0
    for robot0 in ROBOT0:
        for tick in TICKS:
            for seed in SEEDS:
                cfg = dict(NR.LOUD, seed=seed)
                ref, rbias, rz = NR.apply(cfg, robot0, tick, {k: v[:n] for k, v in sens.items()}, bias[:n])
                out, obias, z = host.run(cfg, robot0, tick, sens, bias, n=n)
                e = float(np.abs(z - rz).max())
                print(f"n {n} robot0 {robot0} tick {tick} seed {seed:#x}: worst |z - z_ref| {e:.2e}")
                worst = max(worst, e)
                assert e <= NR.CEILING, e
                assert e <= NR.HOST_BAR, (e, NR.HOST_BAR)
                excess, figs = NR.worst_excess(dict(out, imu_bias=obias), dict(ref, imu_bias=rbias), cfg, NR.HOST_BAR, True, n)
                assert excess <= 0.0, (excess, figs)
                assert all(NR.bits_equal(out[k][n:], sens[k][n:]) for k in out) and NR.bits_equal(obias[n:], bias[n:])
                assert all(not NR.bits_equal(out[k][:n], sens[k][:n]) for k in out) and not NR.bits_equal(obias[:n], bias[:n])
    print(f"n {n}: worst |z - z_ref| {worst:.2e} (host bar {NR.HOST_BAR:.1e})")


def test_determinism_bit_for_bit():
    """a repeated call; robot g alone (robot0 = g, n = 1) against its row in the batch of 65; a batch of 165 split at 100 with robot0 offset, against the whole;
    poisoned rows beyond n stay poisoned; another tick, robot or seed gives other normals, and a robot's normals do not depend on its row"""
    sens, bias = _split(_sensors())
    cfg, tick, robot0, n = NR.LOUD, 7, 100, 65
    whole = host.run(cfg, robot0, tick, sens, bias, n=n)
    assert _same(host.run(cfg, robot0, tick, sens, bias, n=n), whole)
    for i in (0, 15, 16, 40, 64):
        one = host.run(cfg, robot0 + i, tick, {k: v[i:i + 1] for k, v in sens.items()}, bias[i:i + 1])
        assert all(NR.bits_equal(one[0][k], whole[0][k][i:i + 1]) for k in NR.SENSORS) and NR.bits_equal(one[1], whole[1][i:i + 1]) and NR.bits_equal(one[2], whole[2][i:i + 1]), i
    big, cut = _split(NR.random_sensors(165, seed=8200)), 100
    all165 = host.run(cfg, robot0, tick, *big)
    lo = host.run(cfg, robot0, tick, {k: v[:cut] for k, v in big[0].items()}, big[1][:cut])
    hi = host.run(cfg, robot0 + cut, tick, {k: v[cut:] for k, v in big[0].items()}, big[1][cut:])
    for part, rows in ((lo, slice(0, cut)), (hi, slice(cut, 165))):
        assert all(NR.bits_equal(part[0][k], all165[0][k][rows]) for k in NR.SENSORS) and NR.bits_equal(part[1], all165[1][rows]) and NR.bits_equal(part[2], all165[2][rows])
    poisoned = {k: np.where(np.arange(ROWS)[:, None] >= n, np.nan, v) for k, v in sens.items()}
    out, obias, z = host.run(cfg, robot0, tick, poisoned, np.where(np.arange(ROWS)[:, None] >= n, np.nan, bias), n=n)
    assert all(np.isnan(v[n:]).all() and not np.isnan(v[:n]).any() for v in out.values()) and np.isnan(obias[n:]).all() and z.shape == (n, 44) and not np.isnan(z).any()
    # another tick, another robot, another seed: other normals
    assert not NR.bits_equal(host.run(cfg, robot0, tick + 1, sens, bias, n=n)[2], whole[2]) and not NR.bits_equal(host.run(cfg, robot0 + 1, tick, sens, bias, n=n)[2], whole[2])
    assert not NR.bits_equal(host.run(dict(cfg, seed=2027), robot0, tick, sens, bias, n=n)[2], whole[2])
    assert NR.bits_equal(host.run(cfg, robot0 + 1, tick, sens, bias, n=n)[2][:-1], whole[2][1:])   # (robot g's normals do not depend on its row)


def test_reductions_bit_for_bit():
    """all sigmas 0 with the bias NULL leaves every array unchanged, -0 and NaN rows included; with the bias given and both walks 0 the bias keeps its bits and is still
    applied; one sigma on changes only its array; z_out is the same whatever the sigmas; a NULL array is left alone and changes nothing else"""
    s = {k: v.copy() for k, v in _sensors().items()}
    for k in NR.SENSORS:
        s[k][3] = -0.0; s[k][20] = np.nan
        s[k][21].view(np.uint64)[:] = 0x7FF8DEADBEEF0001   # (a NaN with a payload)
    sens, bias = _split(s)
    n = 65
    off = NR.config(seed=2026)
    loud = host.run(NR.LOUD, 0, 7, sens, bias, n=n)
    out, _, z = host.run(off, 0, 7, sens, None, n=n)
    assert all(NR.bits_equal(out[k], sens[k]) for k in NR.SENSORS) and NR.bits_equal(z, loud[2])
    out, obias, z = host.run(off, 0, 7, sens, bias, n=n)
    ref, _, _ = NR.apply(off, 0, 7, sens, bias)
    assert NR.bits_equal(obias, bias) and NR.bits_equal(z, loud[2])
    assert all(NR.bits_equal(out[k][:n], ref[k][:n]) for k in NR.SENSORS)   # (no normal enters: + alone, bit for bit)
    assert not NR.bits_equal(out["imu_gyro_raw"], sens["imu_gyro_raw"]) and NR.bits_equal(out["joint_pos"], sens["joint_pos"]) and NR.bits_equal(out["quat"], sens["quat"])
    owner = dict(gyro_sigma="imu_gyro_raw", acc_sigma="imu_acc_raw", att_sigma="quat", joint_pos_sigma="joint_pos", joint_vel_sigma="joint_vel", foot_force_sigma="foot_force")
    for level, key in owner.items():
        for want_z in (True, False):   # (without z_out the draws of the channels that are off are skipped)
            out, _, z = host.run(NR.config(seed=2026, **{level: NR.LOUD[level]}), 0, 7, sens, None, n=n, want_z=want_z)
            assert [k for k in NR.SENSORS if not NR.bits_equal(out[k], sens[k])] == [key], (level, want_z)
            assert NR.bits_equal(out[key], host.run(NR.LOUD, 0, 7, sens, None, n=n)[0][key]), (level, want_z)
            assert z is None or NR.bits_equal(z, loud[2])
    for level, cols in (("gyro_bias_walk", slice(0, 3)), ("acc_bias_walk", slice(3, 6))):
        out, obias, _ = host.run(NR.config(seed=2026, **{level: NR.LOUD[level]}), 0, 7, sens, bias, n=n, want_z=False)
        other = slice(3, 6) if cols.start == 0 else slice(0, 3)
        assert NR.bits_equal(obias[:n, cols], loud[1][:n, cols]) and NR.bits_equal(obias[:, other], bias[:, other])
    for key in NR.SENSORS:
        out, obias, z = host.run(NR.LOUD, 0, 7, {k: v for k, v in sens.items() if k != key}, bias, n=n)
        assert key not in out and all(NR.bits_equal(out[k], loud[0][k]) for k in out) and NR.bits_equal(obias, loud[1]) and NR.bits_equal(z, loud[2])
    _, obias, z = host.run(NR.LOUD, 0, 7, {}, bias, n=n)
    assert NR.bits_equal(obias, loud[1]) and NR.bits_equal(z, loud[2])


def test_a_nan_row_stays_with_its_robot():
    sens, bias = _split(_sensors())
    n, bad = 65, 37
    base = host.run(NR.LOUD, 0, 7, sens, bias, n=n)
    s2 = {k: v.copy() for k, v in sens.items()}; b2 = bias.copy()
    for v in s2.values():
        v[bad] = np.nan
    b2[bad] = np.nan
    out = host.run(NR.LOUD, 0, 7, s2, b2, n=n)
    keep = np.arange(ROWS) != bad
    assert all(NR.bits_equal(out[0][k][keep], base[0][k][keep]) and np.isnan(out[0][k][bad]).all() for k in NR.SENSORS)
    assert NR.bits_equal(out[1][keep], base[1][keep]) and np.isnan(out[1][bad]).all() and NR.bits_equal(out[2], base[2])


def test_the_quaternion_stays_a_unit_and_turns_by_theta():
    """the norm of q' is 1 within 2 ulp; the rotation from q to q' has the angle |theta| = att_sigma |z[12:15]| to first order (the product is with (1, theta / 2), not
    with (cos, sin): the angle is 2 atan(|theta| / 2), off by |theta|^3 / 12), and its axis, seen from the body, is theta's"""
    sens, _ = _split(_sensors())
    n = 65
    for att in (0.002, 0.05):
        cfg = NR.config(seed=2026, att_sigma=att)
        out, _, z = host.run(cfg, 0, 7, sens, None, n=n)
        q0, q1 = sens["quat"][:n], out["quat"][:n]
        ld = np.longdouble
        nrm = np.sqrt((q1.astype(ld) ** 2).sum(1))
        assert float(np.abs(nrm - 1).max()) <= 2 * np.finfo(np.float64).eps
        # q0^-1 (x) q1, w first
        w0, v0, w1, v1 = q0[:, 0], -q0[:, 1:], q1[:, 0], q1[:, 1:]
        dv = w0[:, None] * v1 + w1[:, None] * v0 + np.cross(v0, v1)
        dw = w0 * w1 - (v0 * v1).sum(1)
        theta = att * z[:, 12:15]
        mag = np.sqrt((theta * theta).sum(1))
        angle = 2.0 * np.arctan2(np.sqrt((dv * dv).sum(1)), dw)
        assert np.abs(angle - mag).max() <= (mag ** 3).max() / 12 + 1e-15, (att, np.abs(angle - mag).max())
        assert np.abs(dv / np.sqrt((dv * dv).sum(1, keepdims=True)) - theta / mag[:, None]).max() <= 1e-12


def test_statistics_of_the_generator():
    """seed 2026, tick 7, 4096 robots, on the restatement and on the kernel text: the mean and variance of all 180 224 normals, the worst per-channel mean and variance,
    the worst correlation of two channels; and the worst lag-1 autocorrelation over ticks 0 .. 1999 of 16 robots.  Each is scaled to a standard normal's size and held to
    5: they are maxima of 44 to 946 near-standard-normal statistics, and a wrong shift, a reused counter or a swapped word misses 5 by orders of magnitude.  The
    restatement's own figures: 0.46, 1.06, 2.50, 2.38, 3.70 and 3.64"""
    n = 4096
    zs = dict(restatement=NR.normals(2026, np.arange(n), 7), kernel=host.run(NR.config(seed=2026), 0, 7, {}, None, n=n)[2])
    zt = dict(restatement=np.stack([NR.normals(2026, np.arange(16), t) for t in range(2000)]),
              kernel=host.run(NR.config(seed=2026), 0, 0, {}, None, n=16, ticks=2000)[2].reshape(2000, 16, 44))
    assert float(np.abs(zs["kernel"] - zs["restatement"]).max()) <= NR.HOST_BAR and float(np.abs(zt["kernel"] - zt["restatement"]).max()) <= NR.HOST_BAR
    for who in zs:
        figs = dict(NR.statistics(zs[who]), lag1=NR.lag1(zt[who]))
        print(who + ": " + ", ".join(f"{k} {v:.2f}" for k, v in figs.items()))
        assert all(v <= 5.0 for v in figs.values()), (who, figs)
        assert np.abs(zs[who]).max() <= 8.6 and np.abs(zs[who]).max() >= 4.0
    # the mistakes the bar is there for: a counter that ignores the tick, and one that ignores the robot
    stuck = np.stack([zt["restatement"][0]] * 50)
    assert NR.lag1(stuck) > 50
    twin = zs["restatement"].copy(); twin[1::2] = twin[0::2]
    assert NR.statistics(np.concatenate([twin[:, :22], twin[:, :22]], 1))["correlation"] > 50


def test_bias_walks_over_consecutive_ticks():
    """100 ticks in one run of the kernel text on the same arrays: the bias is the running sum of walk z, in the restatement's order, bit for bit up to the z bar"""
    n, T = 17, 100
    cfg = NR.config(seed=2026, gyro_bias_walk=1e-5, acc_bias_walk=1e-4)
    _, bias, z = host.run(cfg, 0, 0, {}, np.zeros((n, 6)), n=n, ticks=T)
    z = z.reshape(T, n, 44)
    ref = np.zeros((n, 6))
    for t in range(T):
        _, ref, _ = NR.apply(cfg, 0, t, {}, ref, z=z[t])
    assert NR.bits_equal(bias, ref) and np.abs(bias).max() > 1e-5


# ---- the noisy trot
def test_noisy_trot_on_the_cpu(oracle, scen):
    """4 perturbed standing robots (seed 5), IMU window 1, the schedule of tests/walk_loop.py, NOMINAL noise (seed 2026, robot b = row b, tick = the loop's tick, the bias
    from 0) on the walk sensors: sensor_loop.conditions_hold is empty on every closed tick and the EKF's height is within HEIGHT_ESTIMATE of the plant's (both asserted
    inside run_trot); the walk's conditions hold and the heading speed is inside HEADING_SPEED; the history is not the clean loop's.  Printed, with no bar: the EKF's
    worst velocity error beside the clean run's"""
    n = 4
    sc = SL.perturbed_standing_robots(scen)
    runs = {}
    for name, cfg in (("clean", None), ("noisy", NR.NOMINAL)):
        loop = NL.NoisyWalkLoop(oracle, scen, sc, n, noise=cfg)
        hist, figs = run_trot(loop, n)
        bad, walk = WL.walk_conditions(hist, n)
        runs[name] = (hist, figs, bad, walk, loop.vel_error)
        print(f"{name} trot on the CPU: height estimate off by {figs['height_estimate']:.2e} at most, |roll, pitch| <= {figs['tilt']:.3f}, swings rise "
              f"{walk['swing_rise']:.3f} at least, heading speed {walk['heading_speed'].min():.3f} .. {walk['heading_speed'].max():.3f}, the EKF's velocity off by "
              f"{loop.vel_error:.3f} m/s at most")
    hist, figs, bad, walk, _ = runs["noisy"]
    assert not bad, bad
    assert figs["height_estimate"] <= WL.HEIGHT_ESTIMATE
    assert (walk["heading_speed"] >= WL.HEADING_SPEED[0]).all() and (walk["heading_speed"] <= WL.HEADING_SPEED[1]).all()
    assert not np.array_equal(hist["state"], runs["clean"][0]["state"])
    assert not runs["clean"][2] and np.abs(loop.bias).max() > 0
