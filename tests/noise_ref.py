"""a1mpc_sensor_noise_batch restated in numpy, elementwise, in the header's operation order: Philox4x32-10 on (draw, robot, tick) under the seed, two uniforms of 52 bits
per draw, Box-Muller, and the application to the six sensor arrays and the IMU bias.  Shared by tests/test_noise_host.py (the kernel text on the host),
tests/test_gpu_noise.py (the device) and tests/noise_loop.py (the noisy trot).

What is bit-comparable and what is not: the Philox words, the uniforms and every +, * and / are exact or IEEE on both sides; the normals pass through log, cos and sin,
where numpy, the host's libm and the device library may differ by ulps.  So z is compared within a bar, and an array within sigma times that bar plus one ulp of the value
(the rounding of the last sum may fall the other way).  Each bar is twice the worst |z - z_ref| measured on the first run over the cases of its test file; a measured
value above CEILING would have been a failure, not a bar (|z| <= 8.6 and a few ulps per function put the honest difference near 1e-15)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
NZ, DRAWS = 44, 22
CHANNELS = dict(gyro=slice(0, 3), acc=slice(3, 6), gyro_bias=slice(6, 9), acc_bias=slice(9, 12), att=slice(12, 15), joint_pos=slice(16, 28), joint_vel=slice(28, 40),
                foot_force=slice(40, 44))
SENSORS = ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")
WIDTHS = dict(quat=4, imu_acc_raw=3, imu_gyro_raw=3, joint_pos=12, joint_vel=12, foot_force=4, imu_bias=6, z=NZ)
LEVELS = ("gyro_sigma", "acc_sigma", "gyro_bias_walk", "acc_bias_walk", "att_sigma", "joint_pos_sigma", "joint_vel_sigma", "foot_force_sigma")
OFF = dict(seed=0, **{k: 0.0 for k in LEVELS})
# the levels of the noisy trot (tests/noise_loop.py): an IMU of the MEMS class, encoders, and 5 N on feet that carry 30 N and more
NOMINAL = dict(seed=2026, gyro_sigma=0.01, acc_sigma=0.1, gyro_bias_walk=1e-5, acc_bias_walk=1e-4, att_sigma=0.002, joint_pos_sigma=0.001, joint_vel_sigma=0.05,
               foot_force_sigma=5.0)
# levels of order one on every channel: what the comparisons against the kernel run with, so that a wrong channel cannot hide under a small sigma
LOUD = dict(seed=2026, gyro_sigma=0.3, acc_sigma=1.5, gyro_bias_walk=0.02, acc_bias_walk=0.05, att_sigma=0.05, joint_pos_sigma=0.1, joint_vel_sigma=0.7, foot_force_sigma=9.0)

CEILING = 1e-13
HOST_MEASURED = 4.440892098500626e-16     # (2^-51, at |z| of 2 to 4: one ulp) worst |z - z_ref| of the kernel text on the host (its libm) over the cases of tests/test_noise_host.py
HOST_BAR = 2 * HOST_MEASURED
DEVICE_MEASURED = 4.440892098500626e-16   # (2^-51 as well) worst |z - z_ref| of an MI355X (the device library's log / cos / sin) over the cases of tests/test_gpu_noise.py
DEVICE_BAR = 2 * DEVICE_MEASURED


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint64 arrays holding the 32-bit words of the output"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    c = [x.copy() for x in np.broadcast_arrays(*c)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK); s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # (32 x 32 bits: exact in 64)
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def _known_answers():
    """the two known answers of the issue (the generator's published test vectors)"""
    hexes = lambda x: " ".join(f"{int(v):08x}" for v in x)
    assert hexes(philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


_known_answers()


def uniforms(seed, g, tick):
    """the two uniforms of each of the 22 draws of robots g (any integer array) at `tick` -> (u1, u2), each (len(g), 22), exact"""
    g = np.asarray(g, dtype=np.uint64).reshape(-1)
    assert (g <= np.uint64(MASK)).all()
    seed, tick = int(seed), int(tick)
    j = np.arange(DRAWS, dtype=np.uint64)[None, :]
    x = philox4x32_10((j, g[:, None], tick & MASK, (tick >> 32) & MASK), (seed & MASK, (seed >> 32) & MASK))
    s6, s26 = np.uint64(6), np.uint64(26)
    k1, k2 = ((x[0] >> s6) << s26) | (x[1] >> s6), ((x[2] >> s6) << s26) | (x[3] >> s6)
    return (k1.astype(np.float64) + 0.5) * 2.0 ** -52, (k2.astype(np.float64) + 0.5) * 2.0 ** -52


def normals(seed, g, tick):
    """the 44 unit normals of robots g at `tick` -> (len(g), 44)"""
    u1, u2 = uniforms(seed, g, tick)
    r, a = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    z = np.empty((u1.shape[0], NZ))
    z[:, 0::2] = r * np.cos(a); z[:, 1::2] = r * np.sin(a)
    return z


def config(**fields):
    c = dict(OFF)
    for k, v in fields.items():
        assert k in c, k
        c[k] = v
    return c


def apply(cfg, robot0, tick, sensors, imu_bias=None, z=None):
    """the entry on copies: sensors a dict of some of SENSORS (a missing or None one is left alone), imu_bias (n, 6) or None, z the normals to use (default: normals of
    cfg's seed) -> (dict of the changed copies, the new bias or None, z)"""
    given = {k: np.array(v, dtype=np.float64) for k, v in sensors.items() if v is not None}
    n = (next(iter(given.values())) if given else imu_bias).shape[0]
    z = normals(cfg["seed"], np.arange(n, dtype=np.uint64) + np.uint64(robot0), tick) if z is None else z
    bias = None if imu_bias is None else np.array(imu_bias, dtype=np.float64)
    if bias is not None:
        if cfg["gyro_bias_walk"] != 0.0:
            bias[:, 0:3] = bias[:, 0:3] + cfg["gyro_bias_walk"] * z[:, CHANNELS["gyro_bias"]]
        if cfg["acc_bias_walk"] != 0.0:
            bias[:, 3:6] = bias[:, 3:6] + cfg["acc_bias_walk"] * z[:, CHANNELS["acc_bias"]]
    for key, sig, ch, cols in (("imu_gyro_raw", "gyro_sigma", "gyro", slice(0, 3)), ("imu_acc_raw", "acc_sigma", "acc", slice(3, 6))):
        if key in given:
            v = given[key]
            if bias is not None:
                v = v + bias[:, cols]
            if cfg[sig] != 0.0:
                v = v + cfg[sig] * z[:, CHANNELS[ch]]
            given[key] = v
    for key in ("joint_pos", "joint_vel", "foot_force"):
        if key in given and cfg[key + "_sigma"] != 0.0:
            given[key] = given[key] + cfg[key + "_sigma"] * z[:, CHANNELS[key]]
    if "quat" in given and cfg["att_sigma"] != 0.0:
        q = given["quat"]
        w, x, y, zz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        th = cfg["att_sigma"] * z[:, CHANNELS["att"]]
        dx, dy, dz = th[:, 0] * 0.5, th[:, 1] * 0.5, th[:, 2] * 0.5
        nw = ((w - x * dx) - y * dy) - zz * dz
        nx = ((x + w * dx) + y * dz) - zz * dy
        ny = ((y + w * dy) + zz * dx) - x * dz
        nz = ((zz + w * dz) + x * dy) - y * dx
        nrm = np.sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz)
        given["quat"] = np.stack([nw / nrm, nx / nrm, ny / nrm, nz / nrm], 1)
    return given, bias, z


def level_of(cfg, key, with_bias):
    """the multiple of the z bar that array `key` may be off by: its sigma; the IMU arrays with a bias carry the walk's too (the bias enters the sum with its own
    sigma z); the bias the larger of its two walks"""
    if key == "imu_bias": return max(cfg["gyro_bias_walk"], cfg["acc_bias_walk"])
    if key == "imu_gyro_raw": return cfg["gyro_sigma"] + (cfg["gyro_bias_walk"] if with_bias else 0.0)
    if key == "imu_acc_raw": return cfg["acc_sigma"] + (cfg["acc_bias_walk"] if with_bias else 0.0)
    if key == "quat": return cfg["att_sigma"]
    return cfg[key + "_sigma"]


def worst_excess(out, ref, cfg, bar, with_bias, n):
    """over the arrays of ref: max of |out - ref| - (level * bar + one ulp of the value), rows [0, n) -> (worst excess (<= 0: inside), dict of the worst |out - ref|)"""
    worst, figs = -np.inf, {}
    for k, r in ref.items():
        d = np.abs(out[k][:n] - r[:n])
        figs[k] = float(d.max())
        worst = max(worst, float((d - (level_of(cfg, k, with_bias) * bar + np.spacing(np.abs(r[:n])))).max()))
    return worst, figs


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def random_sensors(n, seed=8100):
    """n rows of plausible sensor values: unit quaternions in all sign patterns, IMU samples around gravity, joint angles and rates, foot forces with exact zeros (swing
    legs), and a bias of the walk's magnitude: computed by the caller once, never changed"""
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, (n, 4)); q = q / np.sqrt((q * q).sum(1, keepdims=True))
    ff = rng.uniform(0, 80, (n, 4)) * (rng.uniform(0, 1, (n, 4)) > 0.4)
    s = dict(quat=q, imu_acc_raw=rng.normal(0, 1, (n, 3)) + [0, 0, 9.8], imu_gyro_raw=rng.normal(0, 0.5, (n, 3)), joint_pos=rng.uniform(-1.5, 1.5, (n, 12)),
             joint_vel=rng.normal(0, 3, (n, 12)), foot_force=ff, imu_bias=rng.normal(0, 0.01, (n, 6)))
    for v in s.values():
        v.setflags(write=False)
    return s


def statistics(z):
    """z (n, 44) of one tick -> the five figures of the issue, each scaled to a standard normal's size"""
    n = z.shape[0]; N = z.size
    c = np.corrcoef(z.T)
    return dict(mean=abs(z.mean()) * np.sqrt(N), var=abs(z.var() - 1.0) * np.sqrt(N / 2), channel_mean=np.abs(z.mean(0)).max() * np.sqrt(n),
                channel_var=np.abs(z.var(0) - 1.0).max() * np.sqrt(n / 2), correlation=np.abs(c - np.eye(NZ)).max() * np.sqrt(n))


def lag1(zt):
    """zt (T, n, 44) of T consecutive ticks -> the worst lag-1 autocorrelation over the n x 44 series (against the known mean 0 and variance 1: the mean of z_t z_t+1),
    times sqrt(T - 1)"""
    T = zt.shape[0]
    return float(np.abs((zt[1:] * zt[:-1]).mean(0)).max() * np.sqrt(T - 1))
