"""a1mpc_sensor_noise_kernel compiled FOR THE HOST from the product's own source text (the walk_sensors_touch_host.py pattern; the kernel sits in the plant-step section of
csrc/a1mpc_hip.hip beside the sensor kernels): 64 host threads in lock step are one wavefront.  Test infrastructure: holds the shipped kernel text -- the Philox rounds,
the draw-to-lane mapping, the LDS image of the normals, the selects -- to tests/noise_ref.py (-ffp-contract=off; sqrt is IEEE, log / cos / sin are the host's libm, not the
device library).  One call runs `ticks` consecutive ticks on the same arrays (the bias walks, the sensors gather noise), z of tick k going to row block k of z_out."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import walk_step_host

_POST = r'''
extern "C" void noise_run(int n, uint64_t seed, uint64_t robot0, uint64_t tick0, int ticks, const double* levels, double* quat, double* acc, double* gyro, double* jpos,
                          double* jvel, double* fforce, double* bias, double* z_out) {
    NoiseArgs a;   // (launch_sensor_noise)
    a.n = n; a.key0 = static_cast<uint32_t>(seed); a.key1 = static_cast<uint32_t>(seed >> 32); a.robot0 = robot0;
    a.gyro_sigma = gyro ? levels[0] : 0.0; a.acc_sigma = acc ? levels[1] : 0.0; a.gyro_walk = bias ? levels[2] : 0.0; a.acc_walk = bias ? levels[3] : 0.0;
    a.att_sigma = quat ? levels[4] : 0.0; a.jpos_sigma = jpos ? levels[5] : 0.0; a.jvel_sigma = jvel ? levels[6] : 0.0; a.fforce_sigma = fforce ? levels[7] : 0.0;
    a.quat = quat; a.acc = acc; a.gyro = gyro; a.jpos = jpos; a.jvel = jvel; a.fforce = fforce; a.bias = bias;
    uint64_t zs = 0;
    const auto on = [&zs](double level, int z0, int count) { if (level != 0.0) zs |= ((uint64_t{1} << count) - 1) << z0; };
    on(a.gyro_sigma, 0, 3); on(a.acc_sigma, 3, 3); on(a.gyro_walk, 6, 3); on(a.acc_walk, 9, 3); on(a.att_sigma, 12, 3); on(a.jpos_sigma, 16, 12); on(a.jvel_sigma, 28, 12);
    on(a.fforce_sigma, 40, 4);
    a.draws = 0;
    for (int j = 0; j < kNoiseDraws; ++j)
        if (z_out || ((zs >> (2 * j)) & 3u)) a.draws |= 1u << j;
    const int blocks = (n + 15) / 16;   // one wavefront per workgroup, 16 robots each
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l) lanes.emplace_back([=] {
        NoiseArgs t = a;
        for (int k = 0; k < ticks; ++k) {
            const uint64_t tick = tick0 + static_cast<uint64_t>(k);
            t.tick_lo = static_cast<uint32_t>(tick); t.tick_hi = static_cast<uint32_t>(tick >> 32);
            t.z = z_out ? z_out + static_cast<size_t>(k) * n * kNoiseZ : nullptr;
            for (int blk = 0; blk < blocks; ++blk) {
                blockIdx.x = blk; threadIdx.x = l;
                a1mpc_sensor_noise_kernel(t);
                g_wave.wait();   // (the next workgroup reuses the static LDS image)
            }
        }
    });
    for (auto& th : lanes) th.join();
}
'''
_PRE = walk_step_host._PRE + "using std::log;\n"
LEVELS = ("gyro_sigma", "acc_sigma", "gyro_bias_walk", "acc_bias_walk", "att_sigma", "joint_pos_sigma", "joint_vel_sigma", "foot_force_sigma")
SENSORS = ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force")


def section():
    s = walk_step_host.section()
    assert "a1mpc_sensor_noise_kernel" in s, "the sensor-noise kernel is not beside the plant step in csrc/a1mpc_hip.hip"
    return s


def load():
    src = _PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_sensor_noise_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"sn_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"sn_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.noise_run.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int] + [C.c_void_p] * 9
    lib.noise_run.restype = None
    return lib


def run(cfg, robot0, tick, sensors, imu_bias=None, n=None, want_z=True, ticks=1):
    """the kernel text on the first n rows (default: all) of COPIES of the arrays of `sensors` (a dict of some of SENSORS; a missing or None one is NULL) and of imu_bias ->
    (dict of the copies, the bias copy or None, z (ticks * n, 44) or None); rows beyond n are the caller's: whatever they hold must come back unchanged"""
    out = {k: np.array(v, dtype=np.float64, order="C") for k, v in sensors.items() if v is not None and k in SENSORS}
    bias = None if imu_bias is None else np.array(imu_bias, dtype=np.float64, order="C")
    rows = (next(iter(out.values())) if out else bias).shape[0] if (out or bias is not None) else n
    n = rows if n is None else n
    z = np.full((ticks * n, 44), np.nan) if want_z else None
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    lv = np.array([cfg[k] for k in LEVELS], dtype=np.float64)
    load().noise_run(n, int(cfg["seed"]), int(robot0), int(tick), int(ticks), p(lv), *[p(out.get(k)) for k in SENSORS], p(bias), p(z))
    return out, bias, z
