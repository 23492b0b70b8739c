"""a1mpc_sensor_frontend_kernel and a1mpc_command_kernel compiled FOR THE HOST from the product's own source text (the balance_wrench_host.py pattern): the two banner
sections of csrc/a1mpc_hip.hip and the Neumaier struct the contact filters share with them are cut out, the HIP keywords are defined away, and the launches of
launch_sensor / launch_command (workgroups of 256 lanes, one lane per robot) run as two nested loops.  Test infrastructure: lets the CPU suite hold the shipped
arithmetic, its operation order, the field-major filter state and the bounds checks to the reference bit for bit (-ffp-contract=off, the same glibc as the reference's
compiled code)."""
import ctypes as C, os, re, subprocess, hashlib, tempfile
import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_SRC = os.path.join(_ROOT, "a1-qp-mpc-controller_amd", "csrc", "a1mpc_hip.hip")
_PRE = r'''
#include <cstdint>
#include <cstddef>
#include <cmath>
#define __global__
#define __device__
#define __launch_bounds__(x)
#define __forceinline__ inline
#define A1MPC_IMU_WINDOW_MAX 64
struct Dim { unsigned x; };
static Dim blockIdx, threadIdx;
using std::fabs; using std::sqrt; using std::atan2; using std::asin; using std::sin; using std::cos;
'''
_POST = r'''
extern "C" int frontend_filters() { return kImuFilters; }
extern "C" void sensor_run(int n, int window, long stride, double* filt, int32_t* cursor, const double* quat, const double* acc_raw, const double* gyro_raw, double* R_world,
                           double* R_z, double* euler, double* acc, double* gyro, double* ang_vel) {
    SensorArgs a;
    a.n = n; a.window = window; a.stride = stride; a.filt = filt; a.cursor = cursor; a.quat = quat; a.acc_raw = acc_raw; a.gyro_raw = gyro_raw;
    a.R_world = R_world; a.R_z = R_z; a.euler = euler; a.acc = acc; a.gyro = gyro; a.ang_vel = ang_vel;
    for (unsigned blk = 0; blk < (static_cast<unsigned>(n) + 255u) / 256u; ++blk)   // the grid of launch_sensor: whole workgroups, the kernel's own bounds check
        for (unsigned l = 0; l < 256u; ++l) { blockIdx.x = blk; threadIdx.x = l; a1mpc_sensor_frontend_kernel(a); }
}
extern "C" void command_run(int n, int init_ticks, const double* cfg5, double dt, const double* cmd, const uint8_t* toggle, const double* root_pos, double* body_height,
                            uint8_t* ctrl_state, double* euler_d, double* pos_d, double* kp_xy, int32_t* init_counter, double* lin_vel_d, double* ang_vel_d,
                            uint8_t* movement_mode, uint8_t* mpc_active, double* pos_d_z) {
    CommandArgs a;
    a.n = n; a.init_ticks = init_ticks; a.dt = dt; a.height_max = cfg5[0]; a.height_min = cfg5[1]; a.lock_x = cfg5[2]; a.lock_y = cfg5[3]; a.lock_speed = cfg5[4];
    a.cmd = cmd; a.toggle = toggle; a.root_pos = root_pos; a.body_height = body_height; a.ctrl_state = ctrl_state; a.euler_d = euler_d; a.pos_d = pos_d; a.kp_xy = kp_xy;
    a.init_counter = init_counter; a.lin_vel_d = lin_vel_d; a.ang_vel_d = ang_vel_d; a.movement_mode = movement_mode; a.mpc_active = mpc_active; a.pos_d_z = pos_d_z;
    for (unsigned blk = 0; blk < (static_cast<unsigned>(n) + 255u) / 256u; ++blk)   // the grid of launch_command
        for (unsigned l = 0; l < 256u; ++l) { blockIdx.x = blk; threadIdx.x = l; a1mpc_command_kernel(a); }
}
'''


def section():
    s = open(_SRC).read()
    neumaier = re.search(r"struct Neumaier \{.*?\n\};\n", s, flags=re.S).group(0)
    i0 = s.index("// ---- sensor front end (a1mpc_sensor_frontend_batch)"); i1 = s.index("// ---- what the entry points of the caller-side stages share")
    assert s.index("// ---- command stage (a1mpc_command_batch)") in range(i0, i1)
    return neumaier + s[i0:i1]


def load():
    src = _PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_frontend_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"fe_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"fe_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


_p = lambda v: v.ctypes.data_as(C.c_void_p)
_f = lambda v: np.ascontiguousarray(v, dtype=np.float64)


class HostSensor:
    """the sensor kernel's text on a filter state of `max_batch` robots (field-major, [6][window + 2][max_batch] doubles and [2][max_batch] cursors: the handle's)"""

    def __init__(self, max_batch, window=5):
        self.lib = load(); self.max_batch = max_batch; self.window = window
        self.reset()

    def reset(self):
        self.filt = np.zeros((self.lib.frontend_filters(), self.window + 2, self.max_batch)); self.cursor = np.zeros((2, self.max_batch), np.int32)

    def run(self, quat, acc_raw, gyro_raw, rows=None):
        """-> dict of the six outputs, `rows` rows each (rows > n: a NaN-poisoned tail the kernel must not touch)"""
        q = _f(quat); n = len(q); rows = n if rows is None else rows
        assert n <= self.max_batch
        acc, gyro = _f(acc_raw), _f(gyro_raw)
        out = {k: np.full((rows, w), np.nan) for k, w in (("R_world", 9), ("R_z", 9), ("root_euler", 3), ("imu_acc", 3), ("imu_ang_vel", 3), ("root_ang_vel", 3))}
        self.lib.sensor_run(C.c_int(n), C.c_int(self.window), C.c_long(self.max_batch), _p(self.filt), _p(self.cursor), _p(q), _p(acc), _p(gyro), *[_p(v) for v in out.values()])
        return out


def command(state, cmd, toggle, root_pos, dt, cfg, rows=None):
    """the command kernel's text on the n robots of `cmd`; `state` (tests/frontend_ref.initial_state) is updated in place; -> dict of the five outputs (`rows` as above)"""
    c = _f(cmd); n = len(c); rows = n if rows is None else rows
    tg = np.ascontiguousarray(toggle, dtype=np.uint8); pos = _f(root_pos)
    cfg5 = _f([cfg[k] for k in ("body_height_max", "body_height_min", "kp_linear_lock_x", "kp_linear_lock_y", "lock_speed")])
    out = dict(root_lin_vel_d=np.full((rows, 3), np.nan), root_ang_vel_d=np.full((rows, 3), np.nan), movement_mode=np.full(rows, 255, np.uint8),
               mpc_active=np.full(rows, 255, np.uint8), root_pos_d_z=np.full(rows, np.nan))
    load().command_run(C.c_int(n), C.c_int(cfg["mpc_init_ticks"]), _p(cfg5), C.c_double(dt), _p(c), _p(tg), _p(pos), _p(state["body_height"]), _p(state["ctrl_state"]),
                       _p(state["root_euler_d"]), _p(state["root_pos_d"]), _p(state["kp_linear_xy"]), _p(state["mpc_init_counter"]), *[_p(v) for v in out.values()])
    return out
