"""a1mpc_walk_sensors_touch_kernel compiled FOR THE HOST from the product's own source text (the walk_sensors_host.py pattern; the kernel sits in the plant-step section
of csrc/a1mpc_hip.hip beside the walk sensors, whose argument record it extends): 64 host threads in lock step are one wavefront.  Test infrastructure: holds the
shipped kernel text to tests/ground_ref.py (-ffp-contract=off; sqrt is IEEE, atan2 / acos / sin / cos are the host's libm, not the device library)."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import sensor_synthesis_host as synth_host
import walk_step_host

_POST = r'''
extern "C" void walk_touch_run(int n, int stride, double mass, const double* rho_fix, const double* rho_opt, const double* state, const double* R, const double* foot,
                               const double* grf, const double* ext, const double* vel, const uint8_t* touch, double touch_force, const uint8_t* contacts, double* quat,
                               double* acc, double* gyro, double* jpos, double* jvel, double* fforce, uint8_t* reach, double* prel, double* vrel) {
    WalkTouchArgs t;
    SynthArgs& a = t.w.s;
    a.n = n; a.stride = stride; a.mass = mass;
    for (int i = 0; i < 20; ++i) a.rho_fix[i] = rho_fix[i];
    for (int i = 0; i < 12; ++i) a.rho_opt[i] = rho_opt[i];
    a.state = state; a.R = R; a.foot = foot; a.grf = grf; a.ext = ext; a.contacts = contacts;
    a.quat = quat; a.acc = acc; a.gyro = gyro; a.jpos = jpos; a.jvel = jvel; a.fforce = fforce; a.reach = reach; a.prel = prel; a.vrel = vrel;
    t.w.vel = vel; t.touch = touch; t.touch_force = touch_force == 0.0 ? 0.0 : touch_force;   // (launch_walk_sensors_touch)
    for (int blk = 0; blk < (n + 15) / 16; ++blk) {   // one wavefront per workgroup, 16 robots each
        std::vector<std::thread> lanes;
        for (int l = 0; l < 64; ++l) lanes.emplace_back([&t, blk, l] { blockIdx.x = blk; threadIdx.x = l; a1mpc_walk_sensors_touch_kernel(t); });
        for (auto& th : lanes) th.join();
    }
}
'''
WIDTHS = synth_host.WIDTHS


def section():
    s = walk_step_host.section()
    assert "a1mpc_walk_sensors_touch_kernel" in s, "the touch-sensors kernel is not beside the plant step in csrc/a1mpc_hip.hip"
    return s


def load():
    src = walk_step_host._PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_walk_sensors_touch_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"wt_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"wt_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


def run(mass, state, R, foot, grf, contacts, foot_vel_body=None, touch=None, touch_force=0.0, ext=None, rho_fix=None, rho_opt=None, rows=None, want_foot_rel=True):
    """the kernel text on the n robots of `R` -> dict of the nine outputs of sensor_synthesis_host.run, `rows` >= n rows each, the rows beyond n NaN-poisoned (reach: 0xFF)"""
    from sensor_synthesis_ref import A1_RHO_FIX
    f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    state, R, foot, grf, ext, vel = f(state), f(R).reshape(-1, 9), f(foot), f(grf), f(ext), f(foot_vel_body)
    ct = np.ascontiguousarray(contacts, dtype=np.uint8)
    tc = None if touch is None else np.ascontiguousarray(touch, dtype=np.uint8)
    fix = f(A1_RHO_FIX if rho_fix is None else rho_fix).reshape(20); opt = f(np.zeros(12) if rho_opt is None else rho_opt).reshape(12)
    n, stride = R.shape[0], state.shape[1]
    rows = n if rows is None else rows
    out = {k: (np.full((rows, w), 0xFF, np.uint8) if k == "reach" else np.full((rows, w), np.nan)) for k, w in WIDTHS.items()}
    if not want_foot_rel:
        out["foot_pos_rel"] = out["foot_vel_rel"] = None
    load().walk_touch_run(C.c_int(n), C.c_int(stride), C.c_double(mass), p(fix), p(opt), p(state), p(R), p(foot), p(grf), p(ext), p(vel), p(tc), C.c_double(touch_force),
                          p(ct), p(out["quat"]), p(out["imu_acc_raw"]), p(out["imu_gyro_raw"]), p(out["joint_pos"]), p(out["joint_vel"]), p(out["foot_force"]),
                          p(out["reach"]), p(out["foot_pos_rel"]), p(out["foot_vel_rel"]))
    return out
