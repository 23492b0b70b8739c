"""a1mpc_walk_step_ground_kernel compiled FOR THE HOST from the product's own source text (the walk_step_host.py pattern): the plant-step section of
csrc/a1mpc_hip.hip, which holds the ground step beside the walk step, is cut out under walk_step_host.py's preamble, and a workgroup (one wavefront) runs as 64 host
threads in lock step.  Test infrastructure: lets the CPU suite hold the shipped lane mapping, LDS images, dead-lane handling and arithmetic to tests/ground_ref.py bit
for bit (-ffp-contract=off; atan2 / asin are the host's libm, not the device library)."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import walk_step_host

_POST = r'''
extern "C" void walk_ground_run(int n, int stride, int substeps, double dt, double gravity, double mass, const double* inertia, double track, int flat_ground,
                                double ground_z, const double* state, const double* R, const double* foot, const double* grf, const double* ext, const uint8_t* contacts,
                                const double* Rz, const double* target, const double* ground, double* state_out, double* R_out, double* foot_out, double* vel_out,
                                uint8_t* touch_out) {
    WalkGroundArgs g;
    WalkArgs& w = g.w;
    PlantArgs& a = w.p;
    a.n = n; a.stride = stride; a.substeps = substeps; a.dt = dt; a.gravity = gravity; a.mass = mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = inertia[i];
    a.state = state; a.R = R; a.foot = foot; a.grf = grf; a.ext = ext; a.contacts = contacts; a.state_out = state_out; a.R_out = R_out; a.foot_out = foot_out;
    const bool track_on = track != 0.0;   // launch_walk_step_ground: without tracking the kernel gets neither pointer; with `ground` cfg's plane is not passed on
    w.track = track_on ? track : 0.0; w.ground_z = ground ? 0.0 : ground_z; w.flat_ground = ground ? 0 : flat_ground;
    w.Rz = track_on ? Rz : nullptr; w.target = track_on ? target : nullptr; w.vel_out = vel_out;
    g.ground = ground; g.touch = touch_out;
    for (int blk = 0; blk < (n + 15) / 16; ++blk) {   // one wavefront per workgroup, 16 robots each
        std::vector<std::thread> lanes;
        for (int l = 0; l < 64; ++l) lanes.emplace_back([&g, blk, l] { blockIdx.x = blk; threadIdx.x = l; a1mpc_walk_step_ground_kernel(g); });
        for (auto& t : lanes) t.join();
    }
}
'''


def section():
    s = walk_step_host.section()
    assert "a1mpc_walk_step_ground_kernel" in s, "the ground-step kernel is not beside the plant step in csrc/a1mpc_hip.hip"
    return s


def load():
    src = walk_step_host._PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_walk_step_ground_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"wg_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"wg_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


def run(params, state, R, foot, grf, contacts, Rz=None, target=None, ground=None, ext=None, dt=0.0025, substeps=1, gravity=-9.8, swing_track=1.0, flat_ground=0,
        ground_z=0.0, rows=None, in_place=False):
    """the kernel text on the n robots of `R` -> (state (rows, stride), R (rows, 9), foot (rows, 12), foot_vel_body (rows, 12), touch (rows, 4) uint8); rows > n leaves a
    poisoned tail (NaN; touch: 0xFF) the kernel must not touch, and words [12:stride) of state_out stay NaN.  in_place: state, R and foot out ARE (copies of) the inputs"""
    f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    state, R, foot, grf, ext, Rz, target, ground = f(state), f(R).reshape(-1, 9), f(foot), f(grf), f(ext), f(Rz), f(target), f(ground)
    ct = np.ascontiguousarray(contacts, dtype=np.uint8)
    n, stride = R.shape[0], state.shape[1]
    rows = n if rows is None else rows
    if in_place:
        state, R, foot = state.copy(), R.copy(), foot.copy()
        so, Ro, fo = state, R, foot
    else:
        so, Ro, fo = np.full((rows, stride), np.nan), np.full((rows, 9), np.nan), np.full((rows, 12), np.nan)
    vo = np.full((rows, 12), np.nan); to = np.full((rows, 4), 0xFF, np.uint8)
    I = f(np.asarray(params["inertia"], float).reshape(9))
    load().walk_ground_run(C.c_int(n), C.c_int(stride), C.c_int(substeps), C.c_double(dt), C.c_double(gravity), C.c_double(params["mass"]), p(I), C.c_double(swing_track),
                           C.c_int(flat_ground), C.c_double(ground_z), p(state), p(R), p(foot), p(grf), p(ext), p(ct), p(Rz), p(target), p(ground), p(so), p(Ro), p(fo),
                           p(vo), p(to))
    return so, Ro, fo, vo, to
