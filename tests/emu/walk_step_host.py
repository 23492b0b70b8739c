"""a1mpc_walk_step_kernel compiled FOR THE HOST from the product's own source text (the plant_host.py pattern): the plant-step section of csrc/a1mpc_hip.hip, which holds
the walking plant's kernels beside the plant step (they use its lane helpers and LDS sizes), is cut out, the HIP keywords are defined away, and a workgroup (one
wavefront) runs as 64 host threads in lock step.  Test infrastructure: lets the CPU suite hold the shipped lane mapping, LDS images, dead-lane handling and arithmetic to
tests/walk_ref.py bit for bit (-ffp-contract=off; atan2 / asin are the host's libm, not the device library)."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import plant_host

_POST = r'''
extern "C" void walk_run(int n, int stride, int substeps, double dt, double gravity, double mass, const double* inertia, double track, int flat_ground, double ground_z,
                         const double* state, const double* R, const double* foot, const double* grf, const double* ext, const uint8_t* contacts, const double* Rz,
                         const double* target, double* state_out, double* R_out, double* foot_out, double* vel_out) {
    WalkArgs w;
    PlantArgs& a = w.p;
    a.n = n; a.stride = stride; a.substeps = substeps; a.dt = dt; a.gravity = gravity; a.mass = mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = inertia[i];
    a.state = state; a.R = R; a.foot = foot; a.grf = grf; a.ext = ext; a.contacts = contacts; a.state_out = state_out; a.R_out = R_out; a.foot_out = foot_out;
    const bool track_on = track != 0.0;   // launch_walk_step: without tracking the kernel gets neither pointer
    w.track = track_on ? track : 0.0; w.ground_z = ground_z; w.flat_ground = flat_ground; w.Rz = track_on ? Rz : nullptr; w.target = track_on ? target : nullptr;
    w.vel_out = vel_out;
    for (int blk = 0; blk < (n + 15) / 16; ++blk) {   // the launch of launch_walk_step: one wavefront per workgroup, 16 robots each
        std::vector<std::thread> lanes;
        for (int l = 0; l < 64; ++l) lanes.emplace_back([&w, blk, l] { blockIdx.x = blk; threadIdx.x = l; a1mpc_walk_step_kernel(w); });
        for (auto& t : lanes) t.join();
    }
}
'''
_PRE = plant_host._PRE + "using std::sqrt; using std::acos; using std::sin; using std::cos;\n"


def section():
    s = plant_host.section()
    assert "a1mpc_walk_step_kernel" in s, "the walk-step kernel is not beside the plant step in csrc/a1mpc_hip.hip"
    return s


def load():
    src = _PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_walk_step_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"ws_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"ws_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


def run(params, state, R, foot, grf, contacts, Rz=None, target=None, ext=None, dt=0.0025, substeps=1, gravity=-9.8, swing_track=1.0, flat_ground=0, ground_z=0.0, rows=None,
        in_place=False):
    """the kernel text on the n robots of `R` -> (state (rows, stride), R (rows, 9), foot (rows, 12), foot_vel_body (rows, 12)); rows > n leaves a NaN-poisoned tail the
    kernel must not touch, and words [12:stride) of state_out stay NaN.  in_place: state, R and foot out ARE (copies of) the inputs"""
    f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    state, R, foot, grf, ext, Rz, target = f(state), f(R).reshape(-1, 9), f(foot), f(grf), f(ext), f(Rz), f(target)
    ct = np.ascontiguousarray(contacts, dtype=np.uint8)
    n, stride = R.shape[0], state.shape[1]
    rows = n if rows is None else rows
    if in_place:
        state, R, foot = state.copy(), R.copy(), foot.copy()
        so, Ro, fo = state, R, foot
    else:
        so, Ro, fo = np.full((rows, stride), np.nan), np.full((rows, 9), np.nan), np.full((rows, 12), np.nan)
    vo = np.full((rows, 12), np.nan)
    I = f(np.asarray(params["inertia"], float).reshape(9))
    load().walk_run(C.c_int(n), C.c_int(stride), C.c_int(substeps), C.c_double(dt), C.c_double(gravity), C.c_double(params["mass"]), p(I), C.c_double(swing_track),
                    C.c_int(flat_ground), C.c_double(ground_z), p(state), p(R), p(foot), p(grf), p(ext), p(ct), p(Rz), p(target), p(so), p(Ro), p(fo), p(vo))
    return so, Ro, fo, vo
