"""a1mpc_walk_step_heightfield_kernel and a1mpc_heightfield_sample_kernel compiled FOR THE HOST from the product's own source text (the walk_step_ground_host.py
pattern): the plant-step section of csrc/a1mpc_hip.hip, which holds the height-field kernels beside the ground step, is cut out under walk_step_host.py's preamble, and
a workgroup (one wavefront) runs as 64 host threads in lock step.  Test infrastructure: lets the CPU suite hold the shipped lane mapping, LDS images, dead-lane
handling, gathers and arithmetic to tests/heightfield_ref.py bit for bit (-ffp-contract=off; atan2 / asin are the host's libm, not the device library)."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import walk_step_host

_PRE = walk_step_host._PRE
_POST = r'''
static HfField hf_field(int nx, int ny, int interp, double x0, double y0, double dx, double dy, const double* H) {   // make_hf_field: the reciprocals once, on the host
    HfField f;
    f.H = H; f.x0 = x0; f.y0 = y0; f.inv_dx = 1.0 / dx; f.inv_dy = 1.0 / dy; f.nx = nx; f.ny = ny; f.interp = interp;
    return f;
}
extern "C" void hf_step_run(int n, int stride, int substeps, double dt, double gravity, double mass, const double* inertia, double track, int nx, int ny, int interp,
                            double x0, double y0, double dx, double dy, const double* H, const double* state, const double* R, const double* foot, const double* grf,
                            const double* ext, const uint8_t* contacts, const double* Rz, const double* target, const double* origin, double* state_out, double* R_out,
                            double* foot_out, double* vel_out, uint8_t* touch_out, double* ground_out) {
    WalkHeightfieldArgs g;
    WalkArgs& w = g.w;
    PlantArgs& a = w.p;
    a.n = n; a.stride = stride; a.substeps = substeps; a.dt = dt; a.gravity = gravity; a.mass = mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = inertia[i];
    a.state = state; a.R = R; a.foot = foot; a.grf = grf; a.ext = ext; a.contacts = contacts; a.state_out = state_out; a.R_out = R_out; a.foot_out = foot_out;
    const bool track_on = track != 0.0;   // launch_heightfield_step: without tracking the kernel gets neither pointer; cfg's plane is not passed on
    w.track = track_on ? track : 0.0; w.ground_z = 0.0; w.flat_ground = 0;
    w.Rz = track_on ? Rz : nullptr; w.target = track_on ? target : nullptr; w.vel_out = vel_out;
    g.f = hf_field(nx, ny, interp, x0, y0, dx, dy, H); g.origin = origin; g.touch = touch_out; g.ground_out = ground_out;
    for (int blk = 0; blk < (n + 15) / 16; ++blk) {   // one wavefront per workgroup, 16 robots each
        std::vector<std::thread> lanes;
        for (int l = 0; l < 64; ++l) lanes.emplace_back([&g, blk, l] { blockIdx.x = blk; threadIdx.x = l; a1mpc_walk_step_heightfield_kernel(g); });
        for (auto& t : lanes) t.join();
    }
}
extern "C" void hf_sample_run(int n, int nx, int ny, int interp, double x0, double y0, double dx, double dy, const double* H, const double* xy, const double* origin,
                              double* out) {
    HfSampleArgs a;
    a.f = hf_field(nx, ny, interp, x0, y0, dx, dy, H); a.n = n; a.xy = xy; a.origin = origin; a.out = out;
    for (int blk = 0; blk < (n + 63) / 64; ++blk)   // launch_heightfield_sample: 64 points per workgroup; no lane waits for another, so they run one after another
        for (int l = 0; l < 64; ++l) { blockIdx.x = blk; threadIdx.x = l; a1mpc_heightfield_sample_kernel(a); }
}
'''


def section():
    s = walk_step_host.section()
    assert "a1mpc_walk_step_heightfield_kernel" in s and "a1mpc_heightfield_sample_kernel" in s, "the height-field kernels are not beside the plant step in csrc/a1mpc_hip.hip"
    return s


def load():
    src = _PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_heightfield_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"hf_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"hf_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


_f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
_p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)


def _field_args(field):
    """field: tests/heightfield_ref.Field -> the scalars and the heights, an array of EXACTLY nx * ny doubles"""
    H = np.array(field.H, dtype=np.float64, order="C").reshape(-1)
    assert H.nbytes == field.nx * field.ny * 8
    return (C.c_int(field.nx), C.c_int(field.ny), C.c_int(field.interp), C.c_double(field.x0), C.c_double(field.y0), C.c_double(field.dx), C.c_double(field.dy)), H


def run(params, state, R, foot, grf, contacts, Rz=None, target=None, field=None, origin=None, ext=None, dt=0.0025, substeps=1, gravity=-9.8, swing_track=1.0, rows=None,
        in_place=False, ground_out=True):
    """the kernel text on the n robots of `R` -> (state (rows, stride), R (rows, 9), foot (rows, 12), foot_vel_body (rows, 12), touch (rows, 4) uint8, ground_out (rows, 3)
    or None); rows > n leaves a poisoned tail (NaN; touch: 0xFF) the kernel must not touch, and words [12:stride) of state_out stay NaN.  in_place: state, R and foot
    out ARE (copies of) the inputs"""
    state, R, foot, grf, ext, Rz, target, origin = _f(state), _f(R).reshape(-1, 9), _f(foot), _f(grf), _f(ext), _f(Rz), _f(target), _f(origin)
    ct = np.ascontiguousarray(contacts, dtype=np.uint8)
    n, stride = R.shape[0], state.shape[1]
    rows = n if rows is None else rows
    if in_place:
        state, R, foot = state.copy(), R.copy(), foot.copy()
        so, Ro, fo = state, R, foot
    else:
        so, Ro, fo = np.full((rows, stride), np.nan), np.full((rows, 9), np.nan), np.full((rows, 12), np.nan)
    vo = np.full((rows, 12), np.nan); to = np.full((rows, 4), 0xFF, np.uint8); go = np.full((rows, 3), np.nan) if ground_out else None
    I = _f(np.asarray(params["inertia"], float).reshape(9))
    scalars, H = _field_args(field)
    load().hf_step_run(C.c_int(n), C.c_int(stride), C.c_int(substeps), C.c_double(dt), C.c_double(gravity), C.c_double(params["mass"]), _p(I), C.c_double(swing_track),
                       *scalars, _p(H), _p(state), _p(R), _p(foot), _p(grf), _p(ext), _p(ct), _p(Rz), _p(target), _p(origin), _p(so), _p(Ro), _p(fo), _p(vo), _p(to), _p(go))
    return so, Ro, fo, vo, to, go


def sample(field, xy, origin=None, rows=None):
    """the sample kernel's text on the points xy (n, 2) -> heights (rows,), poisoned (-1e300) beyond n"""
    xy, origin = _f(xy).reshape(-1, 2), _f(origin)
    n = xy.shape[0]
    out = np.full(n if rows is None else rows, -1e300)
    scalars, H = _field_args(field)
    load().hf_sample_run(C.c_int(n), *scalars, _p(H), _p(xy), _p(origin), _p(out))
    return out
