"""a1mpc_episode_update_kernel and a1mpc_episode_reduce_kernel compiled FOR THE HOST from the product's own source text (the sensor_noise_host.py pattern).  The two
kernels sit in a banner section of their own BEHIND the span the other emulations compile, and use that span's lane helpers, so this file compiles the plant span
followed by the episode section under walk_step_host's shim: 64 host threads in lock step are one wavefront, a wave shuffle is a write to a shared slot, a barrier and a
read of the partner's slot.  Test infrastructure: holds the shipped kernel text -- the lane mapping, the LDS images, the selects, the butterfly, the dead lanes, the
level-by-level launches of the summary -- to tests/episode_ref.py bit for bit (-ffp-contract=off; there is no library function in either kernel)."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import plant_host
import walk_step_host

_POST = r'''
template <class K, class A> static void run_waves(K kernel, const A& a, int blocks) {   // one wavefront per workgroup; the next workgroup reuses the static LDS image
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l) lanes.emplace_back([=] {
        for (int blk = 0; blk < blocks; ++blk) { blockIdx.x = blk; threadIdx.x = l; kernel(a); g_wave.wait(); }
    });
    for (auto& th : lanes) th.join();
}
extern "C" void episode_update_run(int n, int stride, double min_up, double min_height, uint64_t tick, const double* state, const double* R, const double* root_pos,
                                   const double* root_lin_vel, const double* root_lin_vel_d, const double* root_pos_d_z, const double* ground, const double* grf_body,
                                   const uint8_t* contacts, const int32_t* status, const uint8_t* reach, double* episode) {
    EpisodeArgs a;   // (launch_episode_update)
    a.n = n; a.stride = stride; a.min_up = min_up; a.min_height = min_height; a.tick_p1 = static_cast<double>(tick + 1);
    a.state = state; a.R = R; a.est_pos = root_pos; a.est_vel = root_lin_vel; a.cmd = root_lin_vel_d; a.pos_d_z = root_pos_d_z; a.ground = ground;
    a.grf = grf_body; a.contacts = contacts; a.reach = reach; a.status = status; a.episode = episode;
    run_waves(a1mpc_episode_update_kernel, a, (n + 15) / 16);
}
// launch_episode_summary: ws holds the partials of every level but the last -> the number of launches
extern "C" int episode_summary_run(int n, const double* episode, double* summary_out, double* ws) {
    EpisodeReduceArgs a;
    a.in = episode; a.rows = n; a.records = 1;
    int launches = 0;
    for (;;) {
        const int64_t groups = (a.rows + 63) / 64;
        a.last = groups == 1; a.out = a.last ? summary_out : ws;
        run_waves(a1mpc_episode_reduce_kernel, a, static_cast<int>(groups));
        ++launches;
        if (a.last) return launches;
        a.in = ws; a.rows = groups; a.records = 0; ws += groups * kEpSummary;
    }
}
'''
_PRE = walk_step_host._PRE
_SRC = plant_host._SRC
BEGIN, END = "// ---- episode record and batch summary (a1mpc_episode_update_batch, a1mpc_episode_summary_batch)", "// ---- the launch layer's table"
INPUTS = ("root_pos", "root_lin_vel", "root_lin_vel_d", "root_pos_d_z", "ground", "grf_body", "contacts", "status", "reach")
_DTYPE = dict(contacts=np.uint8, reach=np.uint8, status=np.int32)


def section():
    s = open(_SRC).read()
    i0 = s.index(BEGIN); i1 = s.index(END, i0)
    assert i0 > s.index("thread_local std::string g_last_error;"), "the episode section must sit behind the span the other emulations compile"
    return s[i0:i1]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = _PRE + plant_host.section() + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_episode_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"ep_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"ep_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.episode_update_run.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint64] + [C.c_void_p] * 12
    lib.episode_update_run.restype = None
    lib.episode_summary_run.argtypes = [C.c_int] + [C.c_void_p] * 3
    lib.episode_summary_run.restype = C.c_int
    _lib = lib
    return lib


def update(episode, tick, state, R, cfg=None, n=None, **inputs):
    """the kernel text on the first n rows (default: all) of a COPY of `episode` -> the copy; inputs: some of INPUTS (a missing or None one is NULL); rows beyond n are the
    caller's: whatever they hold must come back unchanged"""
    cfg = cfg or dict(min_up=0.5, min_height=0.12)
    ep = np.array(episode, dtype=np.float64, order="C")
    n = ep.shape[0] if n is None else n
    state = np.ascontiguousarray(state, dtype=np.float64); R = np.ascontiguousarray(R, dtype=np.float64)
    arrs = [None if inputs.get(k) is None else np.ascontiguousarray(inputs[k], dtype=_DTYPE.get(k, np.float64)) for k in INPUTS]
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    load().episode_update_run(n, state.shape[1], cfg["min_up"], cfg["min_height"], int(tick), p(state), p(R), *[p(v) for v in arrs], p(ep))
    return ep


def summary(episode, n=None):
    """the kernel text, level by level, on the first n rows -> (the 20 words, the number of launches)"""
    ep = np.ascontiguousarray(episode, dtype=np.float64)
    n = ep.shape[0] if n is None else n
    out = np.full(20, np.nan)
    ws = np.full(((n + 63) // 64 + 8) * 20, np.nan)
    launches = load().episode_summary_run(n, ep.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), ws.ctypes.data_as(C.c_void_p))
    return out, launches
