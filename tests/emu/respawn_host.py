"""a1mpc_respawn_kernel and a1mpc_respawn_rows_kernel compiled FOR THE HOST from the product's own source text (the episode_host.py pattern).  The two kernels sit in a
banner section of their own that no other emulation's span contains and use nothing of another section, so this file compiles that section alone under a shim of its
own: 64 host threads in lock step are one wavefront, a ballot is a write to a shared slot, a barrier and a read of all 64 slots.  Test infrastructure: holds the shipped
kernel text -- the ballots, the wave-uniform loops over the set's robots, the lanes over a region's words and slots, the dead lanes -- to tests/respawn_ref.py bit for
bit.  The kernel walks a table of regions; regions() below builds that table for images of the handle's blocks the way the launcher does for the handle."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import respawn_ref as RR

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_SRC = os.path.join(_ROOT, "a1-qp-mpc-controller_amd", "csrc", "a1mpc_hip.hip")
BEGIN, END = "// ---- respawn (a1mpc_respawn_reset_batch, a1mpc_respawn_batch, a1mpc_respawn_rows_device)", "// ---- what a horizon compiled in has"
OTHER_ENDS = ("thread_local std::string g_last_error;", "// ---- the launch layer's table", "// ---- what the entry points of the caller-side stages share")
LATER_BEGINS = ("// ---- N2b: contact logic", "// ---- sensor front end (a1mpc_sensor_frontend_batch)")

_PRE = r'''
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __launch_bounds__(x)
#define __forceinline__ inline
struct Dim { unsigned x; };
static thread_local Dim blockIdx, threadIdx;
struct Barrier {   // the 64 lanes of the wavefront meet here
    std::mutex m; std::condition_variable cv; int waiting = 0; unsigned long gen = 0;
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        const unsigned long g = gen;
        if (++waiting == 64) { waiting = 0; ++gen; cv.notify_all(); }
        else cv.wait(lk, [&] { return gen != g; });
    }
};
static Barrier g_wave;
static int g_vote[64];
static unsigned long long __ballot(int pred) {
    g_vote[threadIdx.x] = pred != 0; g_wave.wait();
    unsigned long long set = 0;
    for (int l = 0; l < 64; ++l) set |= static_cast<unsigned long long>(g_vote[l]) << l;
    g_wave.wait();
    return set;
}
'''
_POST = r'''
template <class K, class A> static void run_waves(K kernel, const A& a, int blocks) {   // one wavefront per workgroup
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l) lanes.emplace_back([=] {
        for (int blk = 0; blk < blocks; ++blk) { blockIdx.x = blk; threadIdx.x = l; kernel(a); g_wave.wait(); }
    });
    for (auto& th : lanes) th.join();
}
// regions: n_regions x 5 int64 (base, robot_stride, run_step, run_bytes, runs)
extern "C" void respawn_run(int n, const uint8_t* mask, double* record, int32_t* life, double* finished, uint8_t* mask_out, unsigned codes, int hold_ticks,
                            unsigned long long max_ticks, int n_regions, const int64_t* regions) {
    RespawnArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.mask = mask; a.record = record; a.life = life; a.finished = finished; a.mask_out = mask_out; a.codes = codes; a.hold_ticks = hold_ticks;
    a.max_ticks = static_cast<double>(max_ticks); a.n_regions = n_regions;
    for (int k = 0; k < n_regions; ++k) {
        const int64_t* g = regions + 5 * k;
        a.region[k] = RespawnRegion{reinterpret_cast<char*>(g[0]), g[1], g[2], static_cast<int32_t>(g[3]), static_cast<int32_t>(g[4])};
    }
    run_waves(a1mpc_respawn_kernel, a, (n + 63) / 64);
}
// rows: n_rows x 5 int64 (dst, src, row_bytes, src_rows, when); the launcher's `wide` test
extern "C" void respawn_rows_run(int n, const uint8_t* mask, int n_rows, const int64_t* rows) {
    RespawnRowsArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.n_rows = n_rows; a.mask = mask;
    for (int k = 0; k < n_rows; ++k) {
        const int64_t* g = rows + 5 * k;
        const bool wide = ((g[0] | g[1] | g[2]) & 7) == 0;
        a.row[k] = RespawnRow{reinterpret_cast<char*>(g[0]), reinterpret_cast<const char*>(g[1]), static_cast<int32_t>(g[2]), g[3] == 1 ? 1 : 0, static_cast<int32_t>(g[4]),
                              wide ? 1 : 0};
    }
    run_waves(a1mpc_respawn_rows_kernel, a, (n + 63) / 64);
}
extern "C" int respawn_limits(int which) { return which == 0 ? kRespawnRegions : (which == 1 ? kRespawnRowsMax : kRespawnWords); }
'''


def section():
    s = open(_SRC).read()
    i0 = s.index(BEGIN); i1 = s.index(END, i0)
    # the spans the other emulations compile end at OTHER_ENDS; the two that end behind this section begin behind it as well: none of them contains it
    assert s.index(OTHER_ENDS[0]) < i0 and s.index(OTHER_ENDS[1]) < i0 and i1 < s.index(LATER_BEGINS[0]) < s.index(LATER_BEGINS[1]) < s.index(OTHER_ENDS[2]), \
        "the respawn section must lie in no span another emulation compiles"
    return s[i0:i1]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = _PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), "a1mpc_respawn_host"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"rs_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"rs_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.respawn_run.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_uint, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p]; lib.respawn_run.restype = None
    lib.respawn_rows_run.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]; lib.respawn_rows_run.restype = None
    lib.respawn_limits.argtypes = [C.c_int]; lib.respawn_limits.restype = C.c_int
    _lib = lib
    return lib


def regions(images, what, geom):
    """the launcher's table (respawn_regions) for images of the handle's blocks: one run per robot for a block that is contiguous per robot, one run of one word per
    slot for a [slot][max_batch] block"""
    M, H, w = geom["max_batch"], geom["horizon"], geom["window"]
    at = lambda k: images[k].ctypes.data
    block = lambda base, nbytes: (base, nbytes, 0, nbytes, 1)
    slots = lambda base, word, runs: (base, word, word * M, word, runs)
    g = []
    if what & RR.EKF and "ekf" in images:
        g.append(block(at("ekf"), RR.EKF_STATE * 8))
    if what & RR.CONTACT and "contact" in images:
        leg = 4 * RR.LEG_WINDOW * 4 * 8
        g += [block(at("contact"), RR.CT_RECORD), block(at("contact") + M * RR.CT_RECORD, leg), slots(at("contact") + M * (RR.CT_RECORD + leg), 8, RR.TERRAIN_WINDOW)]
    if what & RR.SENSOR and "sensor_filt" in images and "sensor_cursor" in images:
        g += [slots(at("sensor_filt"), 8, RR.IMU_FILTERS * (w + 2)), slots(at("sensor_cursor"), 4, 2)]
    if what & RR.WARM:
        g += [block(at("wx"), 12 * H * 8), block(at("wy"), 20 * H * 8), block(at("rho"), 8)]
        if "carry" in images:
            g.append(block(at("carry"), RR.carry_stride(H) * 8))
    return np.array(g, dtype=np.int64).reshape(-1, 5)


def _p(v):
    return None if v is None else v.ctypes.data_as(C.c_void_p)


def reset(images, mask, what, geom, n=None):
    """the kernel text with the mask given, on COPIES of the images -> the copies"""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    n = mask.shape[0] if n is None else n
    out = {k: np.array(v) for k, v in images.items()}
    g = regions(out, what, geom)
    assert g.shape[0] <= load().respawn_limits(0)
    load().respawn_run(n, _p(mask), None, None, None, None, 0, 0, 0, g.shape[0], _p(g))
    return out


def decide(episode, life, cfg=RR.DEFAULT, finished=None, n=None, images=None, geom=None):
    """the kernel text with the rules, on copies -> (episode, life, finished or None, mask[, images]); rows beyond n are the caller's"""
    ep = np.array(episode, dtype=np.float64, order="C"); lf = np.array(life, dtype=np.int32, order="C")
    fin = None if finished is None else np.array(finished, dtype=np.float64, order="C")
    n = ep.shape[0] if n is None else n
    mask = np.full(ep.shape[0], 0xEE, dtype=np.uint8)
    out = None if images is None else {k: np.array(v) for k, v in images.items()}
    g = np.zeros((0, 5), dtype=np.int64) if images is None else regions(out, cfg["what"], geom)
    load().respawn_run(n, None, _p(ep), _p(lf), _p(fin), _p(mask), cfg["codes"], cfg["hold_ticks"], cfg["max_ticks"], g.shape[0], _p(g))
    return (ep, lf, fin, mask) if images is None else (ep, lf, fin, mask, out)


def rows(mask, table, n=None):
    """the kernel text on the arrays of `table` themselves ([(dst, src, when)], numpy arrays or views: dst is CHANGED IN PLACE, so that a test can hand in views with
    canaries around them and pointers of any alignment)"""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    n = mask.shape[0] if n is None else n
    t = []
    for dst, src, when in table:
        assert dst.flags.c_contiguous and src.flags.c_contiguous
        rb = dst[0].nbytes
        t.append((dst.ctypes.data, src.ctypes.data, rb, src.nbytes // rb, when))
    assert len(t) <= load().respawn_limits(1)
    t = np.array(t, dtype=np.int64).reshape(-1, 5)
    load().respawn_rows_run(n, _p(mask), t.shape[0], _p(t))
