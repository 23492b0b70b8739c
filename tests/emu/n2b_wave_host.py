"""a1mpc_contact_terrain_kernel and a1mpc_contacts_kernel compiled FOR THE HOST from the product's own source text, WITH the wavefront's LDS staging of the records that
tests/emu/n2b_host.py leaves out: the N2b section of csrc/a1mpc_hip.hip up to the handle's contact state is cut out, the HIP keywords are defined away, and a workgroup
(one wavefront, 64 robots) runs as 64 host threads -- __syncthreads is the barrier the lanes meet at, uint4 a 16-byte struct, the record images one static array.  Test
infrastructure: holds the staging (the coalesced 16-byte units in and out, the 400-byte image stride, the tails of a partly filled wavefront, the clamped input loads of
the dead lanes) to n2b_host.HostN2b, which steps contact_terrain_robot robot by robot on the records themselves.  One call runs `ticks` consecutive ticks on the same
state; rec, leg_ring and terrain_ring are three arrays of their own."""
import ctypes as C, os, subprocess, hashlib, tempfile
import numpy as np

import n2b_host

_SRC = n2b_host._SRC
_PRE = n2b_host._PRE + r'''
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#define __shared__ static
struct uint4 { uint32_t x, y, z, w; };
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
static void __syncthreads() { g_wave.wait(); }
'''
_POST = r'''
// mode 0: a1mpc_contact_terrain_kernel; 1: the same with recent_in (the terrain-only entry); 2: a1mpc_contacts_kernel.  Per-tick arrays are [tick][robot]...; pitch is
// (ticks + 1) x n, row 0 the pitch before the first tick (a tick that does not write the pitch leaves the row of the tick before); pk: 7 arrays n x 3 and pos_d_z n, or null
extern "C" void n2b_wave_run(int n, int ticks, int mode, double counter_per_swing, double foot_force_low, int use_terrain_adapt, void* rec, double* leg_ring,
                             double* terrain_ring, const double* gc, const uint8_t* plan, const double* ff, const double* foot, const double* z, double* pitch,
                             uint8_t* contacts, double* recent_out, double* terrain_out, const double* recent_in, const double* pk, double* pk_tick) {
    ContactArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.counter_per_swing = counter_per_swing; a.foot_force_low = foot_force_low; a.use_terrain_adapt = use_terrain_adapt;
    a.rec = reinterpret_cast<CtRecord*>(rec); a.leg_ring = leg_ring; a.terrain_ring = terrain_ring; a.stride = n; a.z_stride = 1; a.pitch_stride = 1;
    if (pk) {
        a.pk_euler = pk; a.pk_pos = pk + 3 * n; a.pk_ang_vel = pk + 6 * n; a.pk_lin_vel = pk + 9 * n; a.pk_euler_d = pk + 12 * n; a.pk_lin_vel_d = pk + 15 * n;
        a.pk_ang_vel_d = pk + 18 * n; a.pk_pos_d_z = pk + 21 * n;
    }
    const int blocks = (n + 63) / 64;   // one wavefront per workgroup, 64 robots each
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l) lanes.emplace_back([=] {
        ContactArgs t = a;
        for (int k = 0; k < ticks; ++k) {
            const size_t r = static_cast<size_t>(k) * n;
            if (l == 0 && pitch) std::memcpy(pitch + r + n, pitch + r, sizeof(double) * n);
            g_wave.wait();
            t.gait_counter = gc ? gc + r * 4 : nullptr; t.plan_contacts = plan ? plan + r * 4 : nullptr; t.foot_force = ff ? ff + r * 4 : nullptr;
            t.foot_pos_abs = foot ? foot + r * 12 : nullptr; t.root_pos_z = z ? z + r : nullptr; t.pitch_d = pitch ? pitch + r + n : nullptr;
            t.contacts = contacts ? contacts + r * 4 : nullptr; t.recent_out = recent_out ? recent_out + r * 12 : nullptr; t.terrain_out = terrain_out ? terrain_out + r : nullptr;
            t.recent_in = recent_in ? recent_in + r * 12 : nullptr; t.pk_tick = pk_tick ? pk_tick + r * 22 : nullptr;
            for (int blk = 0; blk < blocks; ++blk) {
                blockIdx.x = blk; threadIdx.x = l;
                if (mode == 2) a1mpc_contacts_kernel(t); else a1mpc_contact_terrain_kernel(t);
                g_wave.wait();   // (the next workgroup reuses the static record images)
            }
        }
    });
    for (auto& th : lanes) th.join();
}
'''
RECORD, LEG_RING, TERRAIN_WINDOW = 384, 4 * 60 * 4, 100   # bytes per record; doubles per robot; slots


def section():
    s = open(_SRC).read()
    i0 = s.index("// ---- N2b: contact logic"); i1 = s.index("// the handle's contact state: records, then the leg rings, then the terrain rings")
    assert i0 < s.index("void a1mpc_contact_terrain_kernel(") < s.index("void a1mpc_contacts_kernel(") < i1
    return s[i0:i1]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = _PRE + section() + _POST
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    d = os.path.join(tempfile.gettempdir(), f"a1mpc_n2b_wave_host_{os.getuid()}"); os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"nw_{tag}.so")
    if not os.path.exists(so):
        cpp = os.path.join(d, f"nw_{tag}.cpp"); open(cpp, "w").write(src)
        tmp = so + f".{os.getpid()}"
        # (-fno-strict-aliasing: the staging moves the records as uint4 and works on them as CtRecord, which the device compiler allows and g++ -O2 need not)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-pthread", cpp, "-o", tmp],
                       check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    return _lib


def run(mode, gc, plan, ff, foot, z, pitch0, recent_in=None, pk=None, counter_per_swing=120.0, foot_force_low=30.0, use_terrain_adapt=1, state=None):
    """the kernel text over the ticks of z (ticks, n), from empty filters (or `state`: (rec, leg_ring, terrain_ring) of an earlier call, changed in place) -> dict of
    contacts (ticks, n, 4), foot_pos_recent_contact (ticks, n, 12), terrain_angle (ticks, n), root_euler_d_pitch (ticks, n), tick (ticks, n, 22) -- None where the mode
    does not produce it -- and state.  mode: "full", "terrain" (recent_in (ticks, n, 12) given; the contact inputs are not read and may be None) or "contacts" (z gives
    the shape alone).  pk: (8, ...) the seven n x 3 arrays and pos_d_z of the tick record, stacked as (22 n,), or None"""
    f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    gc, ff, foot, z, recent_in, pk = f(gc), f(ff), f(foot), f(z), f(recent_in), f(pk)
    plan = None if plan is None else np.ascontiguousarray(plan, dtype=np.uint8)
    ticks, n = z.shape
    code = dict(full=0, terrain=1, contacts=2)[mode]
    assert (recent_in is not None) == (code == 1) and (pk is None or (code == 0 and pk.shape == (22 * n,)))
    if state is None:
        state = (np.zeros(n * RECORD, np.uint8), np.zeros(n * LEG_RING), np.zeros(TERRAIN_WINDOW * n))
    rec, leg_ring, terrain_ring = state
    assert rec.nbytes == n * RECORD and leg_ring.shape == (n * LEG_RING,) and terrain_ring.shape == (TERRAIN_WINDOW * n,)
    terrain = code != 2
    pitch = np.concatenate([f(pitch0).reshape(1, n), np.full((ticks, n), np.nan)]) if terrain else None
    ct = np.full((ticks, n, 4), 0xFF, np.uint8) if code != 1 else None
    recent = np.full((ticks, n, 12), np.nan) if code != 1 else None
    ang = np.full((ticks, n), np.nan) if terrain else None
    tick = np.full((ticks, n, 22), np.nan) if pk is not None else None
    load().n2b_wave_run(C.c_int(n), C.c_int(ticks), C.c_int(code), C.c_double(counter_per_swing), C.c_double(foot_force_low), C.c_int(use_terrain_adapt), p(rec),
                        p(leg_ring), p(terrain_ring), p(gc), p(plan), p(ff), p(foot), p(z) if terrain else None, p(pitch), p(ct), p(recent), p(ang), p(recent_in), p(pk), p(tick))
    return dict(contacts=ct, foot_pos_recent_contact=recent, terrain_angle=ang, root_euler_d_pitch=None if pitch is None else pitch[1:], tick=tick, state=state)
