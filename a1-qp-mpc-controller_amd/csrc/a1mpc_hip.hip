// a1mpc_hip.hip -- the C ABI of include/a1mpc.h (liba1mpc.so) and the caller-side kernels (gait plan, contacts / terrain, swing legs, leg kinematics, EKF, joint torques,
// the dense-QP formation entry, the queue-order kernel).
//
// The solver's kernels live in csrc/a1mpc_kernels.hpp and are compiled as one translation unit per (horizon, pipeline): csrc/a1mpc_k_*.hip (round 6; build.py compiles the
// units in parallel).  This unit sees only the DECLARATIONS of their launch entry points (csrc/a1mpc_common.hpp), reaches them through ONE per-horizon table (ops_of), holds the
// launch layer's (kernel, device) table (set_lds_attr, resident_workgroups) and decides which way a batch goes (launch_mpc, solve_device_impl): the latency kernel (<= 256 QPs: the rows of a wave share one QP's set-up), the fused kernel (up to the resident rows: one row pair = one QP from
// inputs to outputs; also warm-started ticks of a known batch) or the split pipeline (set-up kernel -> queue-order kernel -> persistent ADMM rows that drain the queue
// longest-first); the general path (per-step feet / contact schedules) has the same three.  The QPs of a batch are independent; nothing is shared between workgroups except the
// read-only (alpha/beta) table and the queue counter, so the blockIdx -> XCD mapping is irrelevant here (no L2 reuse to localise).
//
// There is no CPU path in this file: without a HIP device every entry point fails.
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is dlopen()ed by a1mpc_sharded_create(transport = 1), never linked

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <map>
#include <new>

#include "a1mpc_common.hpp"

extern "C" const char a1mpc_build_id_[];   // a1mpc_build_id.cpp: "sources <hash> arch gfx950"

namespace a1mpc {

// the set-up kernel's cost guess (RowSolver::predict_cost) from the inputs alone, one thread per QP: the queue order of a first solve through a1mpc_solve_queue_kernel
__global__ __launch_bounds__(256) void a1mpc_predict_kernel(const KernelArgs a, int H) {
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (b >= a.n) return;
    double ev[3];
    if (a.tick) {
        const double* k = a.tick + b * 22; const double* R = a.R + b * 9;
        const double vwx = R[0] * k[15] + R[1] * k[16] + R[2] * k[17], vwy = R[3] * k[15] + R[4] * k[16] + R[5] * k[17];
        ev[0] = vwx - k[9]; ev[1] = vwy - k[10]; ev[2] = 0.0 - k[11];
    } else {
        const double* x0 = a.x0 + b * 13; const double* xr = a.xref + b * 13 * H;
        for (int i = 0; i < 3; ++i) ev[i] = xr[9 + i] - x0[9 + i];
    }
    const uint8_t* c = a.contact + b * (a.contact_stride ? 4 * H : 4);
    const bool all_stance = c[0] && c[1] && c[2] && c[3];
    const double hard = 30.0 * ev[2] + 27.0 * sqrt(ev[0] * ev[0] + ev[1] * ev[1]) + (all_stance ? 10.0 : 0.0);
    const double cc = 8.0 * hard + 400.0;
    a.cost[b] = cc > 0.0 ? (cc < 2047.0 ? static_cast<int>(cc) : 2047) : 0;
}

// K3: the next solve's queue order = this solve's QPs by decreasing cost (counting sort, one workgroup).  A batch of 1-4x the resident
// rows is otherwise finished by whichever long QP happened to start last; longest-first makes the makespan max(longest, total / rows).
// Round 6: 8 registers per wavefront and 516 B of LDS, so that the workgroup's four wavefronts per SIMD fit BESIDE a resident persistent wavefront (424 of 512 registers,
// 1 KB of a CU's LDS left at H = 10).  At 24 registers (a serial loop over the buckets on one thread) it had to wait for a CU with no persistent wavefront at all: 6 us
// behind its own batch's set-up with two batches in flight, but 0.4-0.5 ms per launch as soon as a third slot lets a batch's set-up run ahead of its turn (kernel
// trace, profiles/r06_setup_ahead.md); the build's resource gate keeps it at <= 16 (isa_check.MAX_VGPR_BESIDE_PERSISTENT).  The costs (0 .. 2047) are bucketed by 16: scheduling only
constexpr int kOrderThreads = 1024, kOrderBins = 128, kOrderShift = 4;
__global__ __launch_bounds__(kOrderThreads) void a1mpc_order_kernel(int n, const int32_t* __restrict__ cost, int32_t* __restrict__ order) {
    __shared__ int hist[kOrderBins];
    const int tid = static_cast<int>(threadIdx.x);
    if (tid < kOrderBins) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kOrderThreads) {
        const int c = cost[i] >> kOrderShift;
        atomicAdd(&hist[c < 0 ? 0 : (c > kOrderBins - 1 ? kOrderBins - 1 : c)], 1);
    }
    __syncthreads();
    // first queue position of every bucket, most expensive bucket first: an exclusive scan over the buckets in descending order -- thread t < 128 takes bucket 127 - t,
    // wave-level shuffles inside each of the two wavefronts, one word of LDS across them (a serial loop over the buckets on one thread was half of the kernel's 10 us)
    static_assert(kOrderBins == 128 && kOrderThreads >= 128, "two wavefronts scan the buckets");
    __shared__ int carry;
    int mine = 0, incl = 0;
    if (tid < kOrderBins) {
        mine = hist[kOrderBins - 1 - tid]; incl = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if ((tid & 63) >= off) incl += up;
        }
        if (tid == 63) carry = incl;   // buckets 127 .. 64 in total
    }
    __syncthreads();
    if (tid < kOrderBins) hist[kOrderBins - 1 - tid] = incl - mine + (tid >= 64 ? carry : 0);
    __syncthreads();
    for (int i = tid; i < n; i += kOrderThreads) {
        const int c = cost[i] >> kOrderShift;
        order[atomicAdd(&hist[c < 0 ? 0 : (c > kOrderBins - 1 ? kOrderBins - 1 : c)], 1)] = i;
    }
}
void launch_order_kernel(int n, const int32_t* cost, int32_t* order, hipStream_t stream) { hipLaunchKernelGGL(a1mpc_order_kernel, dim3(1), dim3(kOrderThreads), 0, stream, n, cost, order); }
void launch_predict_kernel(const KernelArgs& a, int H, hipStream_t stream) { hipLaunchKernelGGL(a1mpc_predict_kernel, dim3(static_cast<unsigned>((a.n + 255) / 256)), dim3(256), 0, stream, a, H); }


// ---- debug / verification: the dense QP data the reference's ConvexMpc holds in its public members (hessian, gradient, lb, ub --
// S/ConvexMpc.h:84-93, filled by calculate_qp_mats, S/ConvexMpc.cpp:158-245) materialised from the same inputs, per-step feet and
// contacts included.  The solver never forms these (a1mpc_solver.hpp); this kernel exists so that callers which poke the members
// (S/A1RobotControl.cpp:527-537, S/test/test_mpc.cpp:136-140) keep working and so that the implicit Hessian can be compared entry by
// entry with the reference's dense product.  One workgroup per QP; not on the hot path.
struct FormArgs {
    DeviceParams P;
    int32_t n, H, foot_stride, contact_stride;
    const double *x0, *xref, *R, *foot;
    const uint8_t* contact;
    const double* yaw_A;
    double *Pout, *gout, *lout, *uout;   // n x (12H)^2 row-major, n x 12H, n x 20H, n x 20H
};
__global__ __launch_bounds__(256) void a1mpc_form_kernel(const FormArgs a) {
    __shared__ double Bw[20 * 36], TB[20 * 36], w[20 * 12], Ii[9];
    const int64_t b = blockIdx.x;
    const int tid = static_cast<int>(threadIdx.x), H = a.H, n = 12 * H;
    const DeviceParams& P = a.P;
    const double* R = a.R + b * 9;
    const double* x0 = a.x0 + b * 13;
    const double yaw = a.yaw_A ? a.yaw_A[b] : x0[2];
    const double dt = P.dt, cy = cos(yaw), sy = sin(yaw), bv = dt / P.mass;
    if (tid == 0) {  // I_world = R I_b R', inverse by cofactors (S/ConvexMpc.cpp:136-141)
        double t9[9], Iw[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += R[i * 3 + k] * P.inertia[k * 3 + j]; t9[i * 3 + j] = s; }
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += t9[i * 3 + k] * R[j * 3 + k]; Iw[i * 3 + j] = s; }
        const double c00 = Iw[4] * Iw[8] - Iw[5] * Iw[7], c01 = Iw[5] * Iw[6] - Iw[3] * Iw[8], c02 = Iw[3] * Iw[7] - Iw[4] * Iw[6];
        const double id = 1.0 / (Iw[0] * c00 + Iw[1] * c01 + Iw[2] * c02);
        Ii[0] = c00 * id; Ii[1] = (Iw[2] * Iw[7] - Iw[1] * Iw[8]) * id; Ii[2] = (Iw[1] * Iw[5] - Iw[2] * Iw[4]) * id;
        Ii[3] = c01 * id; Ii[4] = (Iw[0] * Iw[8] - Iw[2] * Iw[6]) * id; Ii[5] = (Iw[2] * Iw[3] - Iw[0] * Iw[5]) * id;
        Ii[6] = c02 * id; Ii[7] = (Iw[1] * Iw[6] - Iw[0] * Iw[7]) * id; Ii[8] = (Iw[0] * Iw[4] - Iw[1] * Iw[3]) * id;
        // w_i = Q (A_d^{i+1} x0 - x_ref_i): roll-out with A_d = I + dt A_c (S/ConvexMpc.cpp:123-129,150)
        double xs[12];
        for (int k = 0; k < 12; ++k) xs[k] = x0[k];
        const double* xr = a.xref + b * 13 * H;
        for (int i = 0; i < H; ++i) {
            const double o0 = xs[6], o1 = xs[7], o2 = xs[8];
            xs[0] += dt * (cy * o0 + sy * o1); xs[1] += dt * (-sy * o0 + cy * o1); xs[2] += dt * o2;
            xs[3] += dt * xs[9]; xs[4] += dt * xs[10]; xs[5] += dt * xs[11];
            xs[11] += dt * x0[12];
            for (int k = 0; k < 12; ++k) w[i * 12 + k] = P.q2[k] * (xs[k] - xr[i * 13 + k]);
        }
    }
    __syncthreads();
    for (int e = tid; e < H * 12; e += 256) {  // B~w_t = dt Iw^-1 skew(r_t), T B~w_t
        const int t = e / 12, c = e % 12, leg = c / 3, comp = c % 3;
        const double* fp = a.foot + b * (a.foot_stride ? 12 * H : 12) + static_cast<int64_t>(t) * a.foot_stride + 3 * leg;
        const double rx = fp[0], ry = fp[1], rz = fp[2];
        const double k0 = comp == 0 ? 0.0 : (comp == 1 ? -rz : ry), k1 = comp == 0 ? rz : (comp == 1 ? 0.0 : -rx), k2 = comp == 0 ? -ry : (comp == 1 ? rx : 0.0);
        double bw[3];
        for (int k = 0; k < 3; ++k) bw[k] = (Ii[k * 3 + 0] * k0 + Ii[k * 3 + 1] * k1 + Ii[k * 3 + 2] * k2) * dt;
        for (int k = 0; k < 3; ++k) Bw[(t * 3 + k) * 12 + c] = bw[k];
        TB[(t * 3 + 0) * 12 + c] = cy * bw[0] + sy * bw[1]; TB[(t * 3 + 1) * 12 + c] = -sy * bw[0] + cy * bw[1]; TB[(t * 3 + 2) * 12 + c] = bw[2];
    }
    __syncthreads();
    double* Po = a.Pout + b * static_cast<int64_t>(n) * n;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e / n, j = e % n, s = i / 12, ca = i % 12, t = j / 12, cb = j % 12, m = s > t ? s : t;
        double al = 0.0;
        for (int k = m; k < H; ++k) al += static_cast<double>((k - s) * (k - t));
        const double be = H - m;
        double u = 0.0, v = 0.0;
        for (int c = 0; c < 3; ++c) { u += P.q2[c] * TB[(s * 3 + c) * 12 + ca] * TB[(t * 3 + c) * 12 + cb]; v += P.q2[6 + c] * Bw[(s * 3 + c) * 12 + ca] * Bw[(t * 3 + c) * 12 + cb]; }
        if (ca % 3 == cb % 3) { u += P.q2[3 + ca % 3] * bv * bv; v += P.q2[9 + ca % 3] * bv * bv; }
        Po[e] = al * (u * dt * dt) + be * v + (i == j ? P.r2[ca] : 0.0);
    }
    for (int j = tid; j < n; j += 256) {
        const int t = j / 12, cb = j % 12;
        double g = 0.0;
        for (int i = t; i < H; ++i) {
            const double k = (i - t) * dt;
            double lo = bv * w[i * 12 + 3 + cb % 3], hi = bv * w[i * 12 + 9 + cb % 3];
            for (int c = 0; c < 3; ++c) { lo += TB[(t * 3 + c) * 12 + cb] * w[i * 12 + c]; hi += Bw[(t * 3 + c) * 12 + cb] * w[i * 12 + 6 + c]; }
            g += k * lo + hi;
        }
        a.gout[b * n + j] = g;
    }
    for (int r = tid; r < 20 * H; r += 256) {  // S/ConvexMpc.cpp:223-245, per step
        const int t = r / 20, leg = (r % 20) / 5, row = r % 5;
        const uint8_t* cs = a.contact + b * (a.contact_stride ? 4 * H : 4) + static_cast<int64_t>(t) * a.contact_stride;
        const double cf = cs[leg] ? 1.0 : 0.0;
        double lo, hi;
        if (row == 4) { lo = P.fz_min * cf; hi = P.fz_max * cf; }
        else if (row == 0 || row == 2) { lo = 0.0; hi = kInfty; }
        else { lo = -kInfty; hi = 0.0; }
        a.lout[b * 20 * H + r] = lo; a.uout[b * 20 * H + r] = hi;
    }
}

__global__ void a1mpc_noop_kernel() {}


// ---- N2a: update_plan (S/A1RobotControl.cpp:148-202), one lane per (robot, leg) ------------------------------------------------
// Element-wise and HBM-bound: ~0.5 KB in + 0.3 KB out per robot.  The four lanes of a robot read the same robot-level words
// (one transaction) and write consecutive 24-byte segments.  No FMA contraction: the results are bit-identical to the reference's
// C++ arithmetic (and to the oracle, which is compiled the same way).
// Wave-private LDS stage for the kernels that run one lane per (robot, leg) (round 4).  A lane's results are 3-vectors at a stride of 24 bytes between lanes: stored
// straight from the registers, every store instruction touches 12 cache lines for 512 bytes of data.  The 16 robots of a wavefront own one contiguous run of
// every [robot][12] array (192 doubles), so the wave parks three such arrays at a time in 576 doubles of LDS and stores them back out with 64 consecutive doubles
// per instruction.  Pure data movement: no arithmetic, no bit changes (leg kernel 2.9 -> 5.8 TB/s at 524 288 robots).
struct WaveStage {
    double* sg;          // 576 doubles of LDS owned by this wavefront
    int lane;            // 0..63 = (robot of the wave) * 4 + leg
    int robots;          // live robots of this wavefront (16, fewer in the last one)
    int64_t first;       // first robot of this wavefront
    __device__ static void sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
    // null output pointers are skipped
    __device__ void flush3(const double (&x0)[3], const double (&x1)[3], const double (&x2)[3], double* o0, double* o1, double* o2) const {
#pragma unroll
        for (int r = 0; r < 3; ++r) { sg[3 * lane + r] = x0[r]; sg[192 + 3 * lane + r] = x1[r]; sg[384 + 3 * lane + r] = x2[r]; }
        sync();
        const int cnt = robots * 12;
        double* outs[3] = {o0, o1, o2};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (outs[t] == nullptr) continue;
            double* out = outs[t] + first * 12;
#pragma unroll
            for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cnt) out[e] = sg[192 * t + e]; }
        }
        sync();
    }
};
struct PlanArgs {
    a1mpc_gait_config g;
    int32_t n;
    const uint8_t* movement_mode;
    double* gait_counter;
    const double *gait_counter_speed, *root_lin_vel, *Rz, *Rw, *root_pos, *root_lin_vel_d;
    uint8_t* plan_contacts;
    double *rel, *abs_, *world;
};
// one (robot, leg) of update_plan: the new gait counter (also stored), the planned contact and the three foothold vectors
__device__ __forceinline__ void plan_lane(const PlanArgs& a, const int64_t b, const int leg, double& gc, double (&rel)[3], double (&ab)[3], double (&wo)[3]) {
#pragma clang fp contract(off)
    gc = a.gait_counter[b * 4 + leg];
    const double spd = a.gait_counter_speed[b * 4 + leg];
    uint8_t pc;
    if (!a.movement_mode[b]) {                                  // :150-153
        pc = 1; gc = a.g.gait_counter_reset[leg];
    } else {                                                    // :155-165
        gc = gc + spd;
        gc = fmod(gc, a.g.counter_per_gait);
        pc = gc <= a.g.counter_per_swing ? 1 : 0;
    }
    a.gait_counter[b * 4 + leg] = gc;
    a.plan_contacts[b * 4 + leg] = pc;
    const double* Rz = a.Rz + b * 9; const double* Rw = a.Rw + b * 9;
    const double* v = a.root_lin_vel + b * 3; const double* vd = a.root_lin_vel_d + b * 3; const double* pos = a.root_pos + b * 3;
    const double vrx = Rz[0] * v[0] + Rz[3] * v[1] + Rz[6] * v[2];   // :168-169  Rz' v
    const double vry = Rz[1] * v[0] + Rz[4] * v[1] + Rz[7] * v[2];
    const double k = sqrt(fabs(a.g.default_foot_pos[2]) / 9.8);       // default_foot_pos(2): linear index 2 = z of leg 0
    const double half_swing = ((a.g.counter_per_swing / spd) * a.g.control_dt) / 2.0;
    double dx = k * (vrx - vd[0]) + half_swing * vd[0];              // :175-182
    double dy = k * (vry - vd[1]) + half_swing * vd[1];
    if (dx < -a.g.foot_delta_x_limit) dx = -a.g.foot_delta_x_limit;
    if (dx > a.g.foot_delta_x_limit) dx = a.g.foot_delta_x_limit;
    if (dy < -a.g.foot_delta_y_limit) dy = -a.g.foot_delta_y_limit;
    if (dy > a.g.foot_delta_y_limit) dy = a.g.foot_delta_y_limit;
    rel[0] = a.g.default_foot_pos[3 * leg + 0] + dx; rel[1] = a.g.default_foot_pos[3 * leg + 1] + dy; rel[2] = a.g.default_foot_pos[3 * leg + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {                                    // :198-199
        ab[r] = Rw[r * 3 + 0] * rel[0] + Rw[r * 3 + 1] * rel[1] + Rw[r * 3 + 2] * rel[2];
        wo[r] = ab[r] + pos[r];
    }
}
__global__ __launch_bounds__(256) void a1mpc_plan_kernel(const PlanArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double stage[4][576];
    const int lane = static_cast<int>(threadIdx.x) & 63, wv = static_cast<int>(threadIdx.x) >> 6;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int leg = static_cast<int>(gid & 3);
    const int64_t wave_first = (static_cast<int64_t>(blockIdx.x) * 256 + wv * 64) >> 2;
    if (wave_first >= a.n) return;
    const WaveStage ws{stage[wv], lane, static_cast<int>(a.n - wave_first < 16 ? a.n - wave_first : 16), wave_first};
    double rel[3] = {0, 0, 0}, ab[3] = {0, 0, 0}, wo[3] = {0, 0, 0}, gc = 0.0;
    if (b < a.n) plan_lane(a, b, leg, gc, rel, ab, wo);
    ws.flush3(rel, ab, wo, a.rel, a.abs_, a.world);   // (the three [robot][12] outputs leave through the wave's LDS stage: WaveStage)
}

// ---- the gait-aware horizon (a1mpc_horizon_preview_batch): the contact schedule and the per-step feet that a1mpc_solve_batch_strided takes, produced from the
// state a control tick holds on the device.  One lane per (robot, leg), like the plan kernel; no LDS.  No FMA contraction: schedule and feet are bit-identical
// to the C++ they restate (update_plan's counter rule, S/A1RobotControl.cpp:156-164, run forward; the foot recurrence of S/test/test_mpc.cpp:112-115).
//   schedule  a lane runs its leg's counter forward -- c = fmod(c + speed, counter_per_gait), ticks_per_step times per horizon step, iterated like update_plan itself
//             will, so step t IS the plan_contacts of t * ticks_per_step ticks from now -- and keeps the H contact bits in one register; the four lanes of a robot
//             exchange their registers and lane `leg` stores steps leg, leg + 4, ... as whole 4-byte words (the robot's four lanes: 16 consecutive bytes per store)
//   feet      f_0 = foot_pos_abs, f_(t+1) = f_t - (v * dt): the product is rounded first, then subtracted; v = root_lin_vel_d (mode 1) or R_world * root_lin_vel_d (mode 2)
//   footholds the sibling kernel: where the lane's contact bits show a touchdown (bit t set, bit t - 1 clear, t >= 1) f_t is the leg's foot_pos_target_abs of this tick,
//             update_plan's Raibert foothold (S/A1RobotControl.cpp:166-199), and the recurrence continues from it
struct PreviewArgs {
    int32_t n, H, ticks_per_step;
    int32_t sched_mode;   // 0: contacts[] at every step (the reference's broadcast written out), 1: the gait's schedule
    int32_t foot_mode;    // 1: body-frame command as the reference's lines have it, 2: world-frame command
    double counter_per_gait, counter_per_swing, dt;
    const uint8_t *movement_mode, *contacts;
    const double *gait_counter, *gait_counter_speed, *foot_pos_abs, *Rw, *root_lin_vel_d;
    uint32_t* sched;      // n x H words (4 contact bytes each), or null
    double* foot_steps;   // n x 12H, or null
    const double* foot_target_abs;   // n x 12, this tick's Raibert footholds (a1mpc_horizon_preview_footholds_kernel), or null: the feet are the recurrence alone
};
// bit t: leg `leg` of robot b is in contact at horizon step t
__device__ __forceinline__ uint32_t preview_contact_bits(const PreviewArgs& a, int64_t b, int leg, int H) {
#pragma clang fp contract(off)
    const uint32_t all = (1u << H) - 1u;   // (H <= 20)
    const uint32_t c0 = a.contacts[b * 4 + leg] ? 1u : 0u;   // step 0: the actual contacts[] (S/A1RobotControl.cpp:271), the value the reference broadcasts
    if (a.sched_mode == 0) return c0 ? all : 0u;
    if (!a.movement_mode[b]) return c0 | (all & ~1u);   // stand: every planned contact is 1 (:150-153)
    double c = a.gait_counter[b * 4 + leg];
    const double spd = a.gait_counter_speed[b * 4 + leg];
    uint32_t m = c0;
    for (int t = 1; t < H; ++t) {
        for (int k = 0; k < a.ticks_per_step; ++k) {   // :158-159, one control tick
            c = c + spd;
            c = fmod(c, a.counter_per_gait);
        }
        m |= (c <= a.counter_per_swing ? 1u : 0u) << t;   // :160-164
    }
    return m;
}
// the four lanes of a robot exchange their registers; lane `leg` stores steps leg, leg + 4, ...  (every lane of the wavefront takes part in the exchange: no lane has left)
__device__ __forceinline__ void preview_store_sched(const PreviewArgs& a, uint32_t m, int lane, bool live, int64_t b, int leg, int H) {
    const int q0 = lane & ~3;
    const uint32_t m0 = __shfl(m, q0, 64), m1 = __shfl(m, q0 + 1, 64), m2 = __shfl(m, q0 + 2, 64), m3 = __shfl(m, q0 + 3, 64);
    if (live) {
        uint32_t* out = a.sched + b * H;
        for (int t = leg; t < H; t += 4)
            out[t] = ((m0 >> t) & 1u) | (((m1 >> t) & 1u) << 8) | (((m2 >> t) & 1u) << 16) | (((m3 >> t) & 1u) << 24);
    }
}
// the feet of one (robot, leg).  kFootholds: at a touchdown -- contact bit t set, bit t - 1 clear -- the foot is this tick's foot_pos_target_abs, the words copied, and the
// recurrence goes on from there (a second touchdown inside the horizon is the same target again)
template <bool kFootholds>
__device__ __forceinline__ void preview_feet(const PreviewArgs& a, int64_t b, int leg, int H, uint32_t m) {
#pragma clang fp contract(off)
    const double* vd = a.root_lin_vel_d + b * 3;
    double v[3] = {vd[0], vd[1], vd[2]};
    if (a.foot_mode == 2) {   // root_lin_vel_d_world = root_rot_mat * root_lin_vel_d (S/A1RobotControl.cpp:470)
        const double* R = a.Rw + b * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r) v[r] = R[r * 3 + 0] * vd[0] + R[r * 3 + 1] * vd[1] + R[r * 3 + 2] * vd[2];
    }
    const double* f0 = a.foot_pos_abs + b * 12 + 3 * leg;
    double f[3] = {f0[0], f0[1], f0[2]};
    const double st[3] = {v[0] * a.dt, v[1] * a.dt, v[2] * a.dt};   // root_lin_vel_d * dt: the same product at every step
    double T[3] = {0.0, 0.0, 0.0};
    uint32_t land = 0;   // bit t: a touchdown at step t >= 1
    if (kFootholds) {
        const double* tg = a.foot_target_abs + b * 12 + 3 * leg;   // S/A1RobotControl.cpp:198, update_plan's third output
        T[0] = tg[0]; T[1] = tg[1]; T[2] = tg[2];
        land = m & ~(m << 1) & ~1u;
    }
    double* out = a.foot_steps + b * 12 * H + 3 * leg;
    for (int t = 0; t < H; ++t) {
        if (kFootholds && ((land >> t) & 1u)) { f[0] = T[0]; f[1] = T[1]; f[2] = T[2]; }
        out[0] = f[0]; out[1] = f[1]; out[2] = f[2];
        f[0] = f[0] - st[0]; f[1] = f[1] - st[1]; f[2] = f[2] - st[2];   // S/test/test_mpc.cpp:112-115
        out += 12;
    }
}
__global__ __launch_bounds__(256) void a1mpc_horizon_preview_kernel(const PreviewArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int leg = static_cast<int>(gid & 3);
    const bool live = b < a.n;
    const int H = a.H;
    if (a.sched != nullptr) preview_store_sched(a, live ? preview_contact_bits(a, b, leg, H) : 0u, lane, live, b, leg, H);
    if (a.foot_steps != nullptr && live) preview_feet<false>(a, b, leg, H, 0u);
}
// ... with footholds (a1mpc_horizon_preview_footholds_batch, foot_steps and foot_target_abs non-null, sched_mode 1): the lane's contact bits are computed whether or
// not the schedule is an output, because the feet read them
__global__ __launch_bounds__(256) void a1mpc_horizon_preview_footholds_kernel(const PreviewArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int leg = static_cast<int>(gid & 3);
    const bool live = b < a.n;
    const int H = a.H;
    const uint32_t m = live ? preview_contact_bits(a, b, leg, H) : 0u;
    if (a.sched != nullptr) preview_store_sched(a, m, lane, live, b, leg, H);
    if (live) preview_feet<true>(a, b, leg, H, m);
}

// ---- balance PD wrench (a1mpc_balance_wrench_batch): root_acc of the reference's stance controller of type 0, S/A1RobotControl.cpp:379-391 with the euler error and its
// yaw wrap of :325-332 -- what a1mpc_balance_solve_batch takes as its first input.  One lane per robot, element-wise, HBM-bound: 27 doubles in, 6 out.  Every load of a
// robot is issued before the first operation, every store behind the last.  Plain C++ without intrinsics (the CPU suite compiles this section for the host,
// tests/emu/balance_wrench_host.py); contraction off and only IEEE add / subtract / multiply, every 3-term sum left to right: the result is the reference
// arithmetic's bit for bit, whatever the batch size.  A NaN input gives NaN in its own robot's row only (a NaN yaw error takes neither branch of the wrap).
struct WrenchArgs {
    int32_t n;
    double kp_lin[3], kd_lin[3], kp_ang[3], kd_ang[3], mass;
    const double *pos_d, *pos, *lin_vel_d, *lin_vel, *euler_d, *euler, *ang_vel_d, *ang_vel, *R;   // n x 3 each, R n x 9 row-major; *_d velocities in the body frame
    double* root_acc;                                                                              // n x 6
};
// a1mpc_balance_wrench_kp_batch: kp_linear[0:2] of every robot from kp_xy (n x 2, what the command stage switches between 0 and the lock values, S/GazeboA1ROS.cpp:172-186)
// instead of the gains' -- a kernel of its own around the same per-robot body.  The body is a macro, not an inlined function: expanded with the gains' kp_linear it is token
// for token the kernel this file had before the second one existed, and the compiler gives that kernel the code it gave it then (as an inlined template it did not:
// the same operations, scheduled otherwise).  LOAD_KP: the statement that loads the per-robot gains with the other inputs; KP_LIN(i): kp_linear[i] of robot b.
struct WrenchKpArgs { WrenchArgs w; const double* kp_xy; };
#define A1_WRENCH_ROBOT(LOAD_KP, KP_LIN)                                                                                                                                  \
    _Pragma("clang fp contract(off)")                                                                                                                                     \
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;                                                                                               \
    if (b >= a.n) return;                                                                                                                                                 \
    double pd[3], p[3], vd[3], v[3], ed[3], e[3], wd[3], w[3], R[9];                                                                                                      \
    LOAD_KP                                                                                                                                                               \
    _Pragma("unroll")                                                                                                                                                     \
    for (int i = 0; i < 3; ++i) {                                                                                                                                         \
        pd[i] = a.pos_d[b * 3 + i]; p[i] = a.pos[b * 3 + i]; vd[i] = a.lin_vel_d[b * 3 + i]; v[i] = a.lin_vel[b * 3 + i];                                                 \
        ed[i] = a.euler_d[b * 3 + i]; e[i] = a.euler[b * 3 + i]; wd[i] = a.ang_vel_d[b * 3 + i]; w[i] = a.ang_vel[b * 3 + i];                                             \
    }                                                                                                                                                                     \
    _Pragma("unroll")                                                                                                                                                     \
    for (int k = 0; k < 9; ++k) R[k] = a.R[b * 9 + k];                                                                                                                    \
    double ee[3], t2[3], acc[6];                                                                                                                                          \
    _Pragma("unroll")                                                                                                                                                     \
    for (int i = 0; i < 3; ++i) ee[i] = ed[i] - e[i];                                                                                                                     \
    if (ee[2] > 3.1415926 * 1.5) ee[2] = ed[2] - 3.1415926 * 2 - e[2];                              /* :328-332 (strict comparisons: a yaw error ON the mark is kept) */  \
    else if (ee[2] < -3.1415926 * 1.5) ee[2] = ed[2] + 3.1415926 * 2 - e[2];                                                                                              \
    _Pragma("unroll")                                                                                                                                                     \
    for (int i = 0; i < 3; ++i) {                                                                                                                                         \
        const double t = vd[i] - (R[0 * 3 + i] * v[0] + R[1 * 3 + i] * v[1] + R[2 * 3 + i] * v[2]);   /* root_lin_vel_d - R' root_lin_vel */                              \
        t2[i] = a.kd_lin[i] * t;                                                                                                                                          \
    }                                                                                                                                                                     \
    _Pragma("unroll")                                                                                                                                                     \
    for (int i = 0; i < 3; ++i) {                                                                                                                                         \
        acc[i] = KP_LIN(i) * (pd[i] - p[i]);                                                         /* :380 */                                                           \
        acc[i] = acc[i] + (R[i * 3 + 0] * t2[0] + R[i * 3 + 1] * t2[1] + R[i * 3 + 2] * t2[2]);       /* :382-383 */                                                      \
        acc[3 + i] = a.kp_ang[i] * ee[i];                                                            /* :385 */                                                           \
        acc[3 + i] = acc[3 + i] + a.kd_ang[i] * (wd[i] - (R[0 * 3 + i] * w[0] + R[1 * 3 + i] * w[1] + R[2 * 3 + i] * w[2]));   /* :386-387 */                             \
    }                                                                                                                                                                     \
    acc[2] = acc[2] + a.mass * 9.8;                                                                  /* :391 */                                                           \
    _Pragma("unroll")                                                                                                                                                     \
    for (int k = 0; k < 6; ++k) a.root_acc[b * 6 + k] = acc[k];
#define A1_WRENCH_NO_LOAD
#define A1_WRENCH_GAINS_KP(i) a.kp_lin[i]
#define A1_WRENCH_LOAD_ROW_KP const double kp_row[3] = {k.kp_xy[b * 2 + 0], k.kp_xy[b * 2 + 1], a.kp_lin[2]};
#define A1_WRENCH_ROW_KP(i) kp_row[i]
__global__ __launch_bounds__(256) void a1mpc_balance_wrench_kernel(const WrenchArgs a) {
    A1_WRENCH_ROBOT(A1_WRENCH_NO_LOAD, A1_WRENCH_GAINS_KP)
}
__global__ __launch_bounds__(256) void a1mpc_balance_wrench_kp_kernel(const WrenchKpArgs k) {
    const WrenchArgs& a = k.w;
    { A1_WRENCH_ROBOT(A1_WRENCH_LOAD_ROW_KP, A1_WRENCH_ROW_KP) }   // (a block of its own: the contraction pragma must open a compound statement)
}
#undef A1_WRENCH_ROBOT
#undef A1_WRENCH_NO_LOAD
#undef A1_WRENCH_GAINS_KP
#undef A1_WRENCH_LOAD_ROW_KP
#undef A1_WRENCH_ROW_KP

// ---- predicted horizon states and the cost of a force plan (a1mpc_horizon_states_batch): x_(t+1) = A_d x_t + B_d,t u_t rolled out from x0, i.e. A_qp x0 + B_qp u of the
// reference's public members (S/ConvexMpc.h, S/ConvexMpc.cpp:181-202) without forming either, and the two sums 1/2 e'Qe, 1/2 u'Ru.  Memory-bound: 25H + 34 doubles in,
// 13H + 2 out per QP.
//   lanes     one wavefront = one workgroup = 16 consecutive QPs, lane = 4 * (QP of the wave) + l.  Lane l holds leg l's foot and force (the cross product needs no
//             exchange) and owns state triple l: 0 rpy, 1 pos, 2 omega, 3 v.  The pair sums over legs {0,1} / {2,3} are one exchange with lane ^ 1; the second step is
//             folded into the exchange with lane ^ 2 that also hands the old omega, v to lanes 0, 1: lanes 0 / 1 send their pair's torque / force, lanes 2 / 3 their old
//             state -- every x_t is read before any x_(t+1) is written.  Sum order: (leg 0 + leg 1) + (leg 2 + leg 3).  Plain wave shuffles (64-bit DPP has row_newbcast only).
//   memory    the wave's QPs own ONE contiguous run of u_full, x_ref, the per-step feet and x_pred.  The run is visited kHsChunk steps at a time: the chunk of every array
//             goes through wave-private LDS, 64 consecutive doubles of the chunk per instruction, so that global memory sees pieces of 12 (13) * kHsChunk consecutive
//             doubles per QP (384 / 416 B) instead of one 24-byte triple per lane at a stride of 96H bytes.  x_pred takes x_ref's place in LDS (a lane reads its three
//             reference words, then writes its three state words over them).  Rows of 52 doubles: the 8 QPs of a half wave start 40 banks apart (mod 64), the reads of a
//             component are conflict-free.  3 * 16 * 52 doubles = 19 968 B per wave: eight waves per CU.
//   bits      contraction off, fma() where a product feeds a sum: the results do not depend on where the compiler places the code, nor on the number of QPs in the call.
//   dead lanes (QPs >= n of the last wave) read the wave's first QP, take part in every shuffle and store nothing, neither to LDS nor to memory.  Of the X rows they read
//             their OWN row, not the first QP's: that QP's lanes write their states over it, and only the wave's lock step would order the two.  A dead lane's row is
//             UNINITIALISED LDS (hs_load / hs_store touch the live rows alone, nothing ever writes it): the read is meant, and its value is discarded with the lane's cost.
struct HorizonStatesArgs {
    int32_t n, H, foot_stride;
    double dt, mass, inertia[9], q[12], r[12];
    const double *x0, *tick, *xref, *R, *foot, *yaw_A, *u;   // x0 (n x 13) or tick (n x 22); xref, yaw_A, u may be null
    double *x_pred, *cost;                                   // n x 13H, n x 2; either may be null
};
constexpr int kHsChunk = 4, kHsRow = 52, kHsBuf = 16 * kHsRow;
static_assert(kHsRow >= 13 * kHsChunk && (2 * kHsRow) % 64 == 40, "a chunk of x_ref fits a row; rows start 40 banks apart");
// (QP of the wave, offset in its piece) of element e of a chunk whose pieces are cw doubles: e / cw without an integer division (e < 832, cw >= 12: the quotient is
// never closer than 0.009 to an integer, the float product is off by < 1e-5)
__device__ __forceinline__ int hs_row(int e, float inv_cw) { return static_cast<int>((static_cast<float>(e) + 0.5f) * inv_cw); }
// the chunk [t0, t0 + c) of the wave's run of a [QP][H][W] array -> LDS rows (or back): 64 consecutive doubles of the chunk per instruction, all loads issued before the
// first LDS write.  Only the `live` QPs of the wave are touched: every address lies inside the n x H x W array
template <int W>
__device__ __forceinline__ void hs_load(double* buf, const double* g, int64_t first, int live, int H, int t0, int c, int lane) {
    constexpr int kMax = (16 * kHsChunk * W + 63) / 64;
    const int cw = c * W, cnt = live * cw;
    const float inv = 1.0f / static_cast<float>(cw);
    const double* base = g + (first * H + t0) * W;
    double v[kMax];
#pragma unroll
    for (int m = 0; m < kMax; ++m) {
        const int e = lane + 64 * m, q = hs_row(e, inv);
        v[m] = base[e < cnt ? static_cast<int64_t>(q) * H * W + (e - q * cw) : 0];   // (past the chunk: the chunk's first word again, no branch around the load)
    }
#pragma unroll
    for (int m = 0; m < kMax; ++m) {
        const int e = lane + 64 * m, q = hs_row(e, inv);
        if (e < cnt) buf[q * kHsRow + (e - q * cw)] = v[m];
    }
}
template <int W>
__device__ __forceinline__ void hs_store(const double* buf, double* g, int64_t first, int live, int H, int t0, int c, int lane) {
    constexpr int kMax = (16 * kHsChunk * W + 63) / 64;
    const int cw = c * W, cnt = live * cw;
    const float inv = 1.0f / static_cast<float>(cw);
    double* base = g + (first * H + t0) * W;
#pragma unroll
    for (int m = 0; m < kMax; ++m) {
        const int e = lane + 64 * m, q = hs_row(e, inv);
        if (e < cnt) base[static_cast<int64_t>(q) * H * W + (e - q * cw)] = buf[q * kHsRow + (e - q * cw)];
    }
}
__device__ __forceinline__ double hs_pick(int l, double a0, double a1, double a2, double a3) { return l == 0 ? a0 : (l == 1 ? a1 : (l == 2 ? a2 : a3)); }
__global__ __launch_bounds__(64) void a1mpc_horizon_states_kernel(const HorizonStatesArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double lds[3 * kHsBuf];
    double* const U = lds; double* const F = lds + kHsBuf; double* const X = lds + 2 * kHsBuf;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, H = a.H;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int row = (alive ? qw : 0) * kHsRow;
    const int64_t b = first + (alive ? qw : 0);
    // once per QP: the state triple, yaw, Iw^-1, dt / m (the arithmetic of a1mpc_form_kernel)
    const double* xs = a.tick ? a.tick + b * 22 : a.x0 + b * 13;
    double x[3] = {xs[3 * l], xs[3 * l + 1], xs[3 * l + 2]};
    const double grav = a.tick ? -9.8 : xs[12];
    const double yaw = a.yaw_A ? a.yaw_A[b] : xs[2];
    const double dt = a.dt, cy = cos(yaw), sy = sin(yaw), bv = dt / a.mass;
    const double* R = a.R + b * 9;
    double Ii[9];
    {   // I_world = R I_b R', inverse by cofactors (S/ConvexMpc.cpp:136-141)
        double Rm[9], t9[9], Iw[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rm[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) t9[i * 3 + j] = fma(Rm[i * 3 + 2], a.inertia[6 + j], fma(Rm[i * 3 + 1], a.inertia[3 + j], Rm[i * 3] * a.inertia[j]));
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Iw[i * 3 + j] = fma(t9[i * 3 + 2], Rm[j * 3 + 2], fma(t9[i * 3 + 1], Rm[j * 3 + 1], t9[i * 3] * Rm[j * 3]));
        const double c00 = fma(Iw[4], Iw[8], -(Iw[5] * Iw[7])), c01 = fma(Iw[5], Iw[6], -(Iw[3] * Iw[8])), c02 = fma(Iw[3], Iw[7], -(Iw[4] * Iw[6]));
        const double id = 1.0 / fma(Iw[2], c02, fma(Iw[1], c01, Iw[0] * c00));
        Ii[0] = c00 * id; Ii[1] = fma(Iw[2], Iw[7], -(Iw[1] * Iw[8])) * id; Ii[2] = fma(Iw[1], Iw[5], -(Iw[2] * Iw[4])) * id;
        Ii[3] = c01 * id; Ii[4] = fma(Iw[0], Iw[8], -(Iw[2] * Iw[6])) * id; Ii[5] = fma(Iw[2], Iw[3], -(Iw[0] * Iw[5])) * id;
        Ii[6] = c02 * id; Ii[7] = fma(Iw[1], Iw[6], -(Iw[0] * Iw[7])) * id; Ii[8] = fma(Iw[0], Iw[4], -(Iw[1] * Iw[3])) * id;
    }
    // the lane's 3 x 3 block of [A_d - I | B_d] and what it multiplies: rpy <- (dt T) omega, pos <- (dt I) v, omega <- (dt Iw^-1) sum r x f, v <- (dt / m I) sum f  (+ dt g)
    double M[9];
    {
        const double dc = cy * dt, ds = sy * dt;   // A_d = I + A_c dt (S/ConvexMpc.cpp:150)
        const double dI = l == 1 ? dt : bv;
        M[0] = hs_pick(l, dc, dI, Ii[0] * dt, dI);  M[1] = hs_pick(l, ds, 0.0, Ii[1] * dt, 0.0); M[2] = hs_pick(l, 0.0, 0.0, Ii[2] * dt, 0.0);
        M[3] = hs_pick(l, -ds, 0.0, Ii[3] * dt, 0.0); M[4] = hs_pick(l, dc, dI, Ii[4] * dt, dI); M[5] = hs_pick(l, 0.0, 0.0, Ii[5] * dt, 0.0);
        M[6] = hs_pick(l, 0.0, 0.0, Ii[6] * dt, 0.0); M[7] = hs_pick(l, 0.0, 0.0, Ii[7] * dt, 0.0); M[8] = hs_pick(l, dt, dI, Ii[8] * dt, dI);
    }
    const double gz = l == 3 ? dt * grav : 0.0;   // A_d(11, 12) = dt (S/ConvexMpc.cpp:129)
    const double qk[3] = {hs_pick(l, a.q[0], a.q[3], a.q[6], a.q[9]), hs_pick(l, a.q[1], a.q[4], a.q[7], a.q[10]), hs_pick(l, a.q[2], a.q[5], a.q[8], a.q[11])};
    const double rk[3] = {hs_pick(l, a.r[0], a.r[3], a.r[6], a.r[9]), hs_pick(l, a.r[1], a.r[4], a.r[7], a.r[10]), hs_pick(l, a.r[2], a.r[5], a.r[8], a.r[11])};
    const bool want_cost = a.cost != nullptr;
    // tick record: x_ref_t = base + (slope dt)(t + 1), the set-up's expressions (RowSolver::setup; S/A1RobotControl.cpp:470-488)
    double xb[3] = {0.0, 0.0, 0.0}, xsl[3] = {0.0, 0.0, 0.0};
    if (a.tick && want_cost) {
        const double* k = xs;
        const double vwx = R[0] * k[15] + R[1] * k[16] + R[2] * k[17], vwy = R[3] * k[15] + R[4] * k[16] + R[5] * k[17];
        xb[0] = hs_pick(l, k[12], k[3], k[18], vwx); xb[1] = hs_pick(l, k[13], k[4], k[19], vwy); xb[2] = hs_pick(l, k[2], k[21], k[20], 0.0);
        xsl[0] = l == 1 ? vwx * dt : 0.0; xsl[1] = l == 1 ? vwy * dt : 0.0; xsl[2] = l == 0 ? k[20] * dt : 0.0;
    }
    double r0[3] = {0.0, 0.0, 0.0};
    if (a.foot_stride == 0) { const double* fp = a.foot + b * 12 + 3 * l; r0[0] = fp[0]; r0[1] = fp[1]; r0[2] = fp[2]; }
    double cx = 0.0, cu = 0.0;
    for (int t0 = 0; t0 < H; t0 += kHsChunk) {
        const int c = H - t0 < kHsChunk ? H - t0 : kHsChunk;
        if (a.u) hs_load<12>(U, a.u, first, live, H, t0, c, lane);
        if (a.foot_stride) hs_load<12>(F, a.foot, first, live, H, t0, c, lane);
        if (a.xref && want_cost) hs_load<13>(X, a.xref, first, live, H, t0, c, lane);
        WaveStage::sync();
        for (int tt = 0; tt < c; ++tt) {
            double f[3] = {0.0, 0.0, 0.0}, r[3] = {r0[0], r0[1], r0[2]};
            if (a.u) { const double* p = U + row + tt * 12 + 3 * l; f[0] = p[0]; f[1] = p[1]; f[2] = p[2]; }
            if (a.foot_stride) { const double* p = F + row + tt * 12 + 3 * l; r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; }
            // this leg's r x f and f, summed with the pair's other leg; lanes 0 / 1 then send the pair's torque / force, lanes 2 / 3 their old state
            double snd[3], w[3];
            {
                const double tq[3] = {fma(r[1], f[2], -(r[2] * f[1])), fma(r[2], f[0], -(r[0] * f[2])), fma(r[0], f[1], -(r[1] * f[0]))};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double pt = tq[k] + __shfl_xor(tq[k], 1, 64), pf = f[k] + __shfl_xor(f[k], 1, 64);
                    snd[k] = (l & 1) ? pf : pt;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double got = __shfl_xor(l >= 2 ? x[k] : snd[k], 2, 64);
                w[k] = l >= 2 ? got + snd[k] : got;   // lanes 2 / 3: (leg 0 + leg 1) + (leg 2 + leg 3)
            }
            double* xo = X + qw * kHsRow + tt * 13 + 3 * l;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double xn = fma(M[3 * k + 2], w[2], fma(M[3 * k + 1], w[1], fma(M[3 * k], w[0], x[k])));
                if (k == 2) xn = xn + gz;
                if (want_cost) {
                    const double xr = a.tick ? xb[k] + xsl[k] * static_cast<double>(t0 + tt + 1) : xo[k];
                    const double e = xn - xr;
                    cx = fma(qk[k] * e, e, cx);
                    cu = fma(rk[k] * f[k], f[k], cu);
                }
                x[k] = xn;
            }
            if (alive) {
                xo[0] = x[0]; xo[1] = x[1]; xo[2] = x[2];
                if (l == 0) xo[12] = grav;
            }
        }
        WaveStage::sync();
        if (a.x_pred) hs_store<13>(X, a.x_pred, first, live, H, t0, c, lane);
        WaveStage::sync();
    }
    if (want_cost) {
        cx = cx + __shfl_xor(cx, 1, 64); cx = cx + __shfl_xor(cx, 2, 64);
        cu = cu + __shfl_xor(cu, 1, 64); cu = cu + __shfl_xor(cu, 2, 64);
        if (alive && l == 0) { a.cost[b * 2] = cx; a.cost[b * 2 + 1] = cu; }
    }
}

// ---- single-rigid-body plant step (a1mpc_plant_step_batch): one control period of the nonlinear body under the forces of a solve -- semi-implicit Euler for the
// translation, the Cayley map for the attitude (R brought back to orthogonal to first order at the start of a call), omega from the conserved world angular momentum
// and the NEW attitude; the scheme is stated in include/a1mpc.h.
// Memory- and launch-bound: 12 + 9 + 12 + 12 (+ 6) doubles and 4 bytes in, 12 + 9 + 12 doubles out per robot.
//   lanes     the layout of a1mpc_horizon_states_kernel: one wavefront = one workgroup = 16 consecutive robots, lane = 4 * (robot of the wave) + l.  Lane l holds leg l's
//             lever, force and contact byte (rotation, cross product and foot update need no exchange); the body state is carried by all four lanes of a robot.  The
//             leg sums are x + shfl(lane ^ 1), then + shfl(lane ^ 2): (leg 0 + leg 1) + (leg 2 + leg 3) in every lane, IEEE addition being commutative.
//   memory    the wave's robots own one contiguous run of every array.  Feet and forces are a lane's own 24 bytes of a 1536-byte run: read and written directly.  The
//             state rows (12, 13 or 22 doubles), R and the wrench are shared by a robot's lanes: they pass through wave-private LDS in their memory layout, 64
//             consecutive doubles per instruction.  Every global load is issued before the first operation; outputs may be the inputs (a wave loads all it reads before
//             it stores, and no two waves share a robot).  Words [12, stride) of a state row are not stored.
//   bits      contraction off and no fma: IEEE +, -, *, / alone, three-term sums left to right -- a pure function of the robot's own inputs, restated elementwise in
//             tests/plant_ref.py.  The three inverse trigonometric calls at the end feed nothing.
//   dead lanes (robots >= n of the last wave) load the wave's first robot, take part in every shuffle and store nothing, neither to LDS nor to memory.
struct PlantArgs {
    int32_t n, stride, substeps;
    double dt, gravity, mass, inertia[9];
    const double *state, *R, *foot, *grf, *ext;   // ext may be null
    const uint8_t* contacts;
    double *state_out, *R_out, *foot_out;
};
constexpr int kPlState = 16 * 22, kPlR = 16 * 9, kPlExt = 16 * 6;
__device__ __forceinline__ double pl_pick(int l, double a0, double a1, double a2, double a3) { return l == 0 ? a0 : (l == 1 ? a1 : (l == 2 ? a2 : a3)); }
__device__ __forceinline__ double pl_legs(double x) { const double p = x + __shfl_xor(x, 1, 64); return p + __shfl_xor(p, 2, 64); }
// y = M x and y = M^T x of a row-major 3 x 3, each sum left to right
#define A1_PL_MV(y, M, x) do { _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_) y[i_] = (M[3 * i_] * x[0] + M[3 * i_ + 1] * x[1]) + M[3 * i_ + 2] * x[2]; } while (0)
#define A1_PL_MTV(y, M, x) do { _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_) y[i_] = (M[i_] * x[0] + M[3 + i_] * x[1]) + M[6 + i_] * x[2]; } while (0)
__global__ __launch_bounds__(64) void a1mpc_plant_step_kernel(const PlantArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double plds[kPlState + kPlR + kPlExt];
    double* const S = plds; double* const RL = plds + kPlState; double* const E = plds + kPlState + kPlR;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    // every load, then the LDS writes: element e of the wave's run of an array sits at e in LDS.  Past the run: the run's first word again, no branch around the load
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R;
    double vs[6], vr[3], ve[2];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
    double r[3], f[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0;
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
    WaveStage::sync();
    double pos[3], w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0}, te[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pos[k] = x[3 + k]; w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { fe[k] = E[q * 6 + k]; te[k] = E[q * 6 + 3 + k]; }
    }
    // once: R <- R - R (R^T R - I) / 2, the first-order step to the nearest orthogonal matrix (the rounding of earlier calls' products does not pile up in R^T R,
    // through which L is rebuilt below); I_b^-1 by cofactors; L = R (I_b (R^T omega)); h = dt / substeps
    {
        double E[9], Rp[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[3 * i + j] = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
        E[0] = E[0] - 1.0; E[4] = E[4] - 1.0; E[8] = E[8] - 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rp[3 * i + j] = R[3 * i + j] - 0.5 * ((R[3 * i] * E[j] + R[3 * i + 1] * E[3 + j]) + R[3 * i + 2] * E[6 + j]);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rp[k];
    }
    double Ii[9], L[3];
    {
        const double* I = a.inertia;
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        Ii[0] = c00 * id; Ii[1] = (I[2] * I[7] - I[1] * I[8]) * id; Ii[2] = (I[1] * I[5] - I[2] * I[4]) * id;
        Ii[3] = c01 * id; Ii[4] = (I[0] * I[8] - I[2] * I[6]) * id; Ii[5] = (I[2] * I[3] - I[0] * I[5]) * id;
        Ii[6] = c02 * id; Ii[7] = (I[1] * I[6] - I[0] * I[7]) * id; Ii[8] = (I[0] * I[4] - I[1] * I[3]) * id;
        double wb[3], Iw[3];
        A1_PL_MTV(wb, R, w); A1_PL_MV(Iw, I, wb); A1_PL_MV(L, R, Iw);
    }
    const double h = a.dt / static_cast<double>(a.substeps), half = h / 2.0, m = a.mass, g = a.gravity;
    for (int step = 0; step < a.substeps; ++step) {
        // 1, 2: this leg's world force (a swing leg: +0, selected) and torque, summed over the legs
        double fw[3], F[3], T[3];
        A1_PL_MV(fw, R, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) fw[k] = stance ? fw[k] : 0.0;
        const double tq[3] = {r[1] * fw[2] - r[2] * fw[1], r[2] * fw[0] - r[0] * fw[2], r[0] * fw[1] - r[1] * fw[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            F[k] = pl_legs(fw[k]); T[k] = pl_legs(tq[k]);
            if (with_ext) { F[k] = F[k] + fe[k]; T[k] = T[k] + te[k]; }
        }
        // 3: semi-implicit Euler
        double dp[3];
        v[0] = v[0] + h * (F[0] / m); v[1] = v[1] + h * (F[1] / m); v[2] = v[2] + h * (F[2] / m + g);
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = h * v[k]; pos[k] = pos[k] + dp[k]; }
        // 4: R' = cay((h / 2) omega) R
        double Rn[9];
        {
            const double a0 = half * w[0], a1 = half * w[1], a2 = half * w[2];
            const double s = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
            const double Cm[9] = {1.0 - s * (a1 * a1 + a2 * a2), s * (a0 * a1 - a2), s * (a0 * a2 + a1),
                                  s * (a0 * a1 + a2), 1.0 - s * (a0 * a0 + a2 * a2), s * (a1 * a2 - a0),
                                  s * (a0 * a2 - a1), s * (a1 * a2 + a0), 1.0 - s * (a0 * a0 + a1 * a1)};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j];
        }
        // 5: L' = L + h tau, omega' = R' (I_b^-1 (R'^T L'))
        {
            double Lb[3], wb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) L[k] = L[k] + h * T[k];
            A1_PL_MTV(Lb, Rn, L); A1_PL_MV(wb, Ii, Lb); A1_PL_MV(w, Rn, wb);
        }
        // 6: a stance foot stays where it is in the world, a swing foot where it is in the body
        {
            double rb[3], rs[3];
            A1_PL_MTV(rb, R, r); A1_PL_MV(rs, Rn, rb);
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = stance ? r[k] - dp[k] : rs[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    }
    // the angles of rot_zyx, read off R (an output only)
    const double sp = -R[6], spc = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);   // (a NaN stays a NaN)
    const double roll = atan2(R[7], R[8]), pitch = asin(spc), yaw = atan2(R[3], R[0]);
    // out: lane l puts state triple l (0 euler, 1 pos, 2 omega, 3 v) and, l < 3, row l of R into the LDS images; the images go out as they came in
    WaveStage::sync();   // (every lane has read its inputs)
    if (alive) {
        double* x = S + q * stride + 3 * l;
        x[0] = pl_pick(l, roll, pos[0], w[0], v[0]); x[1] = pl_pick(l, pitch, pos[1], w[1], v[1]); x[2] = pl_pick(l, yaw, pos[2], w[2], v[2]);
        if (l < 3) {
            double* o = RL + q * 9 + 3 * l;
            o[0] = pl_pick(l, R[0], R[3], R[6], 0.0); o[1] = pl_pick(l, R[1], R[4], R[7], 0.0); o[2] = pl_pick(l, R[2], R[5], R[8], 0.0);
        }
        double* fo = a.foot_out + b * 12 + 3 * l;
        fo[0] = r[0]; fo[1] = r[1]; fo[2] = r[2];
    }
    WaveStage::sync();
    double *os = a.state_out + first * stride, *orr = a.R_out + first * 9;
#pragma unroll
    for (int mm = 0; mm < 6; ++mm) {
        const int e = lane + 64 * mm;
        const int col = stride == 12 ? e % 12 : (stride == 13 ? e % 13 : e % 22);
        if (e < cs && col < 12) os[e] = S[e];
    }
#pragma unroll
    for (int mm = 0; mm < 3; ++mm) { const int e = lane + 64 * mm; if (e < cr) orr[e] = RL[e]; }
}

// ---- sensor synthesis (a1mpc_sensor_synthesis_batch): what a robot's sensors read on the plant above -- the inverse of the tick's front stages (quaternion -> R, leg
// forward kinematics and Jacobian, the EKF's accelerometer and foot-velocity relations), so that  sensors -> tick -> plant -> sensors  closes on one stream.  The scheme is
// stated in include/a1mpc.h and restated elementwise in tests/sensor_synthesis_ref.py.
//   lanes     the plant step's: one wavefront = one workgroup = 16 consecutive robots, lane = 4 * (robot of the wave) + l; lane l holds leg l's lever, force and contact
//             byte and does leg l's inverse kinematics.  The accelerometer's leg sum is pl_legs, (leg 0 + leg 1) + (leg 2 + leg 3).
//   memory    state rows, R and the wrench pass through wave-private LDS in their memory layout; every global load is issued before the first operation.  The per-leg
//             outputs are a lane's own words ([robot][12] doubles, [robot][4] doubles and bytes): written directly, once.  The per-robot outputs (quaternion, the two IMU
//             vectors) are parked in LDS by lanes l of the robot (component l) and leave 64 consecutive doubles per instruction.
//   bits      contraction off and no fma; +, -, *, / and sqrt are IEEE, atan2 / acos / sin / cos the device library's.
//   dead lanes (robots >= n of the last wave) load the wave's first robot, take part in every shuffle and store nothing, neither to LDS nor to memory.
struct SynthArgs {
    int32_t n, stride;
    double mass, rho_fix[20], rho_opt[12];
    const double *state, *R, *foot, *grf, *ext;   // ext may be null
    const uint8_t* contacts;
    double *quat, *acc, *gyro, *jpos, *jvel, *fforce, *prel, *vrel;   // prel, vrel may be null
    uint8_t* reach;
};
__global__ __launch_bounds__(64) void a1mpc_sensor_synthesis_kernel(const SynthArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double slds[kPlState + kPlR + kPlExt];
    double* const S = slds; double* const RL = slds + kPlState; double* const E = slds + kPlState + kPlR;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    // every load, then the LDS writes, as in the plant step
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R;
    double vs[6], vr[3], ve[2];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
    double r[3], f[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0;
    const double *gf = a.rho_fix + 5 * l, *go = a.rho_opt + 3 * l;
    const double ox = gf[0], oy = gf[1], L = gf[2] + go[1], lt = gf[3], al = gf[4] - go[2], r0 = go[0];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
    WaveStage::sync();
    double w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fe[k] = E[q * 6 + k];
    }
    const double m = a.mass;
    // gyro = R^T omega; accelerometer = the specific force in the body frame: the stance legs' forces (a swing leg +0, selected) over m, plus R^T f_ext / m
    double gyro[3], acc[3];
    A1_PL_MTV(gyro, R, w);
    {
        double feb[3];
        A1_PL_MTV(feb, R, fe);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] = pl_legs(stance ? f[k] : 0.0) / m;
            if (with_ext) acc[k] = acc[k] + feb[k] / m;
        }
    }
    const double ff = stance ? (R[6] * f[0] + R[7] * f[1]) + R[8] * f[2] : 0.0;   // the world z component of R f_l
    // quaternion (w, x, y, z) of R: Eigen's matrix-to-quaternion, the four branches as selects of the operands around one sqrt
    double qt[4];
    {
        const double tr = (R[0] + R[4]) + R[8];
        const bool pos = tr > 0.0;
        const int i = R[4] > R[0] ? (R[8] > R[4] ? 2 : 1) : (R[8] > R[0] ? 2 : 0);   // the largest diagonal: j = (i + 1) % 3, k = (j + 1) % 3
        const double dii = pl_pick(i, R[0], R[4], R[8], 0.0), djj = pl_pick(i, R[4], R[8], R[0], 0.0), dkk = pl_pick(i, R[8], R[0], R[4], 0.0);
        const double kj = pl_pick(i, R[7], R[2], R[3], 0.0), jk = pl_pick(i, R[5], R[6], R[1], 0.0);   // R(k, j), R(j, k)
        const double ji = pl_pick(i, R[3], R[7], R[2], 0.0), ij = pl_pick(i, R[1], R[5], R[6], 0.0);
        const double ki = pl_pick(i, R[6], R[1], R[5], 0.0), ik = pl_pick(i, R[2], R[3], R[7], 0.0);
        const double t = sqrt(pos ? tr + 1.0 : ((dii - djj) - dkk) + 1.0), hq = 0.5 * t, u = 0.5 / t;
        const double qi = hq, qw4 = (kj - jk) * u, qj = (ji + ij) * u, qk = (ki + ik) * u;
        qt[0] = pos ? hq : qw4;
        qt[1] = pos ? (R[7] - R[5]) * u : pl_pick(i, qi, qk, qj, 0.0);
        qt[2] = pos ? (R[2] - R[6]) * u : pl_pick(i, qj, qi, qk, 0.0);
        qt[3] = pos ? (R[3] - R[1]) * u : pl_pick(i, qk, qj, qi, 0.0);
    }
    // this leg: p = R^T r; the closed-form inverse of a1mpc_leg_kernel's forward map (knee bent back); bit 0 / bit 1 of reach = the hip / knee argument was clamped
    double p[3], jq[3];
    A1_PL_MTV(p, R, r);
    const double dx = p[0] - ox, dy = p[1] - oy;
    const double yz = dy * dy + p[2] * p[2], LL = L * L;
    const bool clamp0 = yz < LL;
    const double Zi = -sqrt(clamp0 ? 0.0 : yz - LL);
    jq[0] = atan2(p[2], dy) - atan2(Zi, L);
    const double ell = sqrt(al * al + r0 * r0), phi = atan2(r0, al);
    const double cq = (((dx * dx + Zi * Zi) - lt * lt) - ell * ell) / ((2.0 * lt) * ell);
    const bool clamp1 = cq < -1.0 || cq > 1.0;
    const double kn = -acos(cq > 1.0 ? 1.0 : (cq < -1.0 ? -1.0 : cq));   // (a NaN stays a NaN)
    jq[1] = atan2(-dx, -Zi) - atan2(ell * sin(kn), lt + ell * cos(kn));
    jq[2] = kn + phi;
    const int flags = (clamp0 ? 1 : 0) | (clamp1 ? 2 : 0);
    // foot velocity in the body frame: a stance foot rests in the world, -(R^T (v + omega x r)); a swing foot rests in the body, +0
    double fv[3];
    {
        const double u[3] = {v[0] + (w[1] * r[2] - w[2] * r[1]), v[1] + (w[2] * r[0] - w[0] * r[2]), v[2] + (w[0] * r[1] - w[1] * r[0])};
        double ub[3];
        A1_PL_MTV(ub, R, u);
#pragma unroll
        for (int k = 0; k < 3; ++k) fv[k] = stance ? -ub[k] : 0.0;
    }
    // joint rates: the leg kernel's Jacobian at the synthesised angles, inverted by cofactors like the plant's I_b^-1; exactly +0 where a reach bit is set
    double jd[3];
    {
        const double s0 = sin(jq[0]), c0 = cos(jq[0]), s1 = sin(jq[1]), c1 = cos(jq[1]), s12 = sin(jq[1] + jq[2]), c12 = cos(jq[1] + jq[2]);
        const double Xq = r0 * c12 - al * s12, Zq = -(al * c12) - r0 * s12;
        const double Xr = Xq - lt * s1, Zp = Zq - lt * c1;
        const double py = oy + (L * c0 - Zp * s0), pz = L * s0 + Zp * c0;
        // row-major J: column c is d p / d q_c of the leg kernel (its J[3 c + row])
        const double I[9] = {0.0, Zp, Zq, -pz, s0 * Xr, s0 * Xq, py - oy, -(c0 * Xr), -(c0 * Xq)};
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        const double Ji[9] = {c00 * id, (I[2] * I[7] - I[1] * I[8]) * id, (I[1] * I[5] - I[2] * I[4]) * id,
                              c01 * id, (I[0] * I[8] - I[2] * I[6]) * id, (I[2] * I[3] - I[0] * I[5]) * id,
                              c02 * id, (I[1] * I[6] - I[0] * I[7]) * id, (I[0] * I[4] - I[1] * I[3]) * id};
        A1_PL_MV(jd, Ji, fv);
#pragma unroll
        for (int k = 0; k < 3; ++k) jd[k] = flags ? 0.0 : jd[k];
    }
    // out: a lane's own words directly; the per-robot vectors through the LDS images (every lane has read its inputs: sync first)
    WaveStage::sync();
    double* const QO = S; double* const AO = S + 64; double* const GO = S + 112;
    if (alive) {
        double *o0 = a.jpos + b * 12 + 3 * l, *o1 = a.jvel + b * 12 + 3 * l;
        o0[0] = jq[0]; o0[1] = jq[1]; o0[2] = jq[2]; o1[0] = jd[0]; o1[1] = jd[1]; o1[2] = jd[2];
        if (a.prel) { double* o = a.prel + b * 12 + 3 * l; o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
        if (a.vrel) { double* o = a.vrel + b * 12 + 3 * l; o[0] = fv[0]; o[1] = fv[1]; o[2] = fv[2]; }
        a.fforce[b * 4 + l] = ff;
        a.reach[b * 4 + l] = static_cast<uint8_t>(flags);
        QO[q * 4 + l] = pl_pick(l, qt[0], qt[1], qt[2], qt[3]);
        if (l < 3) { AO[q * 3 + l] = pl_pick(l, acc[0], acc[1], acc[2], 0.0); GO[q * 3 + l] = pl_pick(l, gyro[0], gyro[1], gyro[2], 0.0); }
    }
    WaveStage::sync();
    if (lane < live * 4) a.quat[first * 4 + lane] = QO[lane];
    if (lane < live * 3) { a.acc[first * 3 + lane] = AO[lane]; a.gyro[first * 3 + lane] = GO[lane]; }
}

// ---- walking plant (a1mpc_walk_step_batch, a1mpc_walk_sensors_batch): the plant step and the sensor synthesis above with swing feet that MOVE in the body frame, to the
// point the tick's swing-leg stage asks for (foot_pos_target_last_time), and a flat rigid ground under the feet.  Kernels of their own: the two above stay as they are,
// and with swing_track = 0 and flat_ground = 0 (foot_vel_body null) these compute their bits.  The scheme is stated in include/a1mpc.h and restated elementwise in
// tests/walk_ref.py.
//   lanes, memory, bits, dead lanes   those of a1mpc_plant_step_kernel.  R_z (shared by a robot's lanes) passes through wave-private LDS like R; the swing target, the
//             commanded foot velocity (out of the step, into the sensors) are a lane's own 24 bytes: moved directly.  With swing_track == 0 neither R_z nor the target is
//             read (wave-uniform: the kernel argument decides).
struct WalkArgs {
    PlantArgs p;
    double track, ground_z;
    int32_t flat_ground;
    const double *Rz, *target;   // null when track == 0
    double* vel_out;
};
__global__ __launch_bounds__(64) void a1mpc_walk_step_kernel(const WalkArgs wa) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double wlds[kPlState + kPlR + kPlExt + kPlR];
    double* const S = wlds; double* const RL = wlds + kPlState; double* const E = wlds + kPlState + kPlR; double* const ZL = wlds + kPlState + kPlR + kPlExt;
    const PlantArgs& a = wa.p;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    const bool track = wa.track != 0.0;
    // every load, then the LDS writes, as in the plant step
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0, cz = track ? cr : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R, *gzp = track ? wa.Rz + first * 9 : a.R;
    double vs[6], vr[3], ve[2], vz[3];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vz[m] = gzp[e < cz ? e : 0]; }
    double r[3], f[3], y[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l, *tp = track ? wa.target + b * 12 + 3 * l : fp;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2]; y[0] = tp[0]; y[1] = tp[1]; y[2] = tp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0;
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cz) ZL[e] = vz[m]; }
    WaveStage::sync();
    double pos[3], w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0}, te[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pos[k] = x[3 + k]; w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { fe[k] = E[q * 6 + k]; te[k] = E[q * 6 + 3 + k]; }
    }
    // 0: the plant step's polish of R, I_b^-1 and L
    {
        double E[9], Rp[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[3 * i + j] = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
        E[0] = E[0] - 1.0; E[4] = E[4] - 1.0; E[8] = E[8] - 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rp[3 * i + j] = R[3 * i + j] - 0.5 * ((R[3 * i] * E[j] + R[3 * i + 1] * E[3 + j]) + R[3 * i + 2] * E[6 + j]);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rp[k];
    }
    double Ii[9], L[3];
    {
        const double* I = a.inertia;
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        Ii[0] = c00 * id; Ii[1] = (I[2] * I[7] - I[1] * I[8]) * id; Ii[2] = (I[1] * I[5] - I[2] * I[4]) * id;
        Ii[3] = c01 * id; Ii[4] = (I[0] * I[8] - I[2] * I[6]) * id; Ii[5] = (I[2] * I[3] - I[0] * I[5]) * id;
        Ii[6] = c02 * id; Ii[7] = (I[1] * I[6] - I[0] * I[7]) * id; Ii[8] = (I[0] * I[4] - I[1] * I[3]) * id;
        double wb[3], Iw[3];
        A1_PL_MTV(wb, R, w); A1_PL_MV(Iw, I, wb); A1_PL_MV(L, R, Iw);
    }
    // the swing foot's move over the call, in the body frame of the polished R: from p0 = R^T r towards p_t = R^T (R_z y), the point the swing-leg stage asked for;
    // d per sub-step, vel the commanded velocity.  swing_track == 0: both exactly +0, selected
    double d[3] = {0.0, 0.0, 0.0}, vel[3] = {0.0, 0.0, 0.0};
    if (track) {
        double Rz[9], p0[3], tw[3], pt[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rz[k] = ZL[q * 9 + k];
        A1_PL_MTV(p0, R, r); A1_PL_MV(tw, Rz, y); A1_PL_MTV(pt, R, tw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dl = wa.track * (pt[k] - p0[k]);
            d[k] = dl / static_cast<double>(a.substeps); vel[k] = dl / a.dt;
        }
    }
    const double h = a.dt / static_cast<double>(a.substeps), half = h / 2.0, m = a.mass, g = a.gravity;
    for (int step = 0; step < a.substeps; ++step) {
        // 1 .. 5: the plant step's
        double fw[3], F[3], T[3];
        A1_PL_MV(fw, R, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) fw[k] = stance ? fw[k] : 0.0;
        const double tq[3] = {r[1] * fw[2] - r[2] * fw[1], r[2] * fw[0] - r[0] * fw[2], r[0] * fw[1] - r[1] * fw[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            F[k] = pl_legs(fw[k]); T[k] = pl_legs(tq[k]);
            if (with_ext) { F[k] = F[k] + fe[k]; T[k] = T[k] + te[k]; }
        }
        double dp[3];
        v[0] = v[0] + h * (F[0] / m); v[1] = v[1] + h * (F[1] / m); v[2] = v[2] + h * (F[2] / m + g);
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = h * v[k]; pos[k] = pos[k] + dp[k]; }
        double Rn[9];
        {
            const double a0 = half * w[0], a1 = half * w[1], a2 = half * w[2];
            const double s = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
            const double Cm[9] = {1.0 - s * (a1 * a1 + a2 * a2), s * (a0 * a1 - a2), s * (a0 * a2 + a1),
                                  s * (a0 * a1 + a2), 1.0 - s * (a0 * a0 + a2 * a2), s * (a1 * a2 - a0),
                                  s * (a0 * a2 - a1), s * (a1 * a2 + a0), 1.0 - s * (a0 * a0 + a1 * a1)};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j];
        }
        {
            double Lb[3], wb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) L[k] = L[k] + h * T[k];
            A1_PL_MTV(Lb, Rn, L); A1_PL_MV(wb, Ii, Lb); A1_PL_MV(w, Rn, wb);
        }
        // 6: a stance foot stays where it is in the world; a swing foot moves by d in the body (swing_track == 0: the sum is skipped, the plant step's bits)
        {
            double rb[3], rs[3];
            A1_PL_MTV(rb, R, r);
            if (track) {
#pragma unroll
                for (int k = 0; k < 3; ++k) rb[k] = rb[k] + d[k];
            }
            A1_PL_MV(rs, Rn, rb);
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = stance ? r[k] - dp[k] : rs[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    }
    // the flat ground, once per call: a stance foot ON the plane z = ground_z of the world, a swing foot not below it (a NaN stays a NaN)
    if (wa.flat_ground) {
        const double gz = wa.ground_z - pos[2];
        r[2] = stance ? gz : (r[2] < gz ? gz : r[2]);
    }
    const double sp = -R[6], spc = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);   // (a NaN stays a NaN)
    const double roll = atan2(R[7], R[8]), pitch = asin(spc), yaw = atan2(R[3], R[0]);
    // out: as the plant step, and the commanded swing velocity (a stance leg: +0, selected -- its target reaches no output)
    WaveStage::sync();   // (every lane has read its inputs)
    if (alive) {
        double* x = S + q * stride + 3 * l;
        x[0] = pl_pick(l, roll, pos[0], w[0], v[0]); x[1] = pl_pick(l, pitch, pos[1], w[1], v[1]); x[2] = pl_pick(l, yaw, pos[2], w[2], v[2]);
        if (l < 3) {
            double* o = RL + q * 9 + 3 * l;
            o[0] = pl_pick(l, R[0], R[3], R[6], 0.0); o[1] = pl_pick(l, R[1], R[4], R[7], 0.0); o[2] = pl_pick(l, R[2], R[5], R[8], 0.0);
        }
        double *fo = a.foot_out + b * 12 + 3 * l, *vo = wa.vel_out + b * 12 + 3 * l;
        fo[0] = r[0]; fo[1] = r[1]; fo[2] = r[2];
        vo[0] = stance ? 0.0 : vel[0]; vo[1] = stance ? 0.0 : vel[1]; vo[2] = stance ? 0.0 : vel[2];
    }
    WaveStage::sync();
    double *os = a.state_out + first * stride, *orr = a.R_out + first * 9;
#pragma unroll
    for (int mm = 0; mm < 6; ++mm) {
        const int e = lane + 64 * mm;
        const int col = stride == 12 ? e % 12 : (stride == 13 ? e % 13 : e % 22);
        if (e < cs && col < 12) os[e] = S[e];
    }
#pragma unroll
    for (int mm = 0; mm < 3; ++mm) { const int e = lane + 64 * mm; if (e < cr) orr[e] = RL[e]; }
}

// the sensors of the walking plant: a1mpc_sensor_synthesis_kernel's arithmetic, except that a swing leg's foot_vel_rel is the commanded body-frame velocity the walk step
// wrote (vel null: +0, the synthesis kernel's bits) and its joint rates J(q)^-1 of that
struct WalkSensorArgs {
    SynthArgs s;
    const double* vel;   // may be null
};
__global__ __launch_bounds__(64) void a1mpc_walk_sensors_kernel(const WalkSensorArgs wa) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double xlds[kPlState + kPlR + kPlExt];
    double* const S = xlds; double* const RL = xlds + kPlState; double* const E = xlds + kPlState + kPlR;
    const SynthArgs& a = wa.s;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    // every load, then the LDS writes, as in the plant step
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R;
    double vs[6], vr[3], ve[2];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
    double r[3], f[3], fb[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l, *vp = wa.vel ? wa.vel + b * 12 + 3 * l : fp;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2]; fb[0] = vp[0]; fb[1] = vp[1]; fb[2] = vp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0, with_vel = wa.vel != nullptr;
    const double *gf = a.rho_fix + 5 * l, *go = a.rho_opt + 3 * l;
    const double ox = gf[0], oy = gf[1], L = gf[2] + go[1], lt = gf[3], al = gf[4] - go[2], r0 = go[0];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
    WaveStage::sync();
    double w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fe[k] = E[q * 6 + k];
    }
    const double m = a.mass;
    double gyro[3], acc[3];
    A1_PL_MTV(gyro, R, w);
    {
        double feb[3];
        A1_PL_MTV(feb, R, fe);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] = pl_legs(stance ? f[k] : 0.0) / m;
            if (with_ext) acc[k] = acc[k] + feb[k] / m;
        }
    }
    const double ff = stance ? (R[6] * f[0] + R[7] * f[1]) + R[8] * f[2] : 0.0;
    double qt[4];
    {
        const double tr = (R[0] + R[4]) + R[8];
        const bool pos = tr > 0.0;
        const int i = R[4] > R[0] ? (R[8] > R[4] ? 2 : 1) : (R[8] > R[0] ? 2 : 0);
        const double dii = pl_pick(i, R[0], R[4], R[8], 0.0), djj = pl_pick(i, R[4], R[8], R[0], 0.0), dkk = pl_pick(i, R[8], R[0], R[4], 0.0);
        const double kj = pl_pick(i, R[7], R[2], R[3], 0.0), jk = pl_pick(i, R[5], R[6], R[1], 0.0);
        const double ji = pl_pick(i, R[3], R[7], R[2], 0.0), ij = pl_pick(i, R[1], R[5], R[6], 0.0);
        const double ki = pl_pick(i, R[6], R[1], R[5], 0.0), ik = pl_pick(i, R[2], R[3], R[7], 0.0);
        const double t = sqrt(pos ? tr + 1.0 : ((dii - djj) - dkk) + 1.0), hq = 0.5 * t, u = 0.5 / t;
        const double qi = hq, qw4 = (kj - jk) * u, qj = (ji + ij) * u, qk = (ki + ik) * u;
        qt[0] = pos ? hq : qw4;
        qt[1] = pos ? (R[7] - R[5]) * u : pl_pick(i, qi, qk, qj, 0.0);
        qt[2] = pos ? (R[2] - R[6]) * u : pl_pick(i, qj, qi, qk, 0.0);
        qt[3] = pos ? (R[3] - R[1]) * u : pl_pick(i, qk, qj, qi, 0.0);
    }
    double p[3], jq[3];
    A1_PL_MTV(p, R, r);
    const double dx = p[0] - ox, dy = p[1] - oy;
    const double yz = dy * dy + p[2] * p[2], LL = L * L;
    const bool clamp0 = yz < LL;
    const double Zi = -sqrt(clamp0 ? 0.0 : yz - LL);
    jq[0] = atan2(p[2], dy) - atan2(Zi, L);
    const double ell = sqrt(al * al + r0 * r0), phi = atan2(r0, al);
    const double cq = (((dx * dx + Zi * Zi) - lt * lt) - ell * ell) / ((2.0 * lt) * ell);
    const bool clamp1 = cq < -1.0 || cq > 1.0;
    const double kn = -acos(cq > 1.0 ? 1.0 : (cq < -1.0 ? -1.0 : cq));   // (a NaN stays a NaN)
    jq[1] = atan2(-dx, -Zi) - atan2(ell * sin(kn), lt + ell * cos(kn));
    jq[2] = kn + phi;
    const int flags = (clamp0 ? 1 : 0) | (clamp1 ? 2 : 0);
    // foot velocity in the body frame: a stance foot rests in the world, -(R^T (v + omega x r)); a swing foot moves as commanded (no command given: +0), selected
    double fv[3];
    {
        const double u[3] = {v[0] + (w[1] * r[2] - w[2] * r[1]), v[1] + (w[2] * r[0] - w[0] * r[2]), v[2] + (w[0] * r[1] - w[1] * r[0])};
        double ub[3];
        A1_PL_MTV(ub, R, u);
#pragma unroll
        for (int k = 0; k < 3; ++k) fv[k] = stance ? -ub[k] : (with_vel ? fb[k] : 0.0);
    }
    double jd[3];
    {
        const double s0 = sin(jq[0]), c0 = cos(jq[0]), s1 = sin(jq[1]), c1 = cos(jq[1]), s12 = sin(jq[1] + jq[2]), c12 = cos(jq[1] + jq[2]);
        const double Xq = r0 * c12 - al * s12, Zq = -(al * c12) - r0 * s12;
        const double Xr = Xq - lt * s1, Zp = Zq - lt * c1;
        const double py = oy + (L * c0 - Zp * s0), pz = L * s0 + Zp * c0;
        const double I[9] = {0.0, Zp, Zq, -pz, s0 * Xr, s0 * Xq, py - oy, -(c0 * Xr), -(c0 * Xq)};
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        const double Ji[9] = {c00 * id, (I[2] * I[7] - I[1] * I[8]) * id, (I[1] * I[5] - I[2] * I[4]) * id,
                              c01 * id, (I[0] * I[8] - I[2] * I[6]) * id, (I[2] * I[3] - I[0] * I[5]) * id,
                              c02 * id, (I[1] * I[6] - I[0] * I[7]) * id, (I[0] * I[4] - I[1] * I[3]) * id};
        A1_PL_MV(jd, Ji, fv);
#pragma unroll
        for (int k = 0; k < 3; ++k) jd[k] = flags ? 0.0 : jd[k];
    }
    WaveStage::sync();
    double* const QO = S; double* const AO = S + 64; double* const GO = S + 112;
    if (alive) {
        double *o0 = a.jpos + b * 12 + 3 * l, *o1 = a.jvel + b * 12 + 3 * l;
        o0[0] = jq[0]; o0[1] = jq[1]; o0[2] = jq[2]; o1[0] = jd[0]; o1[1] = jd[1]; o1[2] = jd[2];
        if (a.prel) { double* o = a.prel + b * 12 + 3 * l; o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
        if (a.vrel) { double* o = a.vrel + b * 12 + 3 * l; o[0] = fv[0]; o[1] = fv[1]; o[2] = fv[2]; }
        a.fforce[b * 4 + l] = ff;
        a.reach[b * 4 + l] = static_cast<uint8_t>(flags);
        QO[q * 4 + l] = pl_pick(l, qt[0], qt[1], qt[2], qt[3]);
        if (l < 3) { AO[q * 3 + l] = pl_pick(l, acc[0], acc[1], acc[2], 0.0); GO[q * 3 + l] = pl_pick(l, gyro[0], gyro[1], gyro[2], 0.0); }
    }
    WaveStage::sync();
    if (lane < live * 4) a.quat[first * 4 + lane] = QO[lane];
    if (lane < live * 3) { a.acc[first * 3 + lane] = AO[lane]; a.gyro[first * 3 + lane] = GO[lane]; }
}

// ---- sloped ground and sensed touchdowns (a1mpc_ground_step_batch, a1mpc_touch_sensors_batch): the two walk kernels above with a ground plane PER ROBOT,
// hz(X, Y) = (z0 + sx X) + sy Y in the world, and a touch byte per leg that says whether the ground holds the foot.  Third copies, not templates of the two above: those
// keep their text, their code objects and their host emulation byte for byte.  The scheme is stated in include/a1mpc.h and restated elementwise in tests/ground_ref.py.
//   lanes, memory, bits, dead lanes   those of a1mpc_walk_step_kernel.  A robot's plane (three words, shared by its four lanes) passes through wave-private LDS like
//             R_z; the touch byte is a lane's own: stored (out of the step) and loaded (into the sensors) directly.  ground null: cfg's plane z = ground_z, or none.
struct WalkGroundArgs {
    WalkArgs w;
    const double* ground;   // may be null: then w.flat_ground / w.ground_z decide
    uint8_t* touch;
};
__global__ __launch_bounds__(64) void a1mpc_walk_step_ground_kernel(const WalkGroundArgs ga) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double glds[kPlState + kPlR + kPlExt + kPlR + 16 * 3];
    double* const S = glds; double* const RL = glds + kPlState; double* const E = glds + kPlState + kPlR; double* const ZL = glds + kPlState + kPlR + kPlExt;
    double* const GL = glds + kPlState + kPlR + kPlExt + kPlR;
    const WalkArgs& wa = ga.w;
    const PlantArgs& a = wa.p;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    const bool track = wa.track != 0.0, sloped = ga.ground != nullptr;
    // every load, then the LDS writes, as in the walk step; the planes are 48 words at most: one load per lane
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0, cz = track ? cr : 0, cg = sloped ? live * 3 : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R, *gzp = track ? wa.Rz + first * 9 : a.R;
    const double* gg = sloped ? ga.ground + first * 3 : a.R;
    double vs[6], vr[3], ve[2], vz[3];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vz[m] = gzp[e < cz ? e : 0]; }
    const double vg = gg[lane < cg ? lane : 0];
    double r[3], f[3], y[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l, *tp = track ? wa.target + b * 12 + 3 * l : fp;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2]; y[0] = tp[0]; y[1] = tp[1]; y[2] = tp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0;
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cz) ZL[e] = vz[m]; }
    if (lane < cg) GL[lane] = vg;
    WaveStage::sync();
    double pos[3], w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0}, te[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pos[k] = x[3 + k]; w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { fe[k] = E[q * 6 + k]; te[k] = E[q * 6 + 3 + k]; }
    }
    // 0: the plant step's polish of R, I_b^-1 and L
    {
        double E[9], Rp[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[3 * i + j] = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
        E[0] = E[0] - 1.0; E[4] = E[4] - 1.0; E[8] = E[8] - 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rp[3 * i + j] = R[3 * i + j] - 0.5 * ((R[3 * i] * E[j] + R[3 * i + 1] * E[3 + j]) + R[3 * i + 2] * E[6 + j]);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rp[k];
    }
    double Ii[9], L[3];
    {
        const double* I = a.inertia;
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        Ii[0] = c00 * id; Ii[1] = (I[2] * I[7] - I[1] * I[8]) * id; Ii[2] = (I[1] * I[5] - I[2] * I[4]) * id;
        Ii[3] = c01 * id; Ii[4] = (I[0] * I[8] - I[2] * I[6]) * id; Ii[5] = (I[2] * I[3] - I[0] * I[5]) * id;
        Ii[6] = c02 * id; Ii[7] = (I[1] * I[6] - I[0] * I[7]) * id; Ii[8] = (I[0] * I[4] - I[1] * I[3]) * id;
        double wb[3], Iw[3];
        A1_PL_MTV(wb, R, w); A1_PL_MV(Iw, I, wb); A1_PL_MV(L, R, Iw);
    }
    // the swing foot's move over the call: the walk step's
    double d[3] = {0.0, 0.0, 0.0}, vel[3] = {0.0, 0.0, 0.0};
    if (track) {
        double Rz[9], p0[3], tw[3], pt[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rz[k] = ZL[q * 9 + k];
        A1_PL_MTV(p0, R, r); A1_PL_MV(tw, Rz, y); A1_PL_MTV(pt, R, tw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dl = wa.track * (pt[k] - p0[k]);
            d[k] = dl / static_cast<double>(a.substeps); vel[k] = dl / a.dt;
        }
    }
    const double h = a.dt / static_cast<double>(a.substeps), half = h / 2.0, m = a.mass, g = a.gravity;
    for (int step = 0; step < a.substeps; ++step) {
        // 1 .. 6: the walk step's
        double fw[3], F[3], T[3];
        A1_PL_MV(fw, R, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) fw[k] = stance ? fw[k] : 0.0;
        const double tq[3] = {r[1] * fw[2] - r[2] * fw[1], r[2] * fw[0] - r[0] * fw[2], r[0] * fw[1] - r[1] * fw[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            F[k] = pl_legs(fw[k]); T[k] = pl_legs(tq[k]);
            if (with_ext) { F[k] = F[k] + fe[k]; T[k] = T[k] + te[k]; }
        }
        double dp[3];
        v[0] = v[0] + h * (F[0] / m); v[1] = v[1] + h * (F[1] / m); v[2] = v[2] + h * (F[2] / m + g);
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = h * v[k]; pos[k] = pos[k] + dp[k]; }
        double Rn[9];
        {
            const double a0 = half * w[0], a1 = half * w[1], a2 = half * w[2];
            const double s = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
            const double Cm[9] = {1.0 - s * (a1 * a1 + a2 * a2), s * (a0 * a1 - a2), s * (a0 * a2 + a1),
                                  s * (a0 * a1 + a2), 1.0 - s * (a0 * a0 + a2 * a2), s * (a1 * a2 - a0),
                                  s * (a0 * a2 - a1), s * (a1 * a2 + a0), 1.0 - s * (a0 * a0 + a1 * a1)};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j];
        }
        {
            double Lb[3], wb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) L[k] = L[k] + h * T[k];
            A1_PL_MTV(Lb, Rn, L); A1_PL_MV(wb, Ii, Lb); A1_PL_MV(w, Rn, wb);
        }
        {
            double rb[3], rs[3];
            A1_PL_MTV(rb, R, r);
            if (track) {
#pragma unroll
                for (int k = 0; k < 3; ++k) rb[k] = rb[k] + d[k];
            }
            A1_PL_MV(rs, Rn, rb);
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = stance ? r[k] - dp[k] : rs[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    }
    // the ground, once per call, straight down: a stance foot ON its robot's plane under its own x and y, a swing foot not below it.  touch: stance, or the comparison
    // that lifted the swing foot (a NaN compares false: the foot keeps its z and touch is 0).  No ground at all: a swing leg touches nothing
    bool touch = stance;
    if (sloped || wa.flat_ground) {
        double top = wa.ground_z;
        if (sloped) {   // (the plane's words wait in LDS until here: its image is not written again)
            const double z0 = GL[q * 3], sx = GL[q * 3 + 1], sy = GL[q * 3 + 2];
            const double X = pos[0] + r[0], Y = pos[1] + r[1];
            top = (z0 + sx * X) + sy * Y;
        }
        const double gz = top - pos[2];
        const bool lifted = r[2] < gz;
        r[2] = stance ? gz : (lifted ? gz : r[2]);
        touch = stance || lifted;
    }
    const double sp = -R[6], spc = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);   // (a NaN stays a NaN)
    const double roll = atan2(R[7], R[8]), pitch = asin(spc), yaw = atan2(R[3], R[0]);
    WaveStage::sync();   // (every lane has read its inputs)
    if (alive) {
        double* x = S + q * stride + 3 * l;
        x[0] = pl_pick(l, roll, pos[0], w[0], v[0]); x[1] = pl_pick(l, pitch, pos[1], w[1], v[1]); x[2] = pl_pick(l, yaw, pos[2], w[2], v[2]);
        if (l < 3) {
            double* o = RL + q * 9 + 3 * l;
            o[0] = pl_pick(l, R[0], R[3], R[6], 0.0); o[1] = pl_pick(l, R[1], R[4], R[7], 0.0); o[2] = pl_pick(l, R[2], R[5], R[8], 0.0);
        }
        double *fo = a.foot_out + b * 12 + 3 * l, *vo = wa.vel_out + b * 12 + 3 * l;
        fo[0] = r[0]; fo[1] = r[1]; fo[2] = r[2];
        vo[0] = stance ? 0.0 : vel[0]; vo[1] = stance ? 0.0 : vel[1]; vo[2] = stance ? 0.0 : vel[2];
        ga.touch[b * 4 + l] = touch ? uint8_t{1} : uint8_t{0};
    }
    WaveStage::sync();
    double *os = a.state_out + first * stride, *orr = a.R_out + first * 9;
#pragma unroll
    for (int mm = 0; mm < 6; ++mm) {
        const int e = lane + 64 * mm;
        const int col = stride == 12 ? e % 12 : (stride == 13 ? e % 13 : e % 22);
        if (e < cs && col < 12) os[e] = S[e];
    }
#pragma unroll
    for (int mm = 0; mm < 3; ++mm) { const int e = lane + 64 * mm; if (e < cr) orr[e] = RL[e]; }
}

// the sensors of the walking plant with a touch sensor: a1mpc_walk_sensors_kernel's arithmetic, except that a swing leg whose touch byte is set reports touch_force
// (selected, not added; a stance leg's byte reaches no output).  touch null, or touch_force == +0: the walk sensors' bits
struct WalkTouchArgs {
    WalkSensorArgs w;
    const uint8_t* touch;   // may be null
    double touch_force;
};
__global__ __launch_bounds__(64) void a1mpc_walk_sensors_touch_kernel(const WalkTouchArgs ta) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double tlds[kPlState + kPlR + kPlExt];
    double* const S = tlds; double* const RL = tlds + kPlState; double* const E = tlds + kPlState + kPlR;
    const WalkSensorArgs& wa = ta.w;
    const SynthArgs& a = wa.s;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    // every load, then the LDS writes, as in the plant step
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R;
    double vs[6], vr[3], ve[2];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
    double r[3], f[3], fb[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l, *vp = wa.vel ? wa.vel + b * 12 + 3 * l : fp;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2]; fb[0] = vp[0]; fb[1] = vp[1]; fb[2] = vp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0, with_vel = wa.vel != nullptr;
    const bool touched = (ta.touch ? ta.touch : a.contacts)[b * 4 + l] != 0 && ta.touch != nullptr;
    const double *gf = a.rho_fix + 5 * l, *go = a.rho_opt + 3 * l;
    const double ox = gf[0], oy = gf[1], L = gf[2] + go[1], lt = gf[3], al = gf[4] - go[2], r0 = go[0];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
    WaveStage::sync();
    double w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fe[k] = E[q * 6 + k];
    }
    const double m = a.mass;
    double gyro[3], acc[3];
    A1_PL_MTV(gyro, R, w);
    {
        double feb[3];
        A1_PL_MTV(feb, R, fe);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] = pl_legs(stance ? f[k] : 0.0) / m;
            if (with_ext) acc[k] = acc[k] + feb[k] / m;
        }
    }
    // the foot-force sensor: a stance leg's applied force along the world's z; a swing leg the ground holds reports the constant, any other swing leg +0
    const double ff = stance ? (R[6] * f[0] + R[7] * f[1]) + R[8] * f[2] : (touched ? ta.touch_force : 0.0);
    double qt[4];
    {
        const double tr = (R[0] + R[4]) + R[8];
        const bool pos = tr > 0.0;
        const int i = R[4] > R[0] ? (R[8] > R[4] ? 2 : 1) : (R[8] > R[0] ? 2 : 0);
        const double dii = pl_pick(i, R[0], R[4], R[8], 0.0), djj = pl_pick(i, R[4], R[8], R[0], 0.0), dkk = pl_pick(i, R[8], R[0], R[4], 0.0);
        const double kj = pl_pick(i, R[7], R[2], R[3], 0.0), jk = pl_pick(i, R[5], R[6], R[1], 0.0);
        const double ji = pl_pick(i, R[3], R[7], R[2], 0.0), ij = pl_pick(i, R[1], R[5], R[6], 0.0);
        const double ki = pl_pick(i, R[6], R[1], R[5], 0.0), ik = pl_pick(i, R[2], R[3], R[7], 0.0);
        const double t = sqrt(pos ? tr + 1.0 : ((dii - djj) - dkk) + 1.0), hq = 0.5 * t, u = 0.5 / t;
        const double qi = hq, qw4 = (kj - jk) * u, qj = (ji + ij) * u, qk = (ki + ik) * u;
        qt[0] = pos ? hq : qw4;
        qt[1] = pos ? (R[7] - R[5]) * u : pl_pick(i, qi, qk, qj, 0.0);
        qt[2] = pos ? (R[2] - R[6]) * u : pl_pick(i, qj, qi, qk, 0.0);
        qt[3] = pos ? (R[3] - R[1]) * u : pl_pick(i, qk, qj, qi, 0.0);
    }
    double p[3], jq[3];
    A1_PL_MTV(p, R, r);
    const double dx = p[0] - ox, dy = p[1] - oy;
    const double yz = dy * dy + p[2] * p[2], LL = L * L;
    const bool clamp0 = yz < LL;
    const double Zi = -sqrt(clamp0 ? 0.0 : yz - LL);
    jq[0] = atan2(p[2], dy) - atan2(Zi, L);
    const double ell = sqrt(al * al + r0 * r0), phi = atan2(r0, al);
    const double cq = (((dx * dx + Zi * Zi) - lt * lt) - ell * ell) / ((2.0 * lt) * ell);
    const bool clamp1 = cq < -1.0 || cq > 1.0;
    const double kn = -acos(cq > 1.0 ? 1.0 : (cq < -1.0 ? -1.0 : cq));   // (a NaN stays a NaN)
    jq[1] = atan2(-dx, -Zi) - atan2(ell * sin(kn), lt + ell * cos(kn));
    jq[2] = kn + phi;
    const int flags = (clamp0 ? 1 : 0) | (clamp1 ? 2 : 0);
    double fv[3];
    {
        const double u[3] = {v[0] + (w[1] * r[2] - w[2] * r[1]), v[1] + (w[2] * r[0] - w[0] * r[2]), v[2] + (w[0] * r[1] - w[1] * r[0])};
        double ub[3];
        A1_PL_MTV(ub, R, u);
#pragma unroll
        for (int k = 0; k < 3; ++k) fv[k] = stance ? -ub[k] : (with_vel ? fb[k] : 0.0);
    }
    double jd[3];
    {
        const double s0 = sin(jq[0]), c0 = cos(jq[0]), s1 = sin(jq[1]), c1 = cos(jq[1]), s12 = sin(jq[1] + jq[2]), c12 = cos(jq[1] + jq[2]);
        const double Xq = r0 * c12 - al * s12, Zq = -(al * c12) - r0 * s12;
        const double Xr = Xq - lt * s1, Zp = Zq - lt * c1;
        const double py = oy + (L * c0 - Zp * s0), pz = L * s0 + Zp * c0;
        const double I[9] = {0.0, Zp, Zq, -pz, s0 * Xr, s0 * Xq, py - oy, -(c0 * Xr), -(c0 * Xq)};
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        const double Ji[9] = {c00 * id, (I[2] * I[7] - I[1] * I[8]) * id, (I[1] * I[5] - I[2] * I[4]) * id,
                              c01 * id, (I[0] * I[8] - I[2] * I[6]) * id, (I[2] * I[3] - I[0] * I[5]) * id,
                              c02 * id, (I[1] * I[6] - I[0] * I[7]) * id, (I[0] * I[4] - I[1] * I[3]) * id};
        A1_PL_MV(jd, Ji, fv);
#pragma unroll
        for (int k = 0; k < 3; ++k) jd[k] = flags ? 0.0 : jd[k];
    }
    WaveStage::sync();
    double* const QO = S; double* const AO = S + 64; double* const GO = S + 112;
    if (alive) {
        double *o0 = a.jpos + b * 12 + 3 * l, *o1 = a.jvel + b * 12 + 3 * l;
        o0[0] = jq[0]; o0[1] = jq[1]; o0[2] = jq[2]; o1[0] = jd[0]; o1[1] = jd[1]; o1[2] = jd[2];
        if (a.prel) { double* o = a.prel + b * 12 + 3 * l; o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
        if (a.vrel) { double* o = a.vrel + b * 12 + 3 * l; o[0] = fv[0]; o[1] = fv[1]; o[2] = fv[2]; }
        a.fforce[b * 4 + l] = ff;
        a.reach[b * 4 + l] = static_cast<uint8_t>(flags);
        QO[q * 4 + l] = pl_pick(l, qt[0], qt[1], qt[2], qt[3]);
        if (l < 3) { AO[q * 3 + l] = pl_pick(l, acc[0], acc[1], acc[2], 0.0); GO[q * 3 + l] = pl_pick(l, gyro[0], gyro[1], gyro[2], 0.0); }
    }
    WaveStage::sync();
    if (lane < live * 4) a.quat[first * 4 + lane] = QO[lane];
    if (lane < live * 3) { a.acc[first * 3 + lane] = AO[lane]; a.gyro[first * 3 + lane] = GO[lane]; }
}

// ---- height-field terrain (a1mpc_heightfield_step_batch, a1mpc_heightfield_sample_batch): the ground step above with ONE gridded field of heights in place of the
// plane per robot -- stairs, kerbs, rough ground -- reached by every robot through an optional origin row (ox, oy, oz), so that several terrains in one batch are tiles
// of one field.  A fourth copy, not a template: the three step kernels above keep their text, their code objects and their host emulation byte for byte.  The rule
// hf(X, Y) is stated in include/a1mpc.h and restated elementwise in tests/heightfield_ref.py; both kernels below call the one function that holds it.
//   lanes, memory, bits, dead lanes   those of a1mpc_walk_step_ground_kernel; a robot's origin row takes the plane's place in wave-private LDS.  The field stays in global
//             memory: a lane gathers one node (cell-constant) or four (bilinear) under its foot and as many under its body, after pos' and r' are known.  The two gathers
//             are issued together, so the kernel has ONE exposed memory round trip behind its input loads.  A dead lane samples node (0, 0) and stores nothing.
struct HfField {   // a1mpc_heightfield as the kernels take it: the reciprocals of the spacings are made once on the host
    const double* H;
    double x0, y0, inv_dx, inv_dy;
    int32_t nx, ny, interp;
};
// hf(X, Y) in the header's operation order.  interp is passed apart from f so that a caller's branch on it folds here; shifted: an origin row is given (ox, oy, oz);
// live false: the lane belongs to no robot and reads node (0, 0).  Only the clamped cx, cy -- finite, in [0, nx - 1] and [0, ny - 1] -- are ever converted to an integer
__device__ __forceinline__ double hf_sample(const HfField& f, const int interp, const bool live, const bool shifted, const double ox, const double oy, const double oz,
                                            const double X, const double Y) {
#pragma clang fp contract(off)
    double ux, uy;
    if (shifted) { ux = ((X - ox) - f.x0) * f.inv_dx; uy = ((Y - oy) - f.y0) * f.inv_dy; }
    else { ux = (X - f.x0) * f.inv_dx; uy = (Y - f.y0) * f.inv_dy; }
    const bool valid = (ux == ux) && (uy == uy);
    const double mx = static_cast<double>(f.nx - 1), my = static_cast<double>(f.ny - 1);
    double cx = ux > 0.0 ? ux : 0.0, cy = uy > 0.0 ? uy : 0.0;   // (a NaN goes to 0)
    cx = cx < mx ? cx : mx; cy = cy < my ? cy : my;
    cx = live ? cx : 0.0; cy = live ? cy : 0.0;
    const int64_t nx = f.nx;
    double h;
    if (interp == 0) {
        const int64_t i = static_cast<int>(cx), j = static_cast<int>(cy);
        h = f.H[j * nx + i];
    } else {
        int i = static_cast<int>(cx), j = static_cast<int>(cy);
        i = i < f.nx - 1 ? i : f.nx - 2; j = j < f.ny - 1 ? j : f.ny - 2;
        const double tx = cx - static_cast<double>(i), ty = cy - static_cast<double>(j);
        const double* p = f.H + (static_cast<int64_t>(j) * nx + i);
        const double h00 = p[0], h10 = p[1], h01 = p[nx], h11 = p[nx + 1];
        const double a = h00 + tx * (h10 - h00), b = h01 + tx * (h11 - h01);
        h = a + ty * (b - a);
    }
    double top = valid ? h : __builtin_nan("");
    if (shifted) top = top + oz;
    return top;
}
struct WalkHeightfieldArgs {
    WalkArgs w;             // (w.flat_ground / w.ground_z are not read)
    HfField f;
    const double* origin;   // may be null
    uint8_t* touch;
    double* ground_out;     // may be null
};
__global__ __launch_bounds__(64) void a1mpc_walk_step_heightfield_kernel(const WalkHeightfieldArgs ha) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double hlds[kPlState + kPlR + kPlExt + kPlR + 16 * 3];
    double* const S = hlds; double* const RL = hlds + kPlState; double* const E = hlds + kPlState + kPlR; double* const ZL = hlds + kPlState + kPlR + kPlExt;
    double* const GL = hlds + kPlState + kPlR + kPlExt + kPlR;
    const WalkArgs& wa = ha.w;
    const PlantArgs& a = wa.p;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    const bool track = wa.track != 0.0, shifted = ha.origin != nullptr;
    // every load, then the LDS writes, as in the ground step; the origin rows are 48 words at most: one load per lane
    const int cs = live * stride, cr = live * 9, ce = a.ext ? live * 6 : 0, cz = track ? cr : 0, cg = shifted ? live * 3 : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9, *ge = a.ext ? a.ext + first * 6 : a.R, *gzp = track ? wa.Rz + first * 9 : a.R;
    const double* gg = shifted ? ha.origin + first * 3 : a.R;
    double vs[6], vr[3], ve[2], vz[3];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; ve[m] = ge[e < ce ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vz[m] = gzp[e < cz ? e : 0]; }
    const double vg = gg[lane < cg ? lane : 0];
    double r[3], f[3], y[3];
    {
        const double *fp = a.foot + b * 12 + 3 * l, *gp = a.grf + b * 12 + 3 * l, *tp = track ? wa.target + b * 12 + 3 * l : fp;
        r[0] = fp[0]; r[1] = fp[1]; r[2] = fp[2]; f[0] = gp[0]; f[1] = gp[1]; f[2] = gp[2]; y[0] = tp[0]; y[1] = tp[1]; y[2] = tp[2];
    }
    const bool stance = a.contacts[b * 4 + l] != 0;
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 2; ++m) { const int e = lane + 64 * m; if (e < ce) E[e] = ve[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cz) ZL[e] = vz[m]; }
    if (lane < cg) GL[lane] = vg;
    WaveStage::sync();
    double pos[3], w[3], v[3], R[9], fe[3] = {0.0, 0.0, 0.0}, te[3] = {0.0, 0.0, 0.0};
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pos[k] = x[3 + k]; w[k] = x[6 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
    }
    const bool with_ext = a.ext != nullptr;
    if (with_ext) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { fe[k] = E[q * 6 + k]; te[k] = E[q * 6 + 3 + k]; }
    }
    // 0: the plant step's polish of R, I_b^-1 and L
    {
        double E[9], Rp[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[3 * i + j] = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
        E[0] = E[0] - 1.0; E[4] = E[4] - 1.0; E[8] = E[8] - 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rp[3 * i + j] = R[3 * i + j] - 0.5 * ((R[3 * i] * E[j] + R[3 * i + 1] * E[3 + j]) + R[3 * i + 2] * E[6 + j]);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rp[k];
    }
    double Ii[9], L[3];
    {
        const double* I = a.inertia;
        const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
        const double id = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02);
        Ii[0] = c00 * id; Ii[1] = (I[2] * I[7] - I[1] * I[8]) * id; Ii[2] = (I[1] * I[5] - I[2] * I[4]) * id;
        Ii[3] = c01 * id; Ii[4] = (I[0] * I[8] - I[2] * I[6]) * id; Ii[5] = (I[2] * I[3] - I[0] * I[5]) * id;
        Ii[6] = c02 * id; Ii[7] = (I[1] * I[6] - I[0] * I[7]) * id; Ii[8] = (I[0] * I[4] - I[1] * I[3]) * id;
        double wb[3], Iw[3];
        A1_PL_MTV(wb, R, w); A1_PL_MV(Iw, I, wb); A1_PL_MV(L, R, Iw);
    }
    // the swing foot's move over the call: the walk step's
    double d[3] = {0.0, 0.0, 0.0}, vel[3] = {0.0, 0.0, 0.0};
    if (track) {
        double Rz[9], p0[3], tw[3], pt[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rz[k] = ZL[q * 9 + k];
        A1_PL_MTV(p0, R, r); A1_PL_MV(tw, Rz, y); A1_PL_MTV(pt, R, tw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dl = wa.track * (pt[k] - p0[k]);
            d[k] = dl / static_cast<double>(a.substeps); vel[k] = dl / a.dt;
        }
    }
    const double h = a.dt / static_cast<double>(a.substeps), half = h / 2.0, m = a.mass, g = a.gravity;
    for (int step = 0; step < a.substeps; ++step) {
        // 1 .. 6: the walk step's
        double fw[3], F[3], T[3];
        A1_PL_MV(fw, R, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) fw[k] = stance ? fw[k] : 0.0;
        const double tq[3] = {r[1] * fw[2] - r[2] * fw[1], r[2] * fw[0] - r[0] * fw[2], r[0] * fw[1] - r[1] * fw[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            F[k] = pl_legs(fw[k]); T[k] = pl_legs(tq[k]);
            if (with_ext) { F[k] = F[k] + fe[k]; T[k] = T[k] + te[k]; }
        }
        double dp[3];
        v[0] = v[0] + h * (F[0] / m); v[1] = v[1] + h * (F[1] / m); v[2] = v[2] + h * (F[2] / m + g);
#pragma unroll
        for (int k = 0; k < 3; ++k) { dp[k] = h * v[k]; pos[k] = pos[k] + dp[k]; }
        double Rn[9];
        {
            const double a0 = half * w[0], a1 = half * w[1], a2 = half * w[2];
            const double s = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
            const double Cm[9] = {1.0 - s * (a1 * a1 + a2 * a2), s * (a0 * a1 - a2), s * (a0 * a2 + a1),
                                  s * (a0 * a1 + a2), 1.0 - s * (a0 * a0 + a2 * a2), s * (a1 * a2 - a0),
                                  s * (a0 * a2 - a1), s * (a1 * a2 + a0), 1.0 - s * (a0 * a0 + a1 * a1)};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Cm[3 * i] * R[j] + Cm[3 * i + 1] * R[3 + j]) + Cm[3 * i + 2] * R[6 + j];
        }
        {
            double Lb[3], wb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) L[k] = L[k] + h * T[k];
            A1_PL_MTV(Lb, Rn, L); A1_PL_MV(wb, Ii, Lb); A1_PL_MV(w, Rn, wb);
        }
        {
            double rb[3], rs[3];
            A1_PL_MTV(rb, R, r);
            if (track) {
#pragma unroll
                for (int k = 0; k < 3; ++k) rb[k] = rb[k] + d[k];
            }
            A1_PL_MV(rs, Rn, rb);
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = stance ? r[k] - dp[k] : rs[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    }
    // the field, once per call, straight down: the heights under the foot and under the body are gathered together (they depend on pos' and r': the kernel's one exposed
    // memory round trip), each branch holding both calls so that their loads stand side by side.  Then the ground step's rule: a stance foot ON the field under its own x
    // and y, a swing foot not below it; touch: stance, or the comparison that lifted the swing foot (a NaN compares false: the foot keeps its z and touch is 0)
    double ox = 0.0, oy = 0.0, oz = 0.0;
    if (shifted) { ox = GL[q * 3]; oy = GL[q * 3 + 1]; oz = GL[q * 3 + 2]; }   // (the origin's words wait in LDS until here: its image is not written again)
    const double X = pos[0] + r[0], Y = pos[1] + r[1];
    double top, under;
    if (ha.f.interp == 0) { top = hf_sample(ha.f, 0, alive, shifted, ox, oy, oz, X, Y); under = hf_sample(ha.f, 0, alive, shifted, ox, oy, oz, pos[0], pos[1]); }
    else { top = hf_sample(ha.f, 1, alive, shifted, ox, oy, oz, X, Y); under = hf_sample(ha.f, 1, alive, shifted, ox, oy, oz, pos[0], pos[1]); }
    const double gz = top - pos[2];
    const bool lifted = r[2] < gz;
    r[2] = stance ? gz : (lifted ? gz : r[2]);
    const bool touch = stance || lifted;
    const double sp = -R[6], spc = sp > 1.0 ? 1.0 : (sp < -1.0 ? -1.0 : sp);   // (a NaN stays a NaN)
    const double roll = atan2(R[7], R[8]), pitch = asin(spc), yaw = atan2(R[3], R[0]);
    WaveStage::sync();   // (every lane has read its inputs)
    if (alive) {
        double* x = S + q * stride + 3 * l;
        x[0] = pl_pick(l, roll, pos[0], w[0], v[0]); x[1] = pl_pick(l, pitch, pos[1], w[1], v[1]); x[2] = pl_pick(l, yaw, pos[2], w[2], v[2]);
        if (l < 3) {
            double* o = RL + q * 9 + 3 * l;
            o[0] = pl_pick(l, R[0], R[3], R[6], 0.0); o[1] = pl_pick(l, R[1], R[4], R[7], 0.0); o[2] = pl_pick(l, R[2], R[5], R[8], 0.0);
            if (ha.ground_out) ha.ground_out[b * 3 + l] = l == 0 ? under : 0.0;   // the row a1mpc_episode_update_batch takes as `ground`: (height, +0, +0)
        }
        double *fo = a.foot_out + b * 12 + 3 * l, *vo = wa.vel_out + b * 12 + 3 * l;
        fo[0] = r[0]; fo[1] = r[1]; fo[2] = r[2];
        vo[0] = stance ? 0.0 : vel[0]; vo[1] = stance ? 0.0 : vel[1]; vo[2] = stance ? 0.0 : vel[2];
        ha.touch[b * 4 + l] = touch ? uint8_t{1} : uint8_t{0};
    }
    WaveStage::sync();
    double *os = a.state_out + first * stride, *orr = a.R_out + first * 9;
#pragma unroll
    for (int mm = 0; mm < 6; ++mm) {
        const int e = lane + 64 * mm;
        const int col = stride == 12 ? e % 12 : (stride == 13 ? e % 13 : e % 22);
        if (e < cs && col < 12) os[e] = S[e];
    }
#pragma unroll
    for (int mm = 0; mm < 3; ++mm) { const int e = lane + 64 * mm; if (e < cr) orr[e] = RL[e]; }
}

// hf on its own, one point per lane: what places spawn templates on the terrain, and the cheapest place to hold the edge cases of the rule
struct HfSampleArgs {
    HfField f;
    int32_t n;
    const double *xy, *origin;   // origin may be null
    double* out;
};
__global__ __launch_bounds__(64) void a1mpc_heightfield_sample_kernel(const HfSampleArgs a) {
#pragma clang fp contract(off)
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 64 + static_cast<int64_t>(threadIdx.x);
    if (b >= a.n) return;
    const bool shifted = a.origin != nullptr;
    const double X = a.xy[b * 2], Y = a.xy[b * 2 + 1];
    double ox = 0.0, oy = 0.0, oz = 0.0;
    if (shifted) { ox = a.origin[b * 3]; oy = a.origin[b * 3 + 1]; oz = a.origin[b * 3 + 2]; }
    a.out[b] = a.f.interp == 0 ? hf_sample(a.f, 0, true, shifted, ox, oy, oz, X, Y) : hf_sample(a.f, 1, true, shifted, ox, oy, oz, X, Y);
}
#undef A1_PL_MV
#undef A1_PL_MTV

// ---- sensor noise and IMU bias (a1mpc_sensor_noise_batch): white Gaussian noise on the six sensor arrays of the synthesis kernels above, IN PLACE, and a random-walk
// bias on the IMU.  The generator is counter-based: draw j = 0 .. 21 of the robot with global index g at `tick` is Philox4x32-10 on the counter (j, g, tick low, tick
// high) under the key (seed low, seed high), its four words give two uniforms of 52 bits and Box-Muller makes two unit normals z[2j], z[2j + 1] of them; so a robot's 44
// normals are a function of (seed, g, tick) alone, whatever the batch, the robot's place in it and the lane that computes them.  z: [0:3) gyro, [3:6) acc, [6:9) gyro
// bias step, [9:12) acc bias step, [12:15) attitude, [15] unused, [16:28) joint angles, [28:40) joint rates, [40:44) foot forces.
// Lanes: 16 robots per wavefront, four lanes per robot as above.  Lane l computes the draws l, l + 4, ... into the wave's LDS image of z (a draw no channel reads is
// skipped and its two slots hold +0: `draws` is the launcher's mask); then lane l applies leg l's joint and force noise, lanes 0 .. 2 one IMU axis each (bias, gyro,
// acc), lane 3 the quaternion.  A sigma of 0 SELECTS the input (nothing is added: -0 and NaN payloads keep their bits); no FMA contraction, sums left to right
constexpr int kNoiseZ = 44, kNoiseDraws = 22;
struct NoiseArgs {
    int32_t n;
    uint32_t draws;              // bit j: draw j is computed
    uint32_t key0, key1;         // the seed's words
    uint32_t tick_lo, tick_hi;
    uint64_t robot0;             // robot0 + n <= 2^32
    double gyro_sigma, acc_sigma, gyro_walk, acc_walk, att_sigma, jpos_sigma, jvel_sigma, fforce_sigma;   // (a sigma whose array is null arrives as 0)
    double *quat, *acc, *gyro, *jpos, *jvel, *fforce;   // in place; each may be null
    double* bias;                // n x 6 in / out, may be null
    double* z;                   // n x 44, may be null
};
__device__ __forceinline__ void noise_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<uint32_t>(p1); c3 = static_cast<uint32_t>(p0); c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;   // (the bump after the tenth round is not used)
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__global__ __launch_bounds__(64) void a1mpc_sensor_noise_kernel(const NoiseArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double zl[16 * kNoiseZ];
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    const uint32_t g = static_cast<uint32_t>(a.robot0 + static_cast<uint64_t>(b));
    double* const zr = zl + q * kNoiseZ;
    if (alive) {
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            const int j = l + 4 * m;
            if (j >= kNoiseDraws) continue;
            double z0 = 0.0, z1 = 0.0;
            if ((a.draws >> j) & 1u) {   // (the same in every lane of a given l: the mask is the launch's)
                uint32_t x[4];
                noise_philox(static_cast<uint32_t>(j), g, a.tick_lo, a.tick_hi, a.key0, a.key1, x);
                const uint64_t k1 = (static_cast<uint64_t>(x[0] >> 6) << 26) | (x[1] >> 6), k2 = (static_cast<uint64_t>(x[2] >> 6) << 26) | (x[3] >> 6);
                const double u1 = (static_cast<double>(k1) + 0.5) * 0x1p-52, u2 = (static_cast<double>(k2) + 0.5) * 0x1p-52;   // exact, in (0, 1)
                const double r = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
                z0 = r * cos(ang); z1 = r * sin(ang);
            }
            zr[2 * j] = z0; zr[2 * j + 1] = z1;
        }
    }
    WaveStage::sync();
    if (alive) {
        if (a.jpos_sigma != 0.0) {
            double* x = a.jpos + b * 12 + 3 * l;
            const double *z = zr + 16 + 3 * l, v0 = x[0], v1 = x[1], v2 = x[2];
            x[0] = v0 + a.jpos_sigma * z[0]; x[1] = v1 + a.jpos_sigma * z[1]; x[2] = v2 + a.jpos_sigma * z[2];
        }
        if (a.jvel_sigma != 0.0) {
            double* x = a.jvel + b * 12 + 3 * l;
            const double *z = zr + 28 + 3 * l, v0 = x[0], v1 = x[1], v2 = x[2];
            x[0] = v0 + a.jvel_sigma * z[0]; x[1] = v1 + a.jvel_sigma * z[1]; x[2] = v2 + a.jvel_sigma * z[2];
        }
        if (a.fforce_sigma != 0.0) { double* x = a.fforce + b * 4 + l; x[0] = x[0] + a.fforce_sigma * zr[40 + l]; }
        if (l < 3) {
            // one IMU axis: the bias walks first and is stored back, then the sample is (raw + bias) + sigma z; a walk of 0 leaves the bias's bits alone
            double bg = 0.0, ba = 0.0;
            if (a.bias) {
                double* pb = a.bias + b * 6;
                bg = pb[l]; ba = pb[3 + l];
                if (a.gyro_walk != 0.0) { bg = bg + a.gyro_walk * zr[6 + l]; pb[l] = bg; }
                if (a.acc_walk != 0.0) { ba = ba + a.acc_walk * zr[9 + l]; pb[3 + l] = ba; }
            }
            if (a.gyro && (a.bias || a.gyro_sigma != 0.0)) {
                double v = a.gyro[b * 3 + l];
                if (a.bias) v = v + bg;
                if (a.gyro_sigma != 0.0) v = v + a.gyro_sigma * zr[l];
                a.gyro[b * 3 + l] = v;
            }
            if (a.acc && (a.bias || a.acc_sigma != 0.0)) {
                double v = a.acc[b * 3 + l];
                if (a.bias) v = v + ba;
                if (a.acc_sigma != 0.0) v = v + a.acc_sigma * zr[3 + l];
                a.acc[b * 3 + l] = v;
            }
        } else if (a.att_sigma != 0.0) {
            // a small rotation in the body frame: q (x) (1, theta / 2), w first, normalised
            double* pq = a.quat + b * 4;
            const double w = pq[0], x = pq[1], y = pq[2], z = pq[3];
            const double dx = (a.att_sigma * zr[12]) * 0.5, dy = (a.att_sigma * zr[13]) * 0.5, dz = (a.att_sigma * zr[14]) * 0.5;
            const double nw = ((w - x * dx) - y * dy) - z * dz, nx = ((x + w * dx) + y * dz) - z * dy;
            const double ny = ((y + w * dy) + z * dx) - x * dz, nz = ((z + w * dz) + x * dy) - y * dx;
            const double nrm = sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz);
            pq[0] = nw / nrm; pq[1] = nx / nrm; pq[2] = ny / nrm; pq[3] = nz / nrm;
        }
    }
    if (a.z) {
        double* oz = a.z + first * kNoiseZ;
        const int cz = live * kNoiseZ;
#pragma unroll
        for (int m = 0; m < 11; ++m) { const int e = lane + 64 * m; if (e < cz) oz[e] = zl[e]; }
    }
}

thread_local std::string g_last_error;
std::mutex g_cache_mu;
thread_local bool g_clk_ran = false;
thread_local bool g_gen_prefer_one_wave = false;

// ---- episode record and batch summary (a1mpc_episode_update_batch, a1mpc_episode_summary_batch): what happened to each robot of a closed loop, kept on the device.  A
// record is 16 doubles per robot, owned by the caller, all zero at the start of an episode: ticks, end_tick_p1, end_code, vel_err_sum, height_err_sum, tilt_max,
// est_pos_err_sum, est_vel_err_sum, est_vel_err_max, effort_sum, fz_max, solver_bad, reach_bad, x0, y0, dist2 (the rules: include/a1mpc.h, restated elementwise in
// tests/episode_ref.py).  The section sits behind the span the host emulations of the plant family compile; it uses that span's WaveStage, pl_legs and pl_pick.
//   update    the plant kernels' layout: 16 robots per one-wave workgroup, lane = 4 robot + leg, every load issued up front, a robot's rows (state, R, the estimate, the
//             commands, its plane, its record) through wave-private LDS; a lane loads its own leg's force, contact and reach byte.  Every lane of a robot computes the
//             robot's whole new record (the leg sums are pl_legs, (leg 0 + leg 1) + (leg 2 + leg 3)), lane l parks words 4 l .. 4 l + 3 in the LDS image and the image
//             leaves with 64 consecutive doubles per instruction.  Selects, no branches on data; IEEE + - * and comparisons only, no contraction
//   reduce    one lane per row, 64 consecutive rows per one-wave workgroup, the rows through an LDS tile; a row becomes the 20 words of a summary (of itself), the xor
//             butterfly 1, 2, 4 .. 32 combines them and lane 0 writes one partial summary.  The same kernel then reduces the partials, level by level, each level a
//             launch: no atomics, nothing waits on another workgroup.  A sum is the balanced tree over the column padded with +0; dead lanes carry +0 in the sums and a
//             copy of the wave's first row in the maxima, which changes neither
constexpr int kEpWords = 16, kEpSummary = 20;
struct EpisodeArgs {
    int32_t n, stride;
    double min_up, min_height;
    double tick_p1;              // tick + 1, exact
    const double *state, *R;
    const double *est_pos, *est_vel;   // both or neither
    const double *cmd, *pos_d_z, *ground;   // each may be null
    const double* grf;           // with contacts, or both null
    const uint8_t *contacts, *reach;
    const int32_t* status;
    double* episode;
};
__device__ __forceinline__ bool ep_finite(double x) { return x - x == 0.0; }   // (an infinity or a NaN gives a NaN)
__global__ __launch_bounds__(64) void a1mpc_episode_update_kernel(const EpisodeArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double elds[kPlState + kPlR + 16 * kEpWords + 4 * 48 + 16];
    double* const S = elds; double* const RL = S + kPlState; double* const EP = RL + kPlR; double* const PL = EP + 16 * kEpWords; double* const VL = PL + 48;
    double* const CL = VL + 48; double* const GL = CL + 48; double* const ZL = GL + 48;
    const int lane = static_cast<int>(threadIdx.x), qw = lane >> 2, l = lane & 3, stride = a.stride;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    if (first >= a.n) return;   // (whole wave)
    const int live = static_cast<int>(a.n - first < 16 ? a.n - first : 16);
    const bool alive = qw < live;
    const int q = alive ? qw : 0;
    const int64_t b = first + q;
    const bool with_est = a.est_pos != nullptr, with_cmd = a.cmd != nullptr, with_z = a.pos_d_z != nullptr, sloped = a.ground != nullptr, with_f = a.grf != nullptr;
    // every load, then the LDS writes, as in the plant step; the three-word rows are 48 words at most: one load per lane each
    const int cs = live * stride, cr = live * 9, cw = live * kEpWords, c3 = live * 3;
    const int cp = with_est ? c3 : 0, cc = with_cmd ? c3 : 0, cg = sloped ? c3 : 0, cz = with_z ? live : 0;
    const double *gs = a.state + first * stride, *gr = a.R + first * 9;
    double* const gw = a.episode + first * kEpWords;
    const double *gp = with_est ? a.est_pos + first * 3 : a.R, *gv = with_est ? a.est_vel + first * 3 : a.R, *gc = with_cmd ? a.cmd + first * 3 : a.R;
    const double *gg = sloped ? a.ground + first * 3 : a.R, *gz = with_z ? a.pos_d_z + first : a.R;
    double vs[6], vr[3], vw[4];
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; vs[m] = gs[e < cs ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; vr[m] = gr[e < cr ? e : 0]; }
#pragma unroll
    for (int m = 0; m < 4; ++m) { const int e = lane + 64 * m; vw[m] = gw[e < cw ? e : 0]; }
    const double vp = gp[lane < cp ? lane : 0], vv = gv[lane < cp ? lane : 0], vc = gc[lane < cc ? lane : 0], vg = gg[lane < cg ? lane : 0], vz = gz[lane < cz ? lane : 0];
    double f[3] = {0.0, 0.0, 0.0};
    bool stance = false, unreached = false;
    if (with_f) {
        const double* fp = a.grf + b * 12 + 3 * l;
        f[0] = fp[0]; f[1] = fp[1]; f[2] = fp[2];
        stance = a.contacts[b * 4 + l] != 0;
    }
    if (a.reach) unreached = a.reach[b * 4 + l] != 0;
    const bool solved = a.status ? a.status[b] == 1 : true;
#pragma unroll
    for (int m = 0; m < 6; ++m) { const int e = lane + 64 * m; if (e < cs) S[e] = vs[m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { const int e = lane + 64 * m; if (e < cr) RL[e] = vr[m]; }
#pragma unroll
    for (int m = 0; m < 4; ++m) { const int e = lane + 64 * m; if (e < cw) EP[e] = vw[m]; }
    if (lane < cp) { PL[lane] = vp; VL[lane] = vv; }
    if (lane < cc) CL[lane] = vc;
    if (lane < cg) GL[lane] = vg;
    if (lane < cz) ZL[lane] = vz;
    WaveStage::sync();
    double pos[3], v[3], R[9], w[kEpWords];
    {
        const double* x = S + q * stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pos[k] = x[3 + k]; v[k] = x[9 + k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = RL[q * 9 + k];
#pragma unroll
        for (int k = 0; k < kEpWords; ++k) w[k] = EP[q * kEpWords + k];
    }
    // 2: the non-finite test over what this robot's rules read (a swing leg's force is selected away, not tested)
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) fin = fin && ep_finite(pos[k]) && ep_finite(v[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && ep_finite(R[k]);
    double ep[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0}, c0 = 0.0, c1 = 0.0, pdz = 0.0, hz = 0.0;
    if (with_est) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { ep[k] = PL[q * 3 + k]; ev[k] = VL[q * 3 + k]; fin = fin && ep_finite(ep[k]) && ep_finite(ev[k]); }
    }
    if (with_cmd) { c0 = CL[q * 3]; c1 = CL[q * 3 + 1]; fin = fin && ep_finite(c0) && ep_finite(c1); }
    if (with_z) { pdz = ZL[q]; fin = fin && ep_finite(pdz); }
    if (sloped) {
        const double z0 = GL[q * 3], sx = GL[q * 3 + 1], sy = GL[q * 3 + 2];
        fin = fin && ep_finite(z0) && ep_finite(sx) && ep_finite(sy);
        hz = (z0 + sx * pos[0]) + sy * pos[1];
    }
    if (with_f) {
        const bool leg_ok = !stance || (ep_finite(f[0]) && ep_finite(f[1]) && ep_finite(f[2]));
        const double bad_legs = pl_legs(leg_ok ? 0.0 : 1.0);   // (every lane shuffles: not behind the && below)
        fin = fin && bad_legs == 0.0;
    }
    // 1, 3, 4: frozen, or ended by this update, or accumulated
    const double height = pos[2] - hz;
    const int code = !fin ? 1 : (R[8] < a.min_up ? 2 : (height < a.min_height ? 3 : 0));
    const bool frozen = w[2] != 0.0, ends = !frozen && code != 0, acc = !frozen && code == 0;
    double nw[kEpWords];
#pragma unroll
    for (int k = 0; k < kEpWords; ++k) nw[k] = w[k];
    nw[1] = ends ? a.tick_p1 : w[1];
    nw[2] = ends ? static_cast<double>(code) : w[2];
    // 5: every word whose inputs are given
    nw[0] = acc ? w[0] + 1.0 : w[0];
    if (with_cmd) {
        const double ex = ((R[0] * v[0] + R[3] * v[1]) + R[6] * v[2]) - c0, ey = ((R[1] * v[0] + R[4] * v[1]) + R[7] * v[2]) - c1;
        nw[3] = acc ? w[3] + (ex * ex + ey * ey) : w[3];
    }
    if (with_z) { const double ez = height - pdz; nw[4] = acc ? w[4] + ez * ez : w[4]; }
    { const double t = 1.0 - R[8]; nw[5] = acc ? (t > w[5] ? t : w[5]) : w[5]; }
    if (with_est) {
        const double dx = ep[0] - pos[0], dy = ep[1] - pos[1], dz = ep[2] - pos[2], ux = ev[0] - v[0], uy = ev[1] - v[1], uz = ev[2] - v[2];
        const double tp = (dx * dx + dy * dy) + dz * dz, tv = (ux * ux + uy * uy) + uz * uz;
        nw[6] = acc ? w[6] + tp : w[6]; nw[7] = acc ? w[7] + tv : w[7]; nw[8] = acc ? (tv > w[8] ? tv : w[8]) : w[8];
    }
    if (with_f) {
        const double sl = stance ? (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] : 0.0;
        const double effort = pl_legs(sl);
        // the largest stance fz of the robot: a swing leg offers the record's own maximum, so the four-lane maximum is the rule's, leg by leg
        double fz = stance ? (f[2] > w[10] ? f[2] : w[10]) : w[10];
        { const double o = __shfl_xor(fz, 1, 64); fz = o > fz ? o : fz; }
        { const double o = __shfl_xor(fz, 2, 64); fz = o > fz ? o : fz; }
        nw[9] = acc ? w[9] + effort : w[9]; nw[10] = acc ? fz : w[10];
    }
    if (a.status) nw[11] = (acc && !solved) ? w[11] + 1.0 : w[11];
    if (a.reach) { const double legs = pl_legs(unreached ? 1.0 : 0.0); nw[12] = acc ? w[12] + legs : w[12]; }
    {
        const bool opens = acc && w[0] == 0.0;
        nw[13] = opens ? pos[0] : w[13]; nw[14] = opens ? pos[1] : w[14];
        const double dx = pos[0] - nw[13], dy = pos[1] - nw[14];
        nw[15] = acc ? dx * dx + dy * dy : w[15];
    }
    WaveStage::sync();   // (every lane has read its robot's record)
    if (alive) {
        double* o = EP + q * kEpWords + 4 * l;
        o[0] = pl_pick(l, nw[0], nw[4], nw[8], nw[12]); o[1] = pl_pick(l, nw[1], nw[5], nw[9], nw[13]);
        o[2] = pl_pick(l, nw[2], nw[6], nw[10], nw[14]); o[3] = pl_pick(l, nw[3], nw[7], nw[11], nw[15]);
    }
    WaveStage::sync();
#pragma unroll
    for (int m = 0; m < 4; ++m) { const int e = lane + 64 * m; if (e < cw) gw[e] = EP[e]; }
}

// n rows -> ceil(n / 64) partial summaries; rows are records (`records`) or partial summaries of the level below.  Words of a summary: 0 rows, 1 .. 4 rows with end_code
// 0 / 1 / 2 / 3, 5 the smallest end_tick_p1 of an ended row (0: none; the last level writes it minus 1), 6 .. 8, 11, 12, 14, 16 .. 18 sums, 9 / 10 the largest tilt_max
// and the lowest row that has it, 13, 15, 19 maxima
struct EpisodeReduceArgs {
    const double* in;
    double* out;
    int64_t rows;
    int32_t records, last;
};
constexpr uint32_t kEpSums = 0x1F | (7u << 6) | (3u << 11) | (1u << 14) | (7u << 16), kEpMaxs = (1u << 13) | (1u << 15) | (1u << 19);
__global__ __launch_bounds__(64) void a1mpc_episode_reduce_kernel(const EpisodeReduceArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double tile[64 * kEpSummary];
    const int lane = static_cast<int>(threadIdx.x);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 64;
    if (first >= a.rows) return;   // (whole wave)
    const int live = static_cast<int>(a.rows - first < 64 ? a.rows - first : 64);
    const bool alive = lane < live, rec = a.records != 0;
    const int width = rec ? kEpWords : kEpSummary, cnt = live * width;
    const double* g = a.in + first * width;
    double vt[kEpSummary];
#pragma unroll
    for (int m = 0; m < kEpSummary; ++m) { const int e = lane + 64 * m; vt[m] = g[e < cnt ? e : 0]; }
    // a record row takes 17 words of the tile (64 x 17 <= 64 x 20): lanes that read their rows 16 words apart would all meet in two banks
#pragma unroll
    for (int m = 0; m < kEpSummary; ++m) { const int e = lane + 64 * m; if (e < cnt) tile[rec ? e + (e >> 4) : e] = vt[m]; }
    WaveStage::sync();
    const int src = alive ? lane : 0;   // (a dead lane: the wave's first row in the maxima, +0 in the sums)
    const double* r = tile + src * (rec ? kEpWords + 1 : kEpSummary);
    double v[kEpSummary];
    if (rec) {
        const double c = r[2];
        v[0] = 1.0; v[1] = c == 0.0 ? 1.0 : 0.0; v[2] = c == 1.0 ? 1.0 : 0.0; v[3] = c == 2.0 ? 1.0 : 0.0; v[4] = c == 3.0 ? 1.0 : 0.0;
        v[5] = c != 0.0 ? r[1] : 0.0;
        v[6] = r[0]; v[7] = r[3]; v[8] = r[4]; v[9] = r[5]; v[10] = static_cast<double>(first + src); v[11] = r[6]; v[12] = r[7]; v[13] = r[8]; v[14] = r[9]; v[15] = r[10];
        v[16] = r[11]; v[17] = r[12]; v[18] = r[15]; v[19] = r[15];
    } else {
#pragma unroll
        for (int k = 0; k < kEpSummary; ++k) v[k] = r[k];
    }
#pragma unroll
    for (int k = 0; k < kEpSummary; ++k)
        if (((kEpSums >> k) & 1u) || k == 5) v[k] = alive ? v[k] : 0.0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const double om = __shfl_xor(v[9], s, 64), orow = __shfl_xor(v[10], s, 64), oe = __shfl_xor(v[5], s, 64);
#pragma unroll
        for (int k = 0; k < kEpSummary; ++k) {
            if ((kEpSums >> k) & 1u) v[k] = v[k] + __shfl_xor(v[k], s, 64);
            else if ((kEpMaxs >> k) & 1u) { const double o = __shfl_xor(v[k], s, 64); v[k] = o > v[k] ? o : v[k]; }
        }
        const bool take = om > v[9] || (om == v[9] && orow < v[10]);
        v[9] = take ? om : v[9]; v[10] = take ? orow : v[10];
        v[5] = v[5] == 0.0 ? oe : (oe == 0.0 ? v[5] : (oe < v[5] ? oe : v[5]));
    }
    if (lane == 0) {
        double* o = a.out + static_cast<int64_t>(blockIdx.x) * kEpSummary;
#pragma unroll
        for (int k = 0; k < kEpSummary; ++k) o[k] = k == 5 && a.last ? v[5] - 1.0 : v[k];
    }
}

// ---- the launch layer's table (a1mpc_common.hpp): (kernel, device) -> resident workgroups.  An entry exists once the kernel's dynamic-LDS limit is set on that device
// and holds 0 until its occupancy has been asked for.  One mutex: handles of different threads may launch at the same time
static std::mutex g_kernel_mu;
static std::map<std::pair<const void*, int>, int> g_kernels;
static a1mpc_status kernel_entry(int dev, const void* fn, size_t lds, int** resident) {   // (g_kernel_mu held)
    auto it = g_kernels.find({fn, dev});
    if (it == g_kernels.end()) {
        A1_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        it = g_kernels.emplace(std::make_pair(fn, dev), 0).first;
    }
    *resident = &it->second;
    return A1MPC_OK;
}
a1mpc_status set_lds_attr(int dev, const void* fn, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_kernel_mu);
    int* resident = nullptr;
    return kernel_entry(dev, fn, bytes, &resident);
}
a1mpc_status resident_workgroups(int dev, const void* fn, int threads, size_t lds, int* out) {
    std::lock_guard<std::mutex> lock(g_kernel_mu);
    int* resident = nullptr;
    if (a1mpc_status st = kernel_entry(dev, fn, lds, &resident); st != A1MPC_OK) return st;
    if (!*resident) {
        int per_cu = 0, cus = 0;
        A1_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds));
        A1_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        *resident = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
    }
    *out = *resident;
    return A1MPC_OK;
}

// ---- respawn (a1mpc_respawn_reset_batch, a1mpc_respawn_batch, a1mpc_respawn_rows_device): a robot whose episode is over gets its lane back on the device.  Two
// kernels in a section of their own, behind every span a host emulation of another family compiles; neither knows a struct of the handle: the launcher hands the first
// a table of regions (where a robot's bytes of each state block lie), the second the caller's table of rows.  The rules: include/a1mpc.h, restated in
// tests/respawn_ref.py; the text below is compiled for the host by tests/emu/respawn_host.py.
//   both      one wavefront owns 64 consecutive robots: lane l decides robot l (its mask byte, or rules 1 - 3 on its record and life), one ballot gives the wave's set,
//             and a wave-uniform loop takes the set's robots one by one with all 64 lanes on that robot's words: consecutive lanes, consecutive words.  A wave with an
//             empty set has read one byte (the decision: 24) per robot and leaves.  Plain stores; no LDS, no atomics, nothing waits on another wavefront
//   region    `runs` runs of `run_bytes` at `run_step` bytes from each other, `robot_stride` bytes between two robots.  A block that is contiguous per robot is one
//             run (lane = word); a block that holds one word per slot and robot, [slot][max_batch], is `runs` runs of one word (lane = slot).  The launcher builds no
//             other shape.  Words are 8 bytes unless run_bytes is an odd multiple of 4 (the IMU count / cursor)
//   decision  copies, comparisons and integer arithmetic: no floating-point operation rounds
constexpr int kRespawnRegions = 10, kRespawnWords = 16, kRespawnRowsMax = 16;
struct RespawnRegion { char* base; int64_t robot_stride, run_step; int32_t run_bytes, runs; };
struct RespawnArgs {
    int32_t n, n_regions;
    const uint8_t* mask;         // given (a1mpc_respawn_reset_batch): bit 0 selects, nothing below is read; or null: the rules
    double* record;              // n x 16, in / out
    int32_t* life;               // n x 2, in / out: hold, episodes_done
    double* finished;            // n x 16 or null
    uint8_t* mask_out;           // n
    uint32_t codes;
    int32_t hold_ticks;
    double max_ticks;            // exact (below 2^53); 0: no limit
    RespawnRegion region[kRespawnRegions];
};
__global__ __launch_bounds__(64) void a1mpc_respawn_kernel(const RespawnArgs a) {
    const int lane = static_cast<int>(threadIdx.x);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 64;
    if (first >= a.n) return;   // (whole wave)
    const int64_t b = first + lane;
    const bool alive = b < a.n;
    int m = 0;
    if (a.mask) {
        if (alive) m = a.mask[b] & 1;
    } else if (alive) {
        const int hold = a.life[2 * b], done = a.life[2 * b + 1];
        const double ticks = a.record[b * kRespawnWords], code = a.record[b * kRespawnWords + 2];
        const bool ended = (code == 1.0 && (a.codes & 2u)) || (code == 2.0 && (a.codes & 4u)) || (code == 3.0 && (a.codes & 8u));
        const bool timed = code == 0.0 && a.max_ticks > 0.0 && ticks >= a.max_ticks;
        m = hold > 0 ? 2 : (ended || timed ? 1 : 0);
        a.mask_out[b] = static_cast<uint8_t>(m);
        if (m == 2) a.life[2 * b] = hold - 1;
        if (m == 1) { a.life[2 * b] = a.hold_ticks; a.life[2 * b + 1] = done + 1; }
    }
    const unsigned long long reset = __ballot(m == 1);
    if (!a.mask) {   // the records of the respawned and the held: 16 lanes on a record
        const unsigned long long cleared = __ballot(m != 0);
        for (unsigned long long set = cleared; set != 0; set &= set - 1) {
            const int r = __builtin_ctzll(set);
            double* const rec = a.record + (first + r) * kRespawnWords;
            if (lane < kRespawnWords) {
                if (((reset >> r) & 1) && a.finished) a.finished[(first + r) * kRespawnWords + lane] = rec[lane];
                rec[lane] = 0.0;
            }
        }
    }
    for (unsigned long long set = reset; set != 0; set &= set - 1) {
        const int64_t rb = first + __builtin_ctzll(set);
        for (int k = 0; k < a.n_regions; ++k) {
            const RespawnRegion& g = a.region[k];
            const bool slots = g.runs > 1, narrow = (g.run_bytes & 7) != 0;
            const int word = narrow ? 4 : 8;
            const int count = slots ? g.runs : g.run_bytes / word;
            const int64_t step = slots ? g.run_step : word;
            char* const p = g.base + rb * g.robot_stride;
            if (narrow) { for (int e = lane; e < count; e += 64) *reinterpret_cast<uint32_t*>(p + e * step) = 0u; }
            else { for (int e = lane; e < count; e += 64) *reinterpret_cast<unsigned long long*>(p + e * step) = 0ull; }
        }
    }
}

// rows: robot b's row of dst becomes the template's (src_rows 1: row 0; else row b) where its mask value selects the entry -- `when` bit 0 on mask 1, bit 1 on mask 2
struct RespawnRow { char* dst; const char* src; int32_t row_bytes, broadcast, when, wide; };   // wide: row_bytes and both pointers are multiples of 8
struct RespawnRowsArgs {
    int32_t n, n_rows;
    const uint8_t* mask;
    RespawnRow row[kRespawnRowsMax];
};
__global__ __launch_bounds__(64) void a1mpc_respawn_rows_kernel(const RespawnRowsArgs a) {
    const int lane = static_cast<int>(threadIdx.x);
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 64;
    if (first >= a.n) return;   // (whole wave)
    const int m = first + lane < a.n ? a.mask[first + lane] : 0;
    const unsigned long long on1 = __ballot(m == 1), on2 = __ballot(m == 2);
    if ((on1 | on2) == 0) return;
    for (int k = 0; k < a.n_rows; ++k) {
        const RespawnRow& g = a.row[k];
        const unsigned long long sel = ((g.when & 1) ? on1 : 0ull) | ((g.when & 2) ? on2 : 0ull);
        for (unsigned long long set = sel; set != 0; set &= set - 1) {
            const int64_t rb = first + __builtin_ctzll(set);
            char* const d = g.dst + rb * g.row_bytes;
            const char* const s = g.src + (g.broadcast ? 0 : rb * g.row_bytes);
            if (g.wide) {
                const int count = g.row_bytes >> 3;
                for (int e = lane; e < count; e += 64) reinterpret_cast<unsigned long long*>(d)[e] = reinterpret_cast<const unsigned long long*>(s)[e];
            } else {
                for (int e = lane; e < g.row_bytes; e += 64) d[e] = s[e];
            }
        }
    }
}

// ---- what a horizon compiled in has: its record sizes and the entry points of its a1mpc_k_*.hip units
struct HorizonOps {
    int horizon;
    size_t carry_stride;   // doubles per QP of the update path's carry (0 at horizon 1: the update path does not apply -- warm_start = 2 behaves like 1)
    size_t prep_stride, prep_stride_gen;   // ... of the hand-off records of the two split pipelines
    Geometry (*admm_geometry)();   // of the persistent ADMM kernel large batches run (a1mpc_kernel_info)
    a1mpc_status (*launch_split)(const KernelArgs&, double*, int*, hipStream_t, hipEvent_t);
    a1mpc_status (*resident_rows)(int*);
    a1mpc_status (*launch)(const KernelArgs&, hipStream_t);
    // the general path (every multi-step horizon; gen_qps = QPs per wavefront of its kernels, 0 = none).  LDS per QP (round 6: the per-step bounds left the image): 22.7 KB
    // (H = 10: six QPs per CU in one-wave workgroups, seven in the CU-wide persistent kernel), 35.9 KB (H = 16: four, one per wavefront like the fast path's), 44.7 KB (H = 20:
    // three, one row per workgroup) -- which also leaves 13 / 26 KB of a CU's LDS free at H = 16 / 20: the set-up kernel of a second batch in flight (11.7 / 15.7 KB per
    // workgroup) now runs BESIDE the persistent kernel instead of behind it (profiles/r06_general_pipeline.md)
    int gen_qps;
    a1mpc_status (*resident_workgroups_gen)(int*);
    a1mpc_status (*launch_gen_split)(const KernelArgs&, double*, int*, hipStream_t, hipEvent_t);
    a1mpc_status (*launch_gen)(const KernelArgs&, hipStream_t);
};
template <int H>
static HorizonOps fast_ops() {
    size_t carry = 0;
    if constexpr (H > 1) carry = Carry<H>::STRIDE;
    return {H, carry, Prep<H>::STRIDE, 0, &admm_geometry<H>, &launch_split<H>, &resident_rows<H>, &launch<H, kModeMpc>, 0, nullptr, nullptr, nullptr};
}
template <int H, int R>
static void add_gen_ops(HorizonOps* o) {
    o->prep_stride_gen = Prep<H>::STRIDE_GEN; o->gen_qps = R;
    o->resident_workgroups_gen = &resident_workgroups_gen<H, R>; o->launch_gen_split = &launch_gen_split_rows<H, R>; o->launch_gen = &launch_gen_rows<H, R>;
}
static std::vector<HorizonOps> horizon_table() {
    std::vector<HorizonOps> t;
    const auto at = [&t](int h) { for (HorizonOps& o : t) if (o.horizon == h) return &o; return static_cast<HorizonOps*>(nullptr); };
#define A1_FAST_OPS(H) t.push_back(fast_ops<H>());
    A1MPC_FAST_HORIZONS(A1_FAST_OPS)
#undef A1_FAST_OPS
#define A1_GEN_OPS(H, R) add_gen_ops<H, R>(at(H));
    A1MPC_GEN_HORIZONS(A1_GEN_OPS)
#undef A1_GEN_OPS
    return t;
}
static const HorizonOps* ops_of(int horizon) {   // null: a horizon that is not compiled in
    static const std::vector<HorizonOps> table = horizon_table();
    for (const HorizonOps& o : table) if (o.horizon == horizon) return &o;
    return nullptr;
}
static size_t carry_stride(int horizon) { const HorizonOps* o = ops_of(horizon); return o ? o->carry_stride : 0; }
static a1mpc_status no_general_path() { return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "per-step feet (foot_stride = 12) and a separate A_c yaw need a horizon > 1"); }
// rows of the general path's ADMM kernel that are resident at once (0: horizon without a general path)
static a1mpc_status resident_rows_gen(const HorizonOps& o, int* rows) {
    int wg = 0;
    *rows = 0;
    if (!o.gen_qps) return A1MPC_OK;
    const a1mpc_status st = o.resident_workgroups_gen(&wg);
    *rows = o.gen_qps * wg;
    return st;
}

static bool warm_fused_enabled() {
    static const bool on = [] { const char* e = getenv("A1MPC_WARM_FUSED"); return !(e && !strcmp(e, "0")); }();
    return on;
}
// largest warm-started batch that runs the fused kernel (see solve_device_impl): measured crossovers, in QPs
static int warm_fused_max(int horizon) {
    static const int over = [] { const char* e = getenv("A1MPC_WARM_FUSED_MAX"); return e ? atoi(e) : 0; }();
    if (over > 0) return over;
    return horizon == 10 ? 8192 : (horizon == 20 ? 2048 : 0);   // (h = 16 / 20 with the fused kernel's quads of rows: profiles/r04_warm_ticks_h16_h20_fused_vs_split.txt -- 2048 x h20
                                                                 // 0.72 -> 0.63 ms per tick; from 4096 on, and at h = 16 everywhere, the split pipeline's denser residency wins)
}
static constexpr int kScheduleMinBatch = 1024;  // below this every QP is resident at once and the order cannot matter

// does a batch of n QPs go through the split pipeline?
static a1mpc_status use_split_pipeline(const HorizonOps& o, int n, bool have_prep, bool* split) {
    *split = false;
    if (!have_prep || pipeline_mode() == 2) return A1MPC_OK;
    if (pipeline_mode() == 1) { *split = true; return A1MPC_OK; }
    int rows = 0;
    const a1mpc_status st = o.resident_rows(&rows);
    *split = n > rows;
    return st;
}

static bool fused_queue_enabled() {
    static const bool on = [] { const char* e = getenv("A1MPC_FUSED_QUEUE"); return e && !strcmp(e, "1"); }();
    return on;
}
static a1mpc_status launch_mpc(const HorizonOps& o, const KernelArgs& a, double* prep, int* counter, hipStream_t s, bool split, hipEvent_t mid) {
    RoctxRange range(split ? "a1mpc solve (split pipeline)" : "a1mpc solve (fused)");
    if (split && counter && o.horizon == 10 && fused_queue_enabled() && a.carry == nullptr && a.clk == nullptr) {
        if (mid) A1_HIP(hipEventRecord(mid, s));
        return launch_fused_queue(a, counter, s);
    }
    if (split && prep && counter) return o.launch_split(a, prep, counter, s, mid);
    return o.launch(a, s);
}

static void to_device_params(const a1mpc_config& c, DeviceParams* p) {
    std::memset(p, 0, sizeof *p);
    p->dt = c.dt; p->mu = c.mu; p->fz_min = c.fz_min; p->fz_max = c.fz_max;
    for (int i = 0; i < 12; ++i) { p->q2[i] = 2.0 * c.q[i]; p->r2[i] = 2.0 * c.r[i]; }  // S/ConvexMpc.cpp:20,41
    p->mass = c.mass;
    for (int i = 0; i < 9; ++i) p->inertia[i] = c.inertia_body[i];
    p->rho0 = c.rho; p->sigma = c.sigma; p->alpha = c.alpha; p->eps_abs = c.eps_abs; p->eps_rel = c.eps_rel;
    p->adaptive_rho_tol = c.adaptive_rho_tolerance;
    p->max_iter = c.max_iter; p->check_every = c.check_termination; p->adaptive_rho = c.adaptive_rho;
    // adaptive_rho_interval = 0 is OSQP's default "automatic" (what the reference actually runs, S/A1RobotControl.cpp:523-524): OSQP fixes the
    // interval in its first solve to c_max(c_roundmultiple(iter, check_termination), check_termination), iter = the iteration at which
    // 0.4 x setup_time of WALL CLOCK has passed (osqp.c, PROFILING).  That rule is evaluated here with the outcome it has whenever 0.4 x setup_time
    // is worth fewer than 1.5 x check_termination iterations (true for these QP sizes on the CPUs the reference runs on): check_termination.
    // Its other possible outcomes (50, 75, ...) are selected by passing that number.
    p->adaptive_rho_every = c.adaptive_rho_interval > 0 ? c.adaptive_rho_interval : (c.check_termination > 0 ? c.check_termination : 25);
    p->scaling_iters = c.scaling; p->warm_start = c.warm_start;
}

// Which configurations the engine accepts (a13).  OSQP validates its data and settings in osqp_setup (auxil.c validate_data: every l_i <= u_i;
// validate_settings: rho, sigma > 0, 0 < alpha < 2, eps >= 0, max_iter > 0, scaling >= 0, adaptive_rho_tolerance >= 1, ...) and refuses to set up otherwise; the
// reference never looks at the outcome (S/A1RobotControl.cpp:532,540) and then "solves" on an uninitialised workspace.  Here the same conditions are a loud
// A1MPC_ERR_INVALID_ARGUMENT at a1mpc_create / a1mpc_update_config / a1mpc_balance_solve_batch.  On everything that passes, the QP family is feasible and bounded:
//   * 0 <= mu, fz_min <= fz_max, fz_max >= 0: per leg and step (0, 0, max(fz_min, 0) c) satisfies the pyramid and the box (c = the contact flag) -- never primal infeasible;
//   * the box and the pyramid bound every force by fz_max (1 + mu) -- the feasible set is compact, so the cost is bounded below whatever the weights: never dual infeasible;
//   * q >= 0, r >= 0 (finite): P = B'QB + R is positive semi-definite -- never OSQP_NON_CVX from the data (the status remains for non-finite INPUTS).
// Hence OSQP's statuses -3 / 3 (primal infeasible) and -4 / 4 (dual infeasible) have no exact certificate on any accepted configuration and the kernels do not evaluate
// the approximate certificate tests (auxil.c is_primal_infeasible / is_dual_infeasible); the oracle does evaluate them, and over every QP the suites compare (> 2 M) it never reported one.
static bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}
static const char* invalid_config(const a1mpc_config& c) {
    if (!std::isfinite(c.dt) || !(c.dt > 0)) return "dt must be positive and finite";
    if (!std::isfinite(c.mass) || !(c.mass > 0)) return "mass must be positive and finite";
    if (!std::isfinite(c.mu) || c.mu < 0) return "mu must be >= 0 and finite (a negative friction coefficient collapses the pyramid to the zero force, and to the empty set -- primal infeasible -- when fz_min > 0)";
    if (!std::isfinite(c.fz_min) || !std::isfinite(c.fz_max)) return "fz_min / fz_max must be finite";
    if (c.fz_min > c.fz_max) return "fz_min > fz_max: OSQP's validate_data refuses l > u (the problem would be primal infeasible)";
    if (c.fz_max < 0) return "fz_max < 0: a stance leg would need fz <= fz_max < 0 inside a pyramid that asks fz >= 0 (primal infeasible)";
    if (!all_finite(c.q, A1MPC_STATE_DIM) || !all_finite(c.r, A1MPC_NUM_DOF)) return "q / r weights must be finite";
    for (int i = 0; i < A1MPC_STATE_DIM; ++i) if (c.q[i] < 0) return "q weights must be >= 0 (a negative weight makes the Hessian indefinite: OSQP_NON_CVX)";
    for (int i = 0; i < A1MPC_NUM_DOF; ++i) if (c.r[i] < 0) return "r weights must be >= 0 (a negative weight makes the Hessian indefinite: OSQP_NON_CVX)";
    if (!all_finite(c.inertia_body, 9)) return "inertia_body must be finite";
    {   // the body inertia is inverted (S/ConvexMpc.cpp:136-141): it must be invertible
        const double* I = c.inertia_body;
        const double det = I[0] * (I[4] * I[8] - I[5] * I[7]) - I[1] * (I[3] * I[8] - I[5] * I[6]) + I[2] * (I[3] * I[7] - I[4] * I[6]);
        if (!(std::fabs(det) > 0)) return "inertia_body must be invertible";
    }
    // osqp auxil.c validate_settings
    if (!std::isfinite(c.rho) || !(c.rho > 0)) return "rho must be positive";
    if (!std::isfinite(c.sigma) || !(c.sigma > 0)) return "sigma must be positive";
    if (!std::isfinite(c.alpha) || !(c.alpha > 0) || !(c.alpha < 2)) return "alpha must lie in (0, 2)";
    if (!std::isfinite(c.eps_abs) || !std::isfinite(c.eps_rel) || c.eps_abs < 0 || c.eps_rel < 0) return "eps_abs / eps_rel must be >= 0 and finite";
    if (c.eps_abs == 0 && c.eps_rel == 0) return "eps_abs and eps_rel must not both be zero";
    if (c.max_iter <= 0) return "max_iter must be positive";
    if (c.check_termination < 0) return "check_termination must be >= 0";
    if (c.scaling < 0) return "scaling must be >= 0";
    if (c.adaptive_rho != 0 && c.adaptive_rho != 1) return "adaptive_rho must be 0 or 1";
    if (c.adaptive_rho_interval < 0) return "adaptive_rho_interval must be >= 0";
    if (c.adaptive_rho && (!std::isfinite(c.adaptive_rho_tolerance) || c.adaptive_rho_tolerance < 1.0)) return "adaptive_rho_tolerance must be >= 1";
    if (c.warm_start < 0 || c.warm_start > 2) return "warm_start must be 0, 1 or 2";
    return nullptr;
}
static const char* invalid_balance_config(const a1mpc_balance_config& q) {
    if (!all_finite(q.Q, 6) || !std::isfinite(q.R) || !std::isfinite(q.mu) || !std::isfinite(q.F_min) || !std::isfinite(q.F_max)) return "balance-QP constants must be finite";
    for (int i = 0; i < 6; ++i) if (q.Q[i] < 0) return "balance-QP weights Q must be >= 0";
    if (q.R < 0) return "balance-QP weight R must be >= 0";
    if (q.mu < 0) return "balance-QP mu must be >= 0";
    if (q.F_min > q.F_max) return "balance-QP F_min > F_max (primal infeasible; OSQP's validate_data refuses l > u)";
    if (q.F_max < 0) return "balance-QP F_max < 0 (primal infeasible)";
    return nullptr;
}

}  // namespace a1mpc

using namespace a1mpc;

struct a1mpc_handle_s {
    a1mpc_config cfg;
    DeviceParams dp;
    int device = 0;
    int max_batch = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    hipEvent_t ev_mark = nullptr;   // marker_at(): a no-timing event recorded where a timing event would be (A1MPC_TICK_MARKERS, profiles/r06_control_tick_timeline.md)
    bool timing = true;   // a1mpc_set_timing: HIP events around the launches (a1mpc_last_kernel_ms / _stage_ms / _control_tick_ms); off = three to five event records less per tick
    double* d_tab = nullptr;      // (alpha/beta, beta) table of cfg.horizon
    double* d_tab1 = nullptr;     // the H = 1 table (balance QP)
    // device staging for the host-pointer entry points
    double *d_x0 = nullptr, *d_xref = nullptr, *d_R = nullptr, *d_foot = nullptr, *d_aux = nullptr, *d_Rz = nullptr;
    uint8_t* d_contact = nullptr;
    double *d_grf = nullptr, *d_u = nullptr;
    int32_t *d_iters = nullptr, *d_status = nullptr, *d_nfact = nullptr;
    hipStream_t last_stream = nullptr;
    // Every launch touches handle-owned scratch (prepared-state records, queue counter / order / cost, nfact, the carried OSQP workspace,
    // the filter states): a call on another stream than the previous call's first waits for that call's work (ev_order, recorded after
    // every launch); the reset functions wait for it on the host.
    double* d_carry = nullptr;     // warm_start = 2 (the reference's update path): n x Carry<H>::STRIDE, allocated on first use
    hipEvent_t ev_order = nullptr;
    hipEvent_t ev_mid = nullptr;   // between the set-up kernel and the persistent ADMM kernel of the split pipeline (a1mpc_last_stage_ms)
    hipEvent_t ev_tick0 = nullptr, ev_tick1 = nullptr;   // around a1mpc_control_tick_device
    bool tick_timed = false, tick_fused = false, tick_km_set = false;
    double tick_km[3] = {0, 0, 0};
    bool staged = false;
    bool busy = false;
    int pipeline_depth = 0;      // > 0: this handle is a slot of an a1mpc_pipeline with that many slots (g_gen_prefer_one_wave)
    // carried OSQP workspace (warm start)
    double *d_wx = nullptr, *d_wy = nullptr, *d_rho = nullptr;
    // split pipeline: prepared state of every QP (set-up kernel -> ADMM kernel) and the work-queue counter
    double* d_prep = nullptr;
    double* d_prep_gen = nullptr;  // the general path's records (B~w_t of every step included), allocated on first use
    int* d_counter = nullptr;
    // queue order of the next solve (longest-first by the previous solve's per-QP cost) -- see a1mpc_set_schedule
    int32_t *d_order = nullptr, *d_cost = nullptr;
    double* d_foot_steps = nullptr;      // general path: n x 12H per-step feet (allocated on first use)
    uint8_t* d_contact_steps = nullptr;  // general path: n x 4H per-step contacts
    double* d_ct_state = nullptr;  // N2b filter state of every robot (allocated on first use)
    double* d_ekf_state = nullptr;  // N4c Kalman filter state of every robot (allocated on first use)
    double* d_tickrec = nullptr;    // a1mpc_control_tick_device: n x 22 tick records + 3 doubles (km_foot), allocated on first use
    uint32_t* d_pv_sched = nullptr; // a1mpc_control_tick_preview_device: n x H words, the horizon's contact schedule (allocated on first use)
    double* d_pv_foot = nullptr;    // ... and n x 12H per-step feet (allocated on first use)
    double* d_sensor_filt = nullptr;      // a1mpc_sensor_frontend_batch: the six IMU filters of every robot, [6][window + 2][max_batch] (allocated on first use, for the window in use)
    int32_t* d_sensor_cursor = nullptr;   // ... and their shared count / cursor, [2][max_batch]
    int32_t sensor_window = 0;            // the window the state was built with (0: none since the last reset); sensor_alloc_window: what the allocation holds
    int32_t sensor_alloc_window = 0;
    double* d_bal_acc = nullptr;    // a1mpc_control_tick_balance_device: n x 6 root_acc where the caller passes no buffer of its own (allocated on first use)
    double *d_hs_u = nullptr, *d_hs_x = nullptr;   // a1mpc_horizon_states_batch (host pointers): n x 12H forces in, n x 13H predicted states out (allocated on first use)
    int32_t ekf_ready_n = 0;        // robots 0 .. ekf_ready_n - 1 have had their filter initialised (the init kernel is not launched for them again)
    // staging of the host-pointer entries of the caller-side stages, allocated on first use (ensure_aux; handed out by Staging)
    double *d_aux_in = nullptr, *d_aux_out = nullptr;
    uint8_t* d_aux_u8 = nullptr;
    double* d_episode_ws = nullptr;   // a1mpc_episode_summary_batch: 20 doubles for the host entry's summary, then the partial summaries of every level (episode_ws_doubles)
    int32_t hint_n = 0;  // batch size the order was built for (0 = none)
    bool profiling = false;        // a1mpc_set_profiling: split-pipeline solves run the clock-stamped instantiation of the ADMM kernel
    long long* d_clk = nullptr;    // n x kTickStages cycles per QP (allocated on first use)
    int32_t clk_n = 0;             // QPs of the last profiled solve (0: the last solve was not profiled)
    bool clk_tick = false;         // ... and it ran the fused / latency kernel: every stage of the record is filled (a1mpc_last_tick_stage_cycles)
    int32_t last_ws_mode = -1;  // warm-start semantics the last MPC solve ran (a1mpc_last_warm_start_mode): the configured mode, or 1 where mode 2 does not exist
    int schedule = 1;    // 1 = history (default), 0 = index order
    // packed device blocks + pinned host mirrors of the host-pointer MPC entry (one copy each way per call)
    char *d_in = nullptr, *d_out = nullptr;
    char* h_pin = nullptr;
    char* d_pin = nullptr;   // the pinned block as the device sees it (hipHostGetDevicePointer), or null: small batches read / write it directly (pin_inputs)
    size_t h_pin_bytes = 0, h_pin_in_bytes = 0;
};

static a1mpc_status order_streams(a1mpc_handle h, hipStream_t s) {
    if (h->busy && h->last_stream != s) A1_HIP(hipStreamWaitEvent(s, h->ev_order, 0));
    return A1MPC_OK;
}
static a1mpc_status mark_launched(a1mpc_handle h, hipStream_t s) {
    A1_HIP(hipEventRecord(h->ev_order, s));
    h->busy = true; h->last_stream = s;
    return A1MPC_OK;
}
#define A1_ORDER(h, s) do { if (a1mpc_status so_ = order_streams(h, s); so_ != A1MPC_OK) return so_; } while (0)
#define A1_MARK(h, s) do { if (a1mpc_status sm_ = mark_launched(h, s); sm_ != A1MPC_OK) return sm_; } while (0)
// grid of the kernels that run one lane per (robot, leg) in workgroups of 256
static dim3 leg_lane_grid(int32_t n) { return dim3(static_cast<unsigned>((static_cast<size_t>(n) * 4 + 255) / 256)); }

extern "C" {

void a1mpc_default_config(a1mpc_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->horizon = 10;         // PLAN_HORIZON, S/A1Params.h:26
    c->dt = 0.0025;          // S/A1RobotControl.cpp:462
    c->mu = 0.3;             // S/ConvexMpc.cpp:8
    c->fz_min = 0.0;         // S/ConvexMpc.cpp:223
    c->fz_max = 180.0;       // S/ConvexMpc.cpp:224
    c->rho = 0.1; c->sigma = 1e-6; c->alpha = 1.6; c->eps_abs = 1e-3; c->eps_rel = 1e-3;  // OSQP 0.6 defaults
    c->adaptive_rho_tolerance = 5.0;
    c->max_iter = 4000; c->check_termination = 25; c->adaptive_rho = 1; c->adaptive_rho_interval = 25; c->scaling = 10;
    c->warm_start = 1;       // S/A1RobotControl.cpp:524
}

void a1mpc_default_balance_config(a1mpc_balance_config* q) {
    if (!q) return;
    const double Q[6] = {1.0, 1.0, 1.0, 400.0, 400.0, 100.0};  // S/A1RobotControl.cpp:11
    std::memcpy(q->Q, Q, sizeof Q);
    q->R = 1e-3; q->mu = 0.7; q->F_min = 0.0; q->F_max = 180.0;  // S/A1RobotControl.cpp:12-15
}

// ---- N2b: contact logic + recent-contact filters, walking-surface fit, terrain pitch (S/A1RobotControl.cpp:256-282, 566-582, 335-376) --------
// Device-resident state per robot, laid out so that one tick touches whole cache lines whatever phase the robots' filters are in (round 3; until then
// every field was its own [robot] array, which coalesces only while all robots' ring cursors agree -- they part with the first early contact):
//   record, 384 B, 128-aligned: 4 x CtLeg (64 B: the leg's window count and cursor -- its three position filters are always updated together, so they
//           share them --, the early-contact flag, 3 x Neumaier sum / correction) + CtRobot (128 B: foot_pos_recent_contact, the terrain-angle filter's header);
//   leg rings  [robot][leg][60 slots][4 doubles] (x, y, z of one tick in one 32-byte sector; the 4th is padding);
//   terrain ring [100 slots][robot]: this filter advances on every tick of a robot that stands (root height > 0.1 m), so the robots' cursors agree unless one of them
//           has been lying down -- neighbouring robots then touch neighbouring words (the leg rings cannot have that: early contacts part their cursors for good).
// One lane per robot: 3 lines of record + one sector per leg in contact + one word of the terrain ring, read and written once.  No FMA contraction.
constexpr int kLegWindow = 60, kTerrainWindow = 100;
struct CtLeg { int32_t count, head; double early, sum[3], corr[3]; };
struct CtRobot { double recent[12]; int32_t count, head; double sum, corr, pad_; };
struct CtRecord { CtLeg leg[4]; CtRobot rb; };   // (no alignas: the records start a hipMalloc block, which is 256-byte aligned, and their LDS image below is not 128-aligned)
static_assert(sizeof(CtLeg) == 64 && sizeof(CtRobot) == 128 && sizeof(CtRecord) == 384, "contact-state record: three 128-byte lines");
constexpr size_t kCtLegRing = 4 * kLegWindow * 4;  // doubles per robot
constexpr size_t kCtBytesPerRobot = sizeof(CtRecord) + (kCtLegRing + kTerrainWindow) * sizeof(double);
struct ContactArgs {
    int32_t n;
    double counter_per_swing, foot_force_low;
    int32_t use_terrain_adapt;
    CtRecord* rec;
    double *leg_ring, *terrain_ring;
    int64_t stride;  // robots per terrain-ring slot (= max_batch)
    const double *gait_counter, *foot_force, *foot_pos_abs, *root_pos_z;
    const uint8_t* plan_contacts;
    double* pitch_d;
    int32_t z_stride, pitch_stride;   // doubles between two robots' root_pos_z / root_euler_d pitch (1: arrays of their own; 3: element 2 of root_pos / element 1 of root_euler_d, a1mpc_control_tick_device)
    // a1mpc_control_tick_device: the lane that has just written a robot's terrain pitch also assembles its 22-number MPC tick record (a1mpc_tick_pack_kernel's job, one
    // launch less per tick), or pk_tick = null
    const double *pk_euler, *pk_pos, *pk_ang_vel, *pk_lin_vel, *pk_euler_d, *pk_lin_vel_d, *pk_ang_vel_d, *pk_pos_d_z;
    double* pk_tick;
    uint8_t* contacts;
    double *recent_out, *terrain_out;
    const double* recent_in;  // terrain-only entry: foot_pos_recent_contact comes from the caller instead of the handle's contact state
};
struct Neumaier {  // S/utils/filter.hpp:26-39,53-66: the moving-window sum with its running compensation
    double sum, corr;
    __device__ inline void add(double val) {
#pragma clang fp contract(off)
        const double ns = sum + val;
        if (fabs(sum) >= fabs(val)) corr += (sum - ns) + val; else corr += (val - ns) + sum;
        sum = ns;
    }
};
__device__ inline void sym3_pinv(const double* m, double* out) {  // pseudo-inverse of a symmetric PSD 3x3 by cyclic Jacobi (S/utils/Utils.cpp:44-52)
#pragma clang fp contract(off)
    double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) a[k] = m[k];
    for (int sweep = 0; sweep < 8; ++sweep) {
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[3 * p + q];
            if (apq == 0.0) continue;
            const double th = (a[3 * q + q] - a[3 * p + p]) / (2.0 * apq);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
            for (int k = 0; k < 3; ++k) { const double akp = a[3 * k + p], akq = a[3 * k + q]; a[3 * k + p] = c * akp - sn * akq; a[3 * k + q] = sn * akp + c * akq; }
            for (int k = 0; k < 3; ++k) { const double apk = a[3 * p + k], aqk = a[3 * q + k]; a[3 * p + k] = c * apk - sn * aqk; a[3 * q + k] = sn * apk + c * aqk; }
            for (int k = 0; k < 3; ++k) { const double vkp = v[3 * k + p], vkq = v[3 * k + q]; v[3 * k + p] = c * vkp - sn * vkq; v[3 * k + q] = sn * vkp + c * vkq; }
        }
    }
    double lmax = fabs(a[0]);
    if (fabs(a[4]) > lmax) lmax = fabs(a[4]);
    if (fabs(a[8]) > lmax) lmax = fabs(a[8]);
    const double tol = 2.220446049250313e-16 * 3.0 * lmax;
    double inv[3];
    for (int k = 0; k < 3; ++k) inv[k] = fabs(a[4 * k]) > tol ? 1.0 / a[4 * k] : 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            out[3 * i + j] = v[3 * i + 0] * inv[0] * v[3 * j + 0] + v[3 * i + 1] * inv[1] * v[3 * j + 1] + v[3 * i + 2] * inv[2] * v[3 * j + 2];
}
// a robot's inputs of one tick: loaded BEFORE its record is staged, so that they travel with the record instead of after it (round 6: until then they were loaded behind the
// staging barrier, the ring sectors behind them, root_pos_z behind the plane fit and the terrain ring's word behind that -- five exposures to the memory latency per robot, now two)
// contacts_only (a literal at every call: folded where these bodies are inlined): the contact block alone, a1mpc_contacts_batch -- root_pos_z is not read, and neither
// the terrain-angle filter, the plane fit, root_euler_d nor a terrain output is touched (S/A1RobotControl.cpp:335: "only do terrain adaptation in MPC")
struct CtInputs { double gc[4], ff[4], fp[12], rz; uint8_t plan[4]; };
__device__ __forceinline__ CtInputs contact_terrain_inputs(const ContactArgs& a, const int64_t b, const bool contacts_only = false) {
    CtInputs in;
    in.rz = contacts_only ? 0.0 : a.root_pos_z[b * a.z_stride];
    if (!a.recent_in) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { in.gc[i] = a.gait_counter[b * 4 + i]; in.ff[i] = a.foot_force[b * 4 + i]; in.plan[i] = a.plan_contacts[b * 4 + i]; }
#pragma unroll
        for (int k = 0; k < 12; ++k) in.fp[k] = a.foot_pos_abs[b * 12 + k];
    }
    return in;
}
// one robot's tick on its record `st` (the kernel hands in the record's LDS image; the terrain-only entry and the host-compiled test double the record itself)
__device__ __forceinline__ void contact_terrain_robot_in(const ContactArgs& a, const int64_t b, CtRecord* st, const CtInputs& in, const bool contacts_only = false) {
#pragma clang fp contract(off)
    double rc[12];
    // the terrain-angle filter's word under its cursor is read here, with the leg rings' sectors: everything a tick reads in place is in flight before anything is computed
    const bool standing = !contacts_only && in.rz > 0.1;
    const int tcount = st->rb.count, thead = st->rb.head;
    double* tr = a.terrain_ring + thead * a.stride + b;
    const double tr_old = (standing && tcount >= kTerrainWindow) ? *tr : 0.0;
    if (a.recent_in) {
#pragma unroll
        for (int k = 0; k < 12; ++k) rc[k] = a.recent_in[b * 12 + k];
    } else {
        CtLeg L[4];
        double slot[4][3];
        const double (&gc)[4] = in.gc, (&ff)[4] = in.ff, (&fp)[12] = in.fp;
        const uint8_t (&plan)[4] = in.plan;
        bool c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) L[i] = st->leg[i];
#pragma unroll
        for (int k = 0; k < 12; ++k) rc[k] = st->rb.recent[k];
        double* ring = a.leg_ring + b * kCtLegRing;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double e = L[i].early;
            if (gc[i] <= a.counter_per_swing * 1.5) e = 0.0;                                                        // :260-262
            if (!plan[i] && gc[i] > a.counter_per_swing * 1.5 && ff[i] > a.foot_force_low) e = 1.0;                 // :263-267
            c[i] = plan[i] != 0 || e != 0.0;                                                                        // :271
            if (e != L[i].early) st->leg[i].early = e;
            a.contacts[b * 4 + i] = c[i] ? 1 : 0;
            const double* sl = ring + (i * kLegWindow + L[i].head) * 4;
            const bool full = c[i] && L[i].count >= kLegWindow;   // only then does the slot under the cursor hold a sample to retire
#pragma unroll
            for (int k = 0; k < 3; ++k) slot[i][k] = full ? sl[k] : 0.0;
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!c[i]) continue;                                                                                    // :274-281
            any = true;
            const bool full = L[i].count >= kLegWindow;
            double* sl = ring + (i * kLegWindow + L[i].head) * 4;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Neumaier f{L[i].sum[k], L[i].corr[k]};
                if (full) f.add(-slot[i][k]);
                f.add(fp[3 * i + k]);
                sl[k] = fp[3 * i + k];
                st->leg[i].sum[k] = f.sum; st->leg[i].corr[k] = f.corr;
                rc[3 * i + k] = (f.sum + f.corr) / static_cast<double>(kLegWindow);
            }
            st->leg[i].count = full ? L[i].count : L[i].count + 1;
            st->leg[i].head = (L[i].head + 1) % kLegWindow;
        }
        if (any) {
#pragma unroll
            for (int k = 0; k < 12; ++k) st->rb.recent[k] = rc[k];
        }
    }
    if (a.recent_out) {
#pragma unroll
        for (int k = 0; k < 12; ++k) a.recent_out[b * 12 + k] = rc[k];
    }
    if (contacts_only) return;
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rhs[3] = {0, 0, 0}, P3[9], co[3];   // :566-582  a = pinv(W'W) W' z
    for (int i = 0; i < 4; ++i) {
        const double w[3] = {1.0, rc[3 * i + 0], rc[3 * i + 1]};
        for (int r = 0; r < 3; ++r) { for (int cc = 0; cc < 3; ++cc) M[3 * r + cc] += w[r] * w[cc]; rhs[r] += w[r] * rc[3 * i + 2]; }
    }
    sym3_pinv(M, P3);
    for (int r = 0; r < 3; ++r) co[r] = P3[3 * r + 0] * rhs[0] + P3[3 * r + 1] * rhs[1] + P3[3 * r + 2] * rhs[2];
    const double s0 = co[1], s1 = co[2], s2 = -1.0;
    double terrain_angle = 0.0;                                                             // :339-352
    if (standing) {
        const double angle_cos = fabs(0.0 * s0 + 0.0 * s1 + 1.0 * s2) / (sqrt(0.0 * 0.0 + 0.0 * 0.0 + 1.0 * 1.0) * sqrt(s0 * s0 + s1 * s1 + s2 * s2));
        const double v = acos(angle_cos);
        Neumaier f{st->rb.sum, st->rb.corr};
        if (tcount >= kTerrainWindow) f.add(-tr_old); else st->rb.count = tcount + 1;
        f.add(v);
        *tr = v;
        st->rb.head = (thead + 1) % kTerrainWindow; st->rb.sum = f.sum; st->rb.corr = f.corr;
        terrain_angle = (f.sum + f.corr) / static_cast<double>(kTerrainWindow);
    }
    if (terrain_angle > 0.5) terrain_angle = 0.5;
    if (terrain_angle < -0.5) terrain_angle = -0.5;
    const double F_R_diff = rc[2] + rc[5] - rc[8] - rc[11];                                // :355
    if (a.use_terrain_adapt) a.pitch_d[b * a.pitch_stride] = F_R_diff > 0.05 ? -terrain_angle : terrain_angle;  // :358-364
    a.terrain_out[b] = terrain_angle;
}
// (a name of its own, not an overload: this section sits inside the ABI's extern "C" block, where two functions of one name are ONE symbol)
__device__ __forceinline__ void contact_terrain_robot(const ContactArgs& a, const int64_t b, CtRecord* st) { contact_terrain_robot_in(a, b, st, contact_terrain_inputs(a, b)); }
// One wavefront = 64 robots.  A lane that walks its own 384-byte record in HBM makes every load instruction touch 64 different lines (measured: 2.5 TB/s of algorithmic
// bytes at 524 288 robots whether the plane fit runs or not).  The wavefront therefore moves its 24 KB of records as 24 fully coalesced 16-byte-per-lane loads into LDS,
// every lane works on the LDS image of its record (stride 400 B = 25 x 16 B: the 16 lanes of a ds_read_b128 phase hit 16 different quad-banks), and the image goes back
// the same way -- whole lines in, whole lines out.  Only the ring sectors are touched in place (one 32-byte sector per leg in contact, wherever that robot's cursor is).
constexpr int kCtLdsStride = 400, kCtUnits = sizeof(CtRecord) / 16;   // bytes per record image; 16-byte units per record
__global__ __launch_bounds__(64) void a1mpc_contact_terrain_kernel(const ContactArgs a) {
    const int64_t base = static_cast<int64_t>(blockIdx.x) * 64;
    const int lane = threadIdx.x;
    const int64_t b = base + lane;
    if (a.recent_in) {   // terrain-only entry: 24 bytes of the record matter
        if (b < a.n) contact_terrain_robot(a, b, a.rec + b);
        return;
    }
    __shared__ __attribute__((aligned(16))) unsigned char img[64 * kCtLdsStride];
    const int cnt = a.n - base < 64 ? static_cast<int>(a.n - base) : 64;
    const CtInputs in = contact_terrain_inputs(a, b < a.n ? b : a.n - 1);   // (in flight together with the record)
    const uint4* src = reinterpret_cast<const uint4*>(a.rec + base);
    uint4 v[kCtUnits];
#pragma unroll
    for (int i = 0; i < kCtUnits; ++i) { const int o = i * 64 + lane; v[i] = o < cnt * kCtUnits ? src[o] : uint4{0, 0, 0, 0}; }
#pragma unroll
    for (int i = 0; i < kCtUnits; ++i) { const int o = i * 64 + lane, r = o / kCtUnits, w = o - r * kCtUnits; *reinterpret_cast<uint4*>(img + r * kCtLdsStride + w * 16) = v[i]; }
    __syncthreads();
    if (b < a.n) contact_terrain_robot_in(a, b, reinterpret_cast<CtRecord*>(img + lane * kCtLdsStride), in);
    if (b < a.n && a.pk_tick != nullptr) {   // (S/A1RobotControl.cpp:452-456, :470-488 read exactly these fields; root_euler_d[1] is the pitch this lane has just written)
        double* t = a.pk_tick + b * 22;
        double tv[22];   // (every load before the first store: written field by field each load waited for the store before it -- the compiler cannot know that t[] and the sources are apart)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tv[k] = a.pk_euler[b * 3 + k]; tv[3 + k] = a.pk_pos[b * 3 + k]; tv[6 + k] = a.pk_ang_vel[b * 3 + k]; tv[9 + k] = a.pk_lin_vel[b * 3 + k];
            tv[12 + k] = a.pk_euler_d[b * 3 + k]; tv[15 + k] = a.pk_lin_vel_d[b * 3 + k]; tv[18 + k] = a.pk_ang_vel_d[b * 3 + k];
        }
        tv[21] = a.pk_pos_d_z[b];
#pragma unroll
        for (int k = 0; k < 22; ++k) t[k] = tv[k];
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(a.rec + base);
#pragma unroll
    for (int i = 0; i < kCtUnits; ++i) { const int o = i * 64 + lane, r = o / kCtUnits, w = o - r * kCtUnits; if (o < cnt * kCtUnits) dst[o] = *reinterpret_cast<const uint4*>(img + r * kCtLdsStride + w * 16); }
}
// The contact block alone (a1mpc_contacts_batch, the balance control tick): the kernel above with contacts_only folded in -- the same staging of the records through LDS
// around the same per-robot body, which returns in front of the plane fit.  A kernel of its own, so that the kernel above keeps its code to the instruction
__global__ __launch_bounds__(64) void a1mpc_contacts_kernel(const ContactArgs a) {
    const int64_t base = static_cast<int64_t>(blockIdx.x) * 64;
    const int lane = threadIdx.x;
    const int64_t b = base + lane;
    __shared__ __attribute__((aligned(16))) unsigned char img[64 * kCtLdsStride];
    const int cnt = a.n - base < 64 ? static_cast<int>(a.n - base) : 64;
    const CtInputs in = contact_terrain_inputs(a, b < a.n ? b : a.n - 1, true);
    const uint4* src = reinterpret_cast<const uint4*>(a.rec + base);
    uint4 v[kCtUnits];
#pragma unroll
    for (int i = 0; i < kCtUnits; ++i) { const int o = i * 64 + lane; v[i] = o < cnt * kCtUnits ? src[o] : uint4{0, 0, 0, 0}; }
#pragma unroll
    for (int i = 0; i < kCtUnits; ++i) { const int o = i * 64 + lane, r = o / kCtUnits, w = o - r * kCtUnits; *reinterpret_cast<uint4*>(img + r * kCtLdsStride + w * 16) = v[i]; }
    __syncthreads();
    if (b < a.n) contact_terrain_robot_in(a, b, reinterpret_cast<CtRecord*>(img + lane * kCtLdsStride), in, true);
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(a.rec + base);
#pragma unroll
    for (int i = 0; i < kCtUnits; ++i) { const int o = i * 64 + lane, r = o / kCtUnits, w = o - r * kCtUnits; if (o < cnt * kCtUnits) dst[o] = *reinterpret_cast<const uint4*>(img + r * kCtLdsStride + w * 16); }
}
// the handle's contact state: records, then the leg rings, then the terrain rings (zero = every filter empty)
static a1mpc_status ensure_contact_state(a1mpc_handle h, hipStream_t s) {
    if (h->d_ct_state) return A1MPC_OK;
    A1_HIP(hipMalloc(&h->d_ct_state, static_cast<size_t>(h->max_batch) * kCtBytesPerRobot));
    A1_HIP(hipMemsetAsync(h->d_ct_state, 0, static_cast<size_t>(h->max_batch) * kCtBytesPerRobot, s));
    return A1MPC_OK;
}
// Every field of ContactArgs, for its four users.  As filled here: root_pos_z / pitch_d are arrays of their own (strides 1), no tick record is packed and
// foot_pos_recent_contact is the handle's; the control tick and a1mpc_terrain_batch set the few fields they differ in on the result.
static ContactArgs make_contact_args(a1mpc_handle h, const a1mpc_contact_config& cfg, int32_t n, const double* gait_counter, const uint8_t* plan_contacts,
                                     const double* foot_force, const double* foot_pos_abs, const double* root_pos_z, double* pitch_d, uint8_t* contacts, double* recent_out,
                                     double* terrain_out) {
    ContactArgs a;
    a.n = n; a.counter_per_swing = cfg.counter_per_swing; a.foot_force_low = cfg.foot_force_low; a.use_terrain_adapt = cfg.use_terrain_adapt;
    a.rec = reinterpret_cast<CtRecord*>(h->d_ct_state);
    a.leg_ring = reinterpret_cast<double*>(a.rec + h->max_batch);
    a.terrain_ring = a.leg_ring + static_cast<size_t>(h->max_batch) * kCtLegRing;
    a.stride = h->max_batch;
    a.gait_counter = gait_counter; a.foot_force = foot_force; a.foot_pos_abs = foot_pos_abs; a.root_pos_z = root_pos_z; a.plan_contacts = plan_contacts;
    a.pitch_d = pitch_d; a.z_stride = 1; a.pitch_stride = 1;
    a.pk_euler = a.pk_pos = a.pk_ang_vel = a.pk_lin_vel = a.pk_euler_d = a.pk_lin_vel_d = a.pk_ang_vel_d = a.pk_pos_d_z = nullptr; a.pk_tick = nullptr;
    a.contacts = contacts; a.recent_out = recent_out; a.terrain_out = terrain_out; a.recent_in = nullptr;
    return a;
}
static void launch_contact_terrain(const ContactArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(a1mpc_contact_terrain_kernel, dim3(static_cast<unsigned>((a.n + 63) / 64)), dim3(64), 0, s, a);
}
// the contact block alone on the handle's contact state: no root_pos_z, no pitch, no terrain output, and the terrain-angle filter stays as it is
static void launch_contacts(a1mpc_handle h, const a1mpc_contact_config& cfg, int32_t n, const double* gait_counter, const uint8_t* plan_contacts, const double* foot_force,
                            const double* foot_pos_abs, uint8_t* contacts, double* recent_out, hipStream_t s) {
    const ContactArgs a = make_contact_args(h, cfg, n, gait_counter, plan_contacts, foot_force, foot_pos_abs, nullptr, nullptr, contacts, recent_out, nullptr);
    hipLaunchKernelGGL(a1mpc_contacts_kernel, dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64), 0, s, a);
}

// ---- sensor front end (a1mpc_sensor_frontend_batch): what the reference's callbacks make of a quaternion and a raw IMU sample -- gt_pose_callback
// (S/GazeboA1ROS.cpp:235-262: root_rot_mat, root_euler, root_rot_mat_z) and imu_callback (:284-300: six MovingWindowFilter(5), root_ang_vel = root_rot_mat * imu_ang_vel).
// One lane per robot, workgroups of 256; 10 doubles in, 30 out, and the six filters' state.
//   state     field-major, [filter][slot 0 .. window - 1 | sum | corr][robot] with `stride` robots per field, then [count | head][robot] as int32: a wavefront's access to
//             one field is one contiguous run of 512 bytes (256 for the two cursors) while the robots' cursors agree, and neighbouring words of `window` runs where they
//             have parted (a call with fewer robots in between).  The six filters of a robot are always updated together and share one count and one cursor.  The window
//             is addressed in memory, by the cursor: no per-lane array, nothing for the compiler to put into scratch.
//   loads     the raw sample, the cursors and the twelve sums / corrections are issued before the first operation, the six slots under the cursor behind the cursor's
//             arrival (the only dependent load); every store follows the last operation.
//   bits      contraction off; Eigen's operation order for both matrices (Quaternion::toRotationMatrix; AngleAxis::toRotationMatrix with the axis (0, 0, 1) written out,
//             products with the axis' zeros included: a NaN yaw fills the matrix as it does there), S/utils/Utils.cpp:7-33 for the angles with the clamp of t2, the
//             filters as S/utils/filter.hpp:26-62 (Neumaier, the division by the window length from the first sample on): everything but atan2, asin, sin and cos is the
//             reference's arithmetic bit for bit.  The quaternion is not normalised, as in the reference.
// Plain C++ without intrinsics: the CPU suite compiles this section for the host (tests/emu/frontend_host.py).
constexpr int kImuWindowMax = A1MPC_IMU_WINDOW_MAX;
constexpr int kImuFilters = 6;   // acc x, y, z, gyro x, y, z
struct SensorArgs {
    int32_t n, window;
    int64_t stride;                               // robots per state field (= max_batch)
    const double *quat, *acc_raw, *gyro_raw;      // n x 4 (w, x, y, z), n x 3, n x 3
    double* filt;                                 // [6][window + 2][stride]
    int32_t* cursor;                              // [2][stride]: samples held (<= window), next slot
    double *R_world, *R_z, *euler, *acc, *gyro, *ang_vel;
};
__global__ __launch_bounds__(256) void a1mpc_sensor_frontend_kernel(const SensorArgs a) {
#pragma clang fp contract(off)
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (b >= a.n) return;
    const int64_t fields = a.window + 2;
    const double qw = a.quat[b * 4 + 0], x = a.quat[b * 4 + 1], y = a.quat[b * 4 + 2], z = a.quat[b * 4 + 3];
    double raw[kImuFilters];
    Neumaier f[kImuFilters];
    const int32_t count = a.cursor[b], head = a.cursor[a.stride + b];
#pragma unroll
    for (int i = 0; i < 3; ++i) { raw[i] = a.acc_raw[b * 3 + i]; raw[3 + i] = a.gyro_raw[b * 3 + i]; }
#pragma unroll
    for (int k = 0; k < kImuFilters; ++k) {
        const double* fk = a.filt + (k * fields + a.window) * a.stride + b;
        f[k].sum = fk[0]; f[k].corr = fk[a.stride];
    }
    double old[kImuFilters];
#pragma unroll
    for (int k = 0; k < kImuFilters; ++k) old[k] = a.filt[(k * fields + head) * a.stride + b];
    // Eigen::Quaternion::toRotationMatrix
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    double R[9];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
    // Utils::quat_to_euler, S/utils/Utils.cpp:17-31
    const double y_sqr = y * y;
    const double t0 = 2.0 * (qw * x + y * z), t1 = 1.0 - 2.0 * (x * x + y_sqr);
    double t2 = 2.0 * (qw * y - z * x);
    t2 = t2 > 1.0 ? 1.0 : t2;
    t2 = t2 < -1.0 ? -1.0 : t2;
    const double t3 = 2.0 * (qw * z + x * y), t4 = 1.0 - 2.0 * (y_sqr + z * z);
    const double roll = atan2(t0, t1), pitch = asin(t2), yaw = atan2(t3, t4);
    // Eigen::AngleAxisd(yaw, UnitZ()).toRotationMatrix(): sin_axis = s * axis, cos1_axis = (1 - c) * axis, the off-diagonal pairs tmp -+ sin_axis, the diagonal cos1_axis .* axis + c
    const double sn = sin(yaw), c = cos(yaw);
    const double ax = 0.0, ay = 0.0, az = 1.0;
    const double sx = sn * ax, sy = sn * ay, sz = sn * az, cx = (1.0 - c) * ax, cy = (1.0 - c) * ay, cz = (1.0 - c) * az;
    double Rz[9];
    double tmp = cx * ay; Rz[1] = tmp - sz; Rz[3] = tmp + sz;
    tmp = cx * az; Rz[2] = tmp + sy; Rz[6] = tmp - sy;
    tmp = cy * az; Rz[5] = tmp - sx; Rz[7] = tmp + sx;
    Rz[0] = cx * ax + c; Rz[4] = cy * ay + c; Rz[8] = cz * az + c;
    // MovingWindowFilter::CalculateAverage, S/utils/filter.hpp:26-39
    const bool full = count >= a.window;
    const double wlen = static_cast<double>(a.window);
    double avg[kImuFilters];
#pragma unroll
    for (int k = 0; k < kImuFilters; ++k) {
        if (full) f[k].add(-old[k]);
        f[k].add(raw[k]);
        avg[k] = (f[k].sum + f[k].corr) / wlen;
    }
    double wv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) wv[i] = R[i * 3 + 0] * avg[3] + R[i * 3 + 1] * avg[4] + R[i * 3 + 2] * avg[5];   // :299
#pragma unroll
    for (int k = 0; k < kImuFilters; ++k) {
        double* fk = a.filt + (k * fields + a.window) * a.stride + b;
        a.filt[(k * fields + head) * a.stride + b] = raw[k];
        fk[0] = f[k].sum; fk[a.stride] = f[k].corr;
    }
    a.cursor[b] = full ? count : count + 1;
    a.cursor[a.stride + b] = head + 1 == a.window ? 0 : head + 1;
#pragma unroll
    for (int k = 0; k < 9; ++k) { a.R_world[b * 9 + k] = R[k]; a.R_z[b * 9 + k] = Rz[k]; }
    a.euler[b * 3 + 0] = roll; a.euler[b * 3 + 1] = pitch; a.euler[b * 3 + 2] = yaw;
#pragma unroll
    for (int i = 0; i < 3; ++i) { a.acc[b * 3 + i] = avg[i]; a.gyro[b * 3 + i] = avg[3 + i]; a.ang_vel[b * 3 + i] = wv[i]; }
}

// ---- command stage (a1mpc_command_batch): the first half of main_update, S/GazeboA1ROS.cpp:124-188, branch for branch -- body-height integrator with its clamps, the mode
// toggle, the commanded velocities, root_euler_d's integration, the xy position lock and the switching of kp_linear[0:2] -- and the mpc_init_counter gate of
// compute_joint_torques (S/A1RobotControl.cpp:292-294).  One lane per robot, workgroups of 256, element-wise: every load before the first operation, every store behind the
// last.  Contraction off (cmd * dt is rounded before it is added); sqrt is IEEE's.  Plain C++ without intrinsics (tests/emu/frontend_host.py compiles this section too).
struct CommandArgs {
    int32_t n, init_ticks;
    double dt, height_max, height_min, lock_x, lock_y, lock_speed;
    const double *cmd, *root_pos;    // n x 6 (velx, vely, velz, roll / pitch / yaw rate), n x 3
    const uint8_t* toggle;           // n
    double *body_height, *euler_d, *pos_d, *kp_xy;   // in/out: n, n x 3, n x 3, n x 2
    uint8_t* ctrl_state;             // in/out, n
    int32_t* init_counter;           // in/out, n
    double *lin_vel_d, *ang_vel_d, *pos_d_z;         // out: n x 3, n x 3, n
    uint8_t *movement_mode, *mpc_active;             // out: n
};
__global__ __launch_bounds__(256) void a1mpc_command_kernel(const CommandArgs a) {
#pragma clang fp contract(off)
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (b >= a.n) return;
    double cmd[6], ed[3], pd[2], kp[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) cmd[k] = a.cmd[b * 6 + k];
    const double px = a.root_pos[b * 3 + 0], py = a.root_pos[b * 3 + 1];
    double height = a.body_height[b];
#pragma unroll
    for (int i = 0; i < 3; ++i) ed[i] = a.euler_d[b * 3 + i];
#pragma unroll
    for (int i = 0; i < 2; ++i) { pd[i] = a.pos_d[b * 3 + i]; kp[i] = a.kp_xy[b * 2 + i]; }
    const int prev = a.ctrl_state[b];
    const bool toggle = a.toggle[b] != 0;
    int32_t ticks = a.init_counter[b];
    height = height + cmd[2] * a.dt;                                            // :124-130
    if (height >= a.height_max) height = a.height_max;
    if (height <= a.height_min) height = a.height_min;
    int state = prev;
    if (toggle) state = (state + 1) % 2;                                        // :142-147
#pragma unroll
    for (int i = 0; i < 3; ++i) ed[i] = ed[i] + cmd[3 + i] * a.dt;              // :158-160
    int mode;
    if (state == 1) mode = 1;                                                   // :164-176
    else if (state == 0 && prev == 1) { mode = 0; pd[0] = px; pd[1] = py; kp[0] = a.lock_x; kp[1] = a.lock_y; }   // leave walking mode: one tick only
    else mode = 0;
    if (mode == 1) {                                                            // :179-188
        if (sqrt(cmd[0] * cmd[0] + cmd[1] * cmd[1]) > a.lock_speed) { pd[0] = px; pd[1] = py; kp[0] = 0.0; kp[1] = 0.0; }
        else { kp[0] = a.lock_x; kp[1] = a.lock_y; }
    }
    if (ticks < 2147483647) ticks = ticks + 1;                                  // S/A1RobotControl.cpp:292 (an int there too; held at its maximum here)
    a.body_height[b] = height; a.ctrl_state[b] = static_cast<uint8_t>(state); a.init_counter[b] = ticks;
#pragma unroll
    for (int i = 0; i < 3; ++i) { a.euler_d[b * 3 + i] = ed[i]; a.lin_vel_d[b * 3 + i] = cmd[i]; a.ang_vel_d[b * 3 + i] = cmd[3 + i]; }
    a.pos_d[b * 3 + 0] = pd[0]; a.pos_d[b * 3 + 1] = pd[1]; a.pos_d[b * 3 + 2] = height; a.pos_d_z[b] = height;
    a.kp_xy[b * 2 + 0] = kp[0]; a.kp_xy[b * 2 + 1] = kp[1];
    a.movement_mode[b] = static_cast<uint8_t>(mode); a.mpc_active[b] = ticks >= a.init_ticks ? 1 : 0;
}

// ---- what the entry points of the caller-side stages share.  A stage has a launcher (launch_<stage>: scalars and DEVICE pointers in, the args struct filled and the
// kernel launched on a stream the caller has ordered) and two entries around it: the device-pointer one is the macros below and the launcher, the host-pointer
// one also stages the caller's arrays through the handle's staging buffers (Staging) on the handle's stream.
//   A1_STAGE_BEGIN   every refusal, all before the first HIP call; then A1_STAGE_DEVICE (on its own where an entry has refusals of its own in front): the device and
//                    the stream `s` (hip_stream, or null = the handle's), ordered behind the handle's previous launch -- once: the launchers do not order again
//   A1_STAGE_LAUNCH  the launch between the timing events, its status, and the mark that the next call's ordering waits for
static hipStream_t stream_or_own(a1mpc_handle h, void* hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream; }
#define A1_STAGE_DEVICE(hip_stream)                                                                           \
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");      \
    if (n == 0) return A1MPC_OK;                                                                             \
    A1_HIP(hipSetDevice(h->device));                                                                         \
    hipStream_t s = stream_or_own(h, hip_stream);                                                            \
    A1_ORDER(h, s)
#define A1_STAGE_BEGIN(ok, what, hip_stream)                                            \
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");                      \
    if (n < 0 || !(ok)) return fail(A1MPC_ERR_INVALID_ARGUMENT, what);                   \
    A1_STAGE_DEVICE(hip_stream)
#define A1_STAGE_LAUNCH(...)                                  \
    do {                                                      \
        if (h->timing) A1_HIP(hipEventRecord(h->ev0, s));     \
        __VA_ARGS__;                                          \
        A1_HIP(hipGetLastError());                            \
        if (h->timing) A1_HIP(hipEventRecord(h->ev1, s));     \
        h->timed = h->timing; A1_MARK(h, s);                  \
    } while (0)

// The handle's staging for the host-pointer entries, allocated on first use.  Per robot: kAuxIn + kAuxOut doubles in two blocks, and kAuxU8 bytes handed out in
// slices of kAuxU8Slice (every byte array starts 8-byte aligned whatever the batch size)
constexpr size_t kAuxIn = 64, kAuxOut = 96, kAuxU8 = 32, kAuxU8Slice = 8;   // (four byte arrays: a1mpc_command_batch)
static a1mpc_status ensure_aux(a1mpc_handle h) {
    if (h->d_aux_in) return A1MPC_OK;
    const size_t n = static_cast<size_t>(h->max_batch);
    A1_HIP(hipMalloc(&h->d_aux_in, n * kAuxIn * sizeof(double)));
    A1_HIP(hipMalloc(&h->d_aux_out, n * kAuxOut * sizeof(double)));
    A1_HIP(hipMalloc(&h->d_aux_u8, n * kAuxU8));
    return A1MPC_OK;
}
// One host-pointer call's view of that staging: consecutive per-robot slices (doubles from d_aux_in while it has room, then from d_aux_out), the inbound copies issued
// as the slices are handed out, the outbound ones remembered in the order they are asked for.  A slice the buffers do not hold is REFUSED: the first refusal or HIP
// error sticks in `st` and every later request returns null without touching the device, so an entry checks st once, before it launches.
extern "C++" {   // (member templates; this section sits inside the ABI's extern "C" block)
struct Staging {
    struct Back { void* host; const void* dev; size_t bytes; };
    a1mpc_handle h; size_t N; hipStream_t s;
    a1mpc_status st;
    size_t used_in = 0, used_out = 0, used_u8 = 0;   // per robot
    Back backs[12]; int n_backs = 0;   // (a1mpc_command_batch: six in/out arrays and five outputs)
    Staging(a1mpc_handle h_, int32_t n, hipStream_t s_) : h(h_), N(static_cast<size_t>(n)), s(s_), st(ensure_aux(h_)) {}
    void hip(hipError_t e, const char* what) { if (e != hipSuccess) st = fail(A1MPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    void refuse(const char* what) { st = fail(A1MPC_ERR_INVALID_ARGUMENT, std::string("internal: ") + what + " beyond what the handle's staging holds"); }
    void take(double*& d, size_t per_robot) {
        if (used_in + per_robot <= kAuxIn) { d = h->d_aux_in + used_in * N; used_in += per_robot; }
        else if (used_out + per_robot <= kAuxOut) { d = h->d_aux_out + used_out * N; used_out += per_robot; }
        else refuse("a slice of doubles");
    }
    void take(uint8_t*& d, size_t per_robot) {
        if (per_robot <= kAuxU8Slice && used_u8 + kAuxU8Slice <= kAuxU8) { d = h->d_aux_u8 + used_u8 * N; used_u8 += kAuxU8Slice; }
        else refuse("a slice of bytes");
    }
    template <class T> T* slice(size_t per_robot) { T* d = nullptr; if (st == A1MPC_OK) take(d, per_robot); return d; }
    // an input: the slice, filled from `host` (null host: the slice alone -- an input the call does not use)
    template <class T> T* in(const T* host, size_t per_robot) {
        T* d = slice<T>(per_robot);
        if (d && host) hip(hipMemcpyAsync(d, host, N * per_robot * sizeof(T), hipMemcpyHostToDevice, s), "hipMemcpyAsync (staging, host to device)");
        return d;
    }
    // `dev` (per_robot elements per robot) goes back to `host` in finish(); a null host is an output the caller does not want: nothing is copied
    template <class T> void back(T* host, const T* dev, size_t per_robot) {
        if (!host || st != A1MPC_OK) return;
        if (n_backs == static_cast<int>(sizeof backs / sizeof backs[0])) return refuse("an output");
        backs[n_backs++] = Back{host, dev, N * per_robot * sizeof(T)};
    }
    // an output: its slice, or null for a null host (the kernels skip a null optional output)
    template <class T> T* out(T* host, size_t per_robot) { if (!host) return nullptr; T* d = slice<T>(per_robot); back(host, d, per_robot); return d; }
    template <class T> T* inout(T* host, size_t per_robot) { T* d = in(host, per_robot); back(host, d, per_robot); return d; }
    a1mpc_status finish() {   // the outbound copies, then the call's one synchronisation
        for (int k = 0; k < n_backs; ++k) A1_HIP(hipMemcpyAsync(backs[k].host, backs[k].dev, backs[k].bytes, hipMemcpyDeviceToHost, s));
        A1_HIP(hipStreamSynchronize(s));
        return A1MPC_OK;
    }
};
}  // extern "C++"
#define A1_STAGED(sg) do { if ((sg).st != A1MPC_OK) return (sg).st; } while (0)

void a1mpc_default_contact_config(a1mpc_contact_config* c) {
    if (!c) return;
    c->counter_per_swing = 120.0; c->foot_force_low = 30.0; c->use_terrain_adapt = 1;
}
a1mpc_status a1mpc_reset_contact_state(a1mpc_handle h) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->d_ct_state) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);  // the memsets below must not overtake a launch still running on a caller's stream
    A1_HIP(hipMemsetAsync(h->d_ct_state, 0, static_cast<size_t>(h->max_batch) * kCtBytesPerRobot, h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    return A1MPC_OK;
}
a1mpc_status a1mpc_contact_terrain_batch(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* gait_counter,
                                         const uint8_t* plan_contacts, const double* foot_force, const double* foot_pos_abs,
                                         const double* root_pos_z, double* root_euler_d_pitch, uint8_t* contacts_out,
                                         double* foot_pos_recent_contact_out, double* terrain_angle_out) {
    A1_STAGE_BEGIN(cfg && gait_counter && plan_contacts && foot_force && foot_pos_abs && root_pos_z && root_euler_d_pitch && contacts_out &&
                   foot_pos_recent_contact_out && terrain_angle_out, "null config or input/output pointer", nullptr);
    Staging sg(h, n, s);
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    const double *d_gc = sg.in(gait_counter, 4), *d_ff = sg.in(foot_force, 4), *d_fp = sg.in(foot_pos_abs, 12), *d_z = sg.in(root_pos_z, 1);
    double* d_pd = sg.in(root_euler_d_pitch, 1);
    const uint8_t* d_pc = sg.in(plan_contacts, 4);
    uint8_t* d_ct = sg.out(contacts_out, 4);
    double *d_rec = sg.out(foot_pos_recent_contact_out, 12), *d_ta = sg.out(terrain_angle_out, 1);
    sg.back(root_euler_d_pitch, d_pd, 1);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_contact_terrain(make_contact_args(h, *cfg, n, d_gc, d_pc, d_ff, d_fp, d_z, d_pd, d_ct, d_rec, d_ta), s));
    return sg.finish();
}
// the terrain block of compute_grf alone (S/A1RobotControl.cpp:335-376 + compute_walking_surface :566-582): foot_pos_recent_contact comes from the caller's
// A1CtrlStates (the reference fills it in generate_swing_legs_ctrl); the terrain-angle filter of every robot lives in the handle.  Not timed (ev0 / ev1 stay the
// previous call's)
a1mpc_status a1mpc_terrain_batch(a1mpc_handle h, int32_t use_terrain_adapt, int32_t n, const double* foot_pos_recent_contact, const double* root_pos_z,
                                 double* root_euler_d_pitch, double* terrain_angle_out) {
    A1_STAGE_BEGIN(foot_pos_recent_contact && root_pos_z && root_euler_d_pitch && terrain_angle_out, "null input/output pointer", nullptr);
    Staging sg(h, n, s);
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    const double *d_rec = sg.in(foot_pos_recent_contact, 12), *d_z = sg.in(root_pos_z, 1);
    double* d_pd = sg.in(root_euler_d_pitch, 1);
    double* d_ta = sg.out(terrain_angle_out, 1);
    sg.back(root_euler_d_pitch, d_pd, 1);
    A1_STAGED(sg);
    ContactArgs a = make_contact_args(h, a1mpc_contact_config{0.0, 0.0, use_terrain_adapt}, n, nullptr, nullptr, nullptr, nullptr, d_z, d_pd, nullptr, nullptr, d_ta);
    a.recent_in = d_rec;
    launch_contact_terrain(a, s);
    A1_HIP(hipGetLastError());
    A1_MARK(h, s);
    return sg.finish();
}

// ---- N4a: swing-leg targets + foot PD force (S/A1RobotControl.cpp:204-254, Bezier: S/utils/Utils.cpp:64-104), one lane per (robot, leg) ------
struct SwingArgs {
    int32_t n;
    double counter_per_swing, dt, kp[3], kd[3];
    const double *Rz, *foot_pos_abs, *gait_counter, *target_rel;
    double *start, *rel_last, *target_last, *cur_out, *kin_out;
};
// one (robot, leg) of generate_swing_legs_ctrl's first block: gc = the leg's gait counter, target_rel = its foothold (both may come straight from plan_lane's registers)
__device__ __forceinline__ void swing_lane(const SwingArgs& a, const int64_t b, const int i, const double gc, const double (&target_rel)[3], double (&cur)[3], double (&st)[3],
                                           double (&tl)[3], double (&kin)[3]) {
#pragma clang fp contract(off)
    const double* Rz = a.Rz + b * 9;
    const double* fa = a.foot_pos_abs + b * 12 + 3 * i;
    const int64_t o = b * 12 + 3 * i;
#pragma unroll
    for (int r = 0; r < 3; ++r) cur[r] = Rz[0 * 3 + r] * fa[0] + Rz[1 * 3 + r] * fa[1] + Rz[2 * 3 + r] * fa[2];   // :224
    float spline_time = 0.0f;
    if (gc <= a.counter_per_swing) {                                                                                  // :227-232  (foot_pos_start <- the current position)
#pragma unroll
        for (int r = 0; r < 3; ++r) st[r] = cur[r];
    } else {                                                                                                          // :233-236  (foot_pos_start stays: written back as read)
        spline_time = static_cast<float>(gc - a.counter_per_swing) / static_cast<float>(a.counter_per_swing);
#pragma unroll
        for (int r = 0; r < 3; ++r) st[r] = a.start[o + r];
    }
    const double t = spline_time, u = 1 - t;
    const double t2 = t * t, t3 = t2 * t, t4 = t2 * t2, u2 = u * u, u3 = u2 * u, u4 = u2 * u2;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fin = target_rel[r];
        double P1 = st[r], P2 = fin;
        if (r == 2) { P1 += 0.0f; P2 += 0.4f + 0.5 * 0.0; }                                                           // FOOT_SWING_CLEARANCE1 / 2
        double y = 0;                                                                                                 // Utils.cpp:97-104
        y += 1.0 * 1.0 * u4 * st[r];
        y += 4.0 * t * u3 * P1;
        y += 6.0 * t2 * u2 * P2;
        y += 4.0 * t3 * u * fin;
        y += 1.0 * t4 * 1.0 * fin;
        const double vel_cur = (cur[r] - a.rel_last[o + r]) / a.dt;                                                   // :243-252
        const double vel_tgt = (y - a.target_last[o + r]) / a.dt;
        tl[r] = y;
        kin[r] = (y - cur[r]) * a.kp[r] + (vel_tgt - vel_cur) * a.kd[r];
    }
}
__global__ __launch_bounds__(256) void a1mpc_swing_kernel(const SwingArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double stage[4][576];
    const int lane = static_cast<int>(threadIdx.x) & 63, wv = static_cast<int>(threadIdx.x) >> 6;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int i = static_cast<int>(gid & 3);
    const int64_t wave_first = (static_cast<int64_t>(blockIdx.x) * 256 + wv * 64) >> 2;
    if (wave_first >= a.n) return;
    const WaveStage ws{stage[wv], lane, static_cast<int>(a.n - wave_first < 16 ? a.n - wave_first : 16), wave_first};
    double cur[3] = {0, 0, 0}, st[3] = {0, 0, 0}, tl[3] = {0, 0, 0}, kin[3] = {0, 0, 0};
    if (b < a.n) {
        const double tr[3] = {a.target_rel[b * 12 + 3 * i], a.target_rel[b * 12 + 3 * i + 1], a.target_rel[b * 12 + 3 * i + 2]};
        swing_lane(a, b, i, a.gait_counter[b * 4 + i], tr, cur, st, tl, kin);
    }
    // start / rel_last / target_last are updated in place, and a staged store writes OTHER lanes' words of this wavefront's 16 robots (no other wavefront touches
    // these robots).  Every load above must have returned before the first such store: an explicit s_waitcnt vmcnt(0) -- rel_last / target_last only feed `kin`, which
    // is parked in the SECOND flush, so the first flush's data dependences alone would not cover them
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
    ws.flush3(st, cur, tl, a.start, a.rel_last, a.target_last);   // foot_pos_start, foot_pos_rel_last_time <- cur, foot_pos_target_last_time <- y
    ws.flush3(kin, cur, cur, a.kin_out, a.cur_out, nullptr);
}
// a1mpc_control_tick_device: update_plan and the swing-leg block in ONE launch -- both run one lane per (robot, leg), and the swing block's inputs from the plan (the
// leg's new gait counter and foothold) are the lane's own registers.  Same lane functions as the two kernels: same bits, one launch less per tick.
__global__ __launch_bounds__(256) void a1mpc_plan_swing_kernel(const PlanArgs pa, const SwingArgs sa) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double stage[4][576];
    const int lane = static_cast<int>(threadIdx.x) & 63, wv = static_cast<int>(threadIdx.x) >> 6;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int leg = static_cast<int>(gid & 3);
    const int64_t wave_first = (static_cast<int64_t>(blockIdx.x) * 256 + wv * 64) >> 2;
    if (wave_first >= pa.n) return;
    const WaveStage ws{stage[wv], lane, static_cast<int>(pa.n - wave_first < 16 ? pa.n - wave_first : 16), wave_first};
    double rel[3] = {0, 0, 0}, ab[3] = {0, 0, 0}, wo[3] = {0, 0, 0}, gc = 0.0;
    double cur[3] = {0, 0, 0}, st[3] = {0, 0, 0}, tl[3] = {0, 0, 0}, kin[3] = {0, 0, 0};
    if (b < pa.n) {
        plan_lane(pa, b, leg, gc, rel, ab, wo);
        swing_lane(sa, b, leg, gc, rel, cur, st, tl, kin);
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): every load of the in-place arrays has returned before the staged stores write other lanes' words of them (see a1mpc_swing_kernel)
    ws.flush3(rel, ab, wo, pa.rel, pa.abs_, pa.world);
    ws.flush3(st, cur, tl, sa.start, sa.rel_last, sa.target_last);
    ws.flush3(kin, cur, cur, sa.kin_out, sa.cur_out, nullptr);
}

static SwingArgs make_swing_args(int32_t n, double counter_per_swing, double dt, const double* kp_foot, const double* kd_foot, const double* R_z, const double* foot_pos_abs,
                                 const double* gait_counter, const double* foot_pos_target_rel, double* foot_pos_start, double* foot_pos_rel_last_time,
                                 double* foot_pos_target_last_time, double* foot_pos_cur_out, double* foot_forces_kin_out) {
    SwingArgs a;
    a.n = n; a.counter_per_swing = counter_per_swing; a.dt = dt;
    for (int k = 0; k < 3; ++k) { a.kp[k] = kp_foot[k]; a.kd[k] = kd_foot[k]; }
    a.Rz = R_z; a.foot_pos_abs = foot_pos_abs; a.gait_counter = gait_counter; a.target_rel = foot_pos_target_rel; a.start = foot_pos_start;
    a.rel_last = foot_pos_rel_last_time; a.target_last = foot_pos_target_last_time; a.cur_out = foot_pos_cur_out; a.kin_out = foot_forces_kin_out;
    return a;
}
static void launch_swing(const SwingArgs& a, hipStream_t s) { hipLaunchKernelGGL(a1mpc_swing_kernel, leg_lane_grid(a.n), dim3(256), 0, s, a); }

a1mpc_status a1mpc_swing_legs_batch(a1mpc_handle h, int32_t n, double counter_per_swing, double dt, const double* R_z,
                                    const double* foot_pos_abs, const double* gait_counter, const double* foot_pos_target_rel,
                                    const double* kp_foot, const double* kd_foot, double* foot_pos_start, double* foot_pos_rel_last_time,
                                    double* foot_pos_target_last_time, double* foot_pos_cur_out, double* foot_forces_kin_out) {
    A1_STAGE_BEGIN(R_z && foot_pos_abs && gait_counter && foot_pos_target_rel && kp_foot && kd_foot && foot_pos_start && foot_pos_rel_last_time &&
                   foot_pos_target_last_time && foot_pos_cur_out && foot_forces_kin_out && dt > 0, "null input/output pointer or dt <= 0", nullptr);
    Staging sg(h, n, s);
    const double *d_Rz = sg.in(R_z, 9), *d_fa = sg.in(foot_pos_abs, 12), *d_gc = sg.in(gait_counter, 4), *d_tr = sg.in(foot_pos_target_rel, 12);
    double *d_st = sg.inout(foot_pos_start, 12), *d_rl = sg.inout(foot_pos_rel_last_time, 12), *d_tl = sg.inout(foot_pos_target_last_time, 12);
    double *d_cur = sg.out(foot_pos_cur_out, 12), *d_kin = sg.out(foot_forces_kin_out, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_swing(make_swing_args(n, counter_per_swing, dt, kp_foot, kd_foot, d_Rz, d_fa, d_gc, d_tr, d_st, d_rl, d_tl, d_cur, d_kin), s));
    return sg.finish();
}

// ---- N4b: leg kinematics (S/GazeboA1ROS.cpp:264-279, A1Kinematics fk / jac restated from the leg model), one lane per (robot, leg) -----------
struct LegArgs {
    int32_t n;
    double rho_fix[20], rho_opt[12];
    const double *q, *qd, *R, *pos, *vel;
    double *rel, *Jb, *vrel, *pabs, *vabs, *pworld, *vworld;
};
// Round 4: the outputs (9 + 6 x 3 doubles per lane at strides of 72 / 24 bytes between lanes) leave through the wave's LDS stage (WaveStage): 64 consecutive doubles per
// store instruction instead of 36 / 12 cache lines touched for 512 bytes; 0.213 -> 0.106 ms at 524 288 robots, bit-identical.
__global__ __launch_bounds__(256) void a1mpc_leg_kernel(const LegArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double stage[4][576];
    const int lane = static_cast<int>(threadIdx.x) & 63, wv = static_cast<int>(threadIdx.x) >> 6;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int i = static_cast<int>(gid & 3);
    const int64_t wave_first = (static_cast<int64_t>(blockIdx.x) * 256 + wv * 64) >> 2;     // first robot of this wavefront
    if (wave_first >= a.n) return;
    const int wave_robots = static_cast<int>(a.n - wave_first < 16 ? a.n - wave_first : 16);
    const bool live = b < a.n;
    double p[3] = {0, 0, 0}, v[3] = {0, 0, 0}, J[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pa[3] = {0, 0, 0}, va[3] = {0, 0, 0}, pw[3] = {0, 0, 0}, vw[3] = {0, 0, 0};
    if (live) {
        const double *q = a.q + b * 12 + 3 * i, *qd = a.qd + b * 12 + 3 * i, *f = a.rho_fix + 5 * i, *o = a.rho_opt + 3 * i;
        const double ox = f[0], oy = f[1], L = f[2] + o[1], lt = f[3], al = f[4] - o[2], r0 = o[0];
        const double s0 = sin(q[0]), c0 = cos(q[0]), s1 = sin(q[1]), c1 = cos(q[1]), s12 = sin(q[1] + q[2]), c12 = cos(q[1] + q[2]);
        const double Xq = r0 * c12 - al * s12, Zq = -(al * c12) - r0 * s12;
        const double Xr = Xq - lt * s1, Zp = Zq - lt * c1;
        p[0] = ox + Xr; p[1] = oy + (L * c0 - Zp * s0); p[2] = L * s0 + Zp * c0;
        J[0] = 0.0; J[1] = -p[2]; J[2] = p[1] - oy; J[3] = Zp; J[4] = s0 * Xr; J[5] = -(c0 * Xr); J[6] = Zq; J[7] = s0 * Xq; J[8] = -(c0 * Xq);
#pragma unroll
        for (int r = 0; r < 3; ++r) v[r] = J[r] * qd[0] + J[3 + r] * qd[1] + J[6 + r] * qd[2];
        const double* R = a.R + b * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            pa[r] = R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2];
            va[r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2];
            pw[r] = pa[r] + a.pos[b * 3 + r];
            vw[r] = va[r] + a.vel[b * 3 + r];
        }
    }
    const WaveStage ws{stage[wv], lane, wave_robots, wave_first};
    double* sg = stage[wv];
    // J blocks: lane (robot, leg) holds doubles [9 lane, 9 lane + 9) of the wave's 576
#pragma unroll
    for (int k = 0; k < 9; ++k) sg[9 * lane + k] = J[k];
    WaveStage::sync();
    {
        double* out = a.Jb + wave_first * 36;
        const int cnt = wave_robots * 36;
#pragma unroll
        for (int m = 0; m < 9; ++m) { const int e = lane + 64 * m; if (e < cnt) out[e] = sg[e]; }
    }
    WaveStage::sync();
    ws.flush3(p, v, pa, a.rel, a.vrel, a.pabs);
    ws.flush3(va, pw, vw, a.vabs, a.pworld, a.vworld);
}

// (the five outputs after j_foot_blocks are optional: null = not wanted)
static void launch_leg(int32_t n, const double* rho_fix, const double* rho_opt, const double* joint_pos, const double* joint_vel, const double* R_world, const double* root_pos,
                       const double* root_lin_vel, double* foot_pos_rel_out, double* j_foot_blocks_out, double* foot_vel_rel_out, double* foot_pos_abs_out,
                       double* foot_vel_abs_out, double* foot_pos_world_out, double* foot_vel_world_out, hipStream_t s) {
    LegArgs a;
    a.n = n;
    std::memcpy(a.rho_fix, rho_fix, sizeof a.rho_fix); std::memcpy(a.rho_opt, rho_opt, sizeof a.rho_opt);
    a.q = joint_pos; a.qd = joint_vel; a.R = R_world; a.pos = root_pos; a.vel = root_lin_vel; a.rel = foot_pos_rel_out; a.Jb = j_foot_blocks_out;
    a.vrel = foot_vel_rel_out; a.pabs = foot_pos_abs_out; a.vabs = foot_vel_abs_out; a.pworld = foot_pos_world_out; a.vworld = foot_vel_world_out;
    hipLaunchKernelGGL(a1mpc_leg_kernel, leg_lane_grid(n), dim3(256), 0, s, a);
}

a1mpc_status a1mpc_leg_state_batch(a1mpc_handle h, int32_t n, const double* joint_pos, const double* joint_vel, const double* R_world,
                                   const double* root_pos, const double* root_lin_vel, const double* rho_fix, const double* rho_opt,
                                   double* foot_pos_rel_out, double* j_foot_blocks_out, double* foot_vel_rel_out, double* foot_pos_abs_out,
                                   double* foot_vel_abs_out, double* foot_pos_world_out, double* foot_vel_world_out) {
    A1_STAGE_BEGIN(joint_pos && joint_vel && R_world && root_pos && root_lin_vel && rho_fix && rho_opt && foot_pos_rel_out && j_foot_blocks_out,
                   "null input/output pointer", nullptr);
    Staging sg(h, n, s);
    const double *d_q = sg.in(joint_pos, 12), *d_qd = sg.in(joint_vel, 12), *d_R = sg.in(R_world, 9), *d_pos = sg.in(root_pos, 3), *d_vel = sg.in(root_lin_vel, 3);
    double *d_rel = sg.out(foot_pos_rel_out, 12), *d_Jb = sg.out(j_foot_blocks_out, 36), *d_vrel = sg.out(foot_vel_rel_out, 12), *d_pabs = sg.out(foot_pos_abs_out, 12);
    double *d_vabs = sg.out(foot_vel_abs_out, 12), *d_pw = sg.out(foot_pos_world_out, 12), *d_vw = sg.out(foot_vel_world_out, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_leg(n, rho_fix, rho_opt, d_q, d_qd, d_R, d_pos, d_vel, d_rel, d_Jb, d_vrel, d_pabs, d_vabs, d_pw, d_vw, s));
    return sg.finish();
}

// ---- N4c: A1BasicEKF (S/A1BasicEKF.cpp), 32 lanes per robot, two robots per wavefront -----------------------------------------------
// Lane r owns row r of every matrix (18 state rows, 28 measurement rows); rows meet through the robot's LDS image (P, Pbar, S / S^-1 C, the
// pivot row of the elimination).  The arithmetic follows the dense products of the reference term for term (inner index ascending, the
// exact zeros of A, B, C dropped), no FMA contraction, so the result is bit-identical to the oracle's dense restatement.
constexpr int kEkfState = 18 + 18 * 18 + 1;
struct EkfArgs {
    int32_t n;
    double dt;
    int32_t flat;
    double* state;
    const uint8_t* mode;
    const double *ff, *R, *acc, *w, *fk, *fv;
    double *pos_out, *vel_out;
    uint8_t* ec_out;
};
__global__ __launch_bounds__(256) void a1mpc_ekf_init_kernel(const EkfArgs a) {  // init_state :54-68 for robots whose filter is new
#pragma clang fp contract(off)
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (b >= a.n) return;
    double* st = a.state + b * kEkfState;
    if (st[18 + 324] != 0.0) return;
    double *x = st, *P = st + 18;
    for (int i = 0; i < 324; ++i) P[i] = 0.0;
    for (int i = 0; i < 18; ++i) { P[i * 18 + i] = 1.0 * 3; x[i] = 0.0; }
    x[2] = 0.09;
    const double* R = a.R + b * 9; const double* fk = a.fk + b * 12;
    for (int i = 0; i < 4; ++i)
        for (int r = 0; r < 3; ++r) x[6 + i * 3 + r] = (R[3 * r] * fk[3 * i] + R[3 * r + 1] * fk[3 * i + 1] + R[3 * r + 2] * fk[3 * i + 2]) + x[r];
    st[18 + 324] = 2.0;  // initialised in THIS call: the update kernel turns it into 1 and leaves the robot alone
    for (int r = 0; r < 3; ++r) { a.pos_out[b * 3 + r] = x[r]; a.vel_out[b * 3 + r] = x[3 + r]; }
    for (int i = 0; i < 4; ++i) a.ec_out[b * 4 + i] = 0;
}
__device__ inline void half_sync() {  // orders LDS traffic between the lanes of a wavefront (see row_sync)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// column list of C's row r: up to two (column, sign) pairs in ascending column order
__device__ inline void ekf_c_row(int r, int& c0, double& s0, int& c1, double& s1) {
    c1 = -1; s1 = 0.0;
    if (r < 12) { c0 = r % 3; s0 = -1.0; c1 = 6 + r; s1 = 1.0; }            // -pos + foot
    else if (r < 24) { c0 = 3 + (r - 12) % 3; s0 = 1.0; }                    // vel
    else { c0 = 6 + (r - 24) * 3 + 2; s0 = 1.0; }                            // foot height
}
// ONE arithmetic, round 6: the measurement update never forms S^-1.  S = L D L' by forward elimination without pivoting (S is symmetric positive definite), the
// right-hand sides [C Pbar | error_y] ride along, and with Y = L^-1 [C Pbar | error_y]
//     x = xbar + Y_P' D^-1 y_e,      P = Pbar - Y_P' D^-1 Y_P                                                                  (:134-139)
// -- nothing is solved backwards, and the four dense products behind the explicit inverse (S^-1 error_y, S^-1 C, Pbar C' (S^-1 C), (..) Pbar) are one 28-term
// rank update.  A third of the inverse's arithmetic, and closer to an 80-bit evaluation of the filter than the explicit inverse is (state 9.8e-15 against 7.3e-14,
// covariance 1.0e-15 against 1.0e-12 per tick: the CPU suite measures it).  Until round 6: in-place Gauss-Jordan sweeps to -S^-1 (2 x 28^3 multiply-adds per robot) with the
// pivot column exchanged through LDS, two residencies of it (profiles/r05_ekf_residency.txt).
// No LDS in the elimination.  A robot is two DPP rows of 16 lanes; lane i holds ROW i of S (M[28]) and COLUMN i of the right-hand sides (B[28]: column c < 18 of C Pbar,
// column 18 = error_y).  Step k, p = a_kk:  f_i = a_ik / p,  a_ij -= f_i a_jk (j > k);  t_c = b_kc / p,  b_ic -= a_ik t_c (i > k).  a_jk and a_ik live in lanes j and i: the column reaches
// the lane that needs it as the DPP source of a v_fmac_f64_dpp (row_newbcast), after one v_permlane16_swap pair has put each 16-lane half of it on both rows of the
// robot (ekf_rows) -- one exchange per step serves both updates.  The pivot row is taken from COLUMN k as the other lanes hold it (a_jk for a_kj): only entries of the lower triangle ever feed another entry, so this
// is the standard right-looking L D L' and the upper triangle a lane drags along is never read.  Rows / columns that are done keep executing the updates on dead
// registers (no branch inside a step).  The rank update reads y_rb from lane b the same way.  (First cut of this round: rows of Y published to LDS by the pivot lane,
// 10 masked 16-byte stores per step -- 40 % fewer VALU instructions than the inverse and SLOWER, 0.59 ms per 65 536 robots against 0.49: every multiply-add took a fresh
// broadcast operand from LDS and the CU's one LDS served four SIMDs, profiles/r06_ekf_ldl.md.)  oracle/a1mpc_oracle.c ekf_step_impl(device = 1) is the same
// arithmetic in the same order.
extern "C++" {   // (this section sits inside the ABI's extern "C" block)
template <int I, int N, class F>
__device__ __forceinline__ void ekf_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); ekf_for<I + 1, N>(f); }
}
// (ua, ub) <- x:  ua = the lanes of the robot's EVEN row of x on both of its rows, ub = the odd row's (v_permlane16_swap: odd rows of vdst <-> even rows of src)
__device__ __forceinline__ void ekf_rows(double x, double& ua, double& ub) {
    double c0, c1;
    asm("v_mov_b64 %0, %2\n"
        "v_mov_b64 %1, %2\n"
        "s_nop 1" : "=&v"(c0), "=&v"(c1) : "v"(x));   // (VALU write -> v_permlane16_swap read: 2 wait states, which hipcc cannot see behind an asm statement)
    const unsigned long long b0 = __builtin_bit_cast(unsigned long long, c0), b1 = __builtin_bit_cast(unsigned long long, c1);
    const auto r0 = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(b0), static_cast<unsigned>(b1), false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(b0 >> 32), static_cast<unsigned>(b1 >> 32), false, false);
    ua = __builtin_bit_cast(double, static_cast<unsigned long long>(r0[0]) | (static_cast<unsigned long long>(r1[0]) << 32));
    ub = __builtin_bit_cast(double, static_cast<unsigned long long>(r0[1]) | (static_cast<unsigned long long>(r1[1]) << 32));
    asm volatile("s_nop 1" : "+v"(ua), "+v"(ub));     // (VALU write -> DPP read: 2 wait states; the DPP reads below sit inside asm statements)
}
template <int L>
__device__ __forceinline__ double ekf_bcast(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + L, 0xF, 0xF, true); }   // row_newbcast:L
// acc += m * (lane L of my row's x)  /  acc -= ..  as ONE instruction (v_fmac_f64 is the only FP64 arithmetic with a DPP form)
template <int L>
__device__ __forceinline__ void ekf_fma(double& acc, double m, double x) {
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(m), "n"(L));
}
template <int L>
__device__ __forceinline__ void ekf_fnma(double& acc, double m, double x) {
    asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(m), "n"(L));
}
constexpr int kEkfLds = 324 + 16 + 18 + 18 + 28;   // doubles per robot: Pbar (+ 16 words that idle lanes read past it), x, xbar, error_y: 3.2 KB
__device__ __forceinline__ void ekf_update_robot(const EkfArgs& a, double* __restrict__ lds_g, const int g, const int l) {
#pragma clang fp contract(off)
    const int64_t b = static_cast<int64_t>(blockIdx.x) * 2 + g;
    if (b >= a.n) return;
    double* st = a.state + b * kEkfState;
    double *Pb = lds_g, *xs = Pb + 324 + 16, *xb = xs + 18, *zs = xb + 18;
    const double dt = a.dt;
    // Every global load of the tick is issued here, before the first use of any of them: ONE exposure to the memory latency per robot.  (Until round 6 the loads sat where
    // they were used, behind the lane-dependent branches of the process update and of the measurement vector -- 18 pairs of row loads each waited for on its own, the
    // contact inputs behind the flag: half of a wavefront's life was spent parked at s_waitcnt, SQ_WAIT_ANY / SQ_WAVE_CYCLES = 0.49, profiles/r06_ekf_ldl.md.)
    const double* Pg = st + 18;  // P of the previous tick: lane i < 18 reads row i (and row 3 + i for i < 3: A P) straight from global memory
    const int rowA = l < 18 ? l : 0, rowB = l < 3 ? 3 + l : rowA;
    const int r = l < 28 ? l : 27;                                       // my row of S / C (lanes 28 - 31 idle along on row 27's inputs)
    const int leg = r < 24 ? (r % 12) / 3 : r - 24, cr = l % 3;         // the leg my measurement row belongs to; my component (process rows 3 - 5 and measurement rows alike)
    const double flag = st[18 + 324];
    double Pa[18], Pc[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) { Pa[j] = Pg[rowA * 18 + j]; Pc[j] = Pg[rowB * 18 + j]; }
    const double xl = st[rowA];
    const int mode = a.mode[b];
    double ffv[4], accv[3], wv[3], Rc[3], f[3], v[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) ffv[i] = a.ff[b * 4 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { accv[i] = a.acc[b * 3 + i]; wv[i] = a.w[b * 3 + i]; Rc[i] = a.R[b * 9 + 3 * cr + i]; f[i] = a.fk[b * 12 + 3 * leg + i]; v[i] = a.fv[b * 12 + 3 * leg + i]; }
    // (a robot whose filter was initialised in THIS call -- flag 2 -- or never -- flag 0 -- runs through the arithmetic on whatever its state holds and stores nothing: the
    // flag is looked at where the results leave, so its load is not a round trip of its own ahead of the others)
    if (l < 18) xs[l] = xl;
    double ec[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ec[i] = mode == 0 ? 1.0 : fmin(fmax(ffv[i] / (100.0 - 0.0), 0.0), 1.0);   // :79-86
    const double PIMU = 0.01, VIMU = 0.01, PFOOT = 0.01, S_PIMU_REL = 0.001, S_VIMU_REL = 0.1, S_ZFOOT = 0.001;       // A1BasicEKF.h:15-20
    half_sync();
    // ---- process update (:72-112): xbar = A x + B u, Pbar = A P A' + Q; lane i < 18 owns row i
    double xbv = 0.0;
    if (l < 18) {
        if (l < 3) xbv = (xl + dt * xs[3 + l]) + 0.0;
        else if (l < 6) { const double u = (Rc[0] * accv[0] + Rc[1] * accv[1] + Rc[2] * accv[2]) + (cr == 2 ? -9.81 : 0.0); xbv = xl + dt * u; }
        else xbv = xl + 0.0;
        xb[l] = xbv;
        double T[18];
#pragma unroll
        for (int j = 0; j < 18; ++j) T[j] = l < 3 ? Pa[j] + dt * Pc[j] : Pa[j];
        double q;
        if (l < 3) q = PIMU * dt / 20.0; else if (l < 6) q = VIMU * dt * 9.8 / 20.0; else q = (1 + (1 - ec[(l - 6) / 3]) * 1e3) * dt * PFOOT;
#pragma unroll
        for (int j = 0; j < 18; ++j) Pb[l * 18 + j] = (j < 3 ? T[j] + T[3 + j] * dt : T[j]) + (j == l ? q : 0.0);
    }
    half_sync();
    // ---- innovation (:115-131): lane r < 28 owns row r of S and its error_y entry
    double M[28];
#pragma unroll
    for (int c = 0; c < 28; ++c) M[c] = 0.0;
    if (l < 28) {
        int c0, c1; double s0, s1;
        ekf_c_row(r, c0, s0, c1, s1);
        const double yhat = c1 >= 0 ? s0 * xb[c0] + s1 * xb[c1] : s0 * xb[c0];
        // the three kinds of measurement rows, each evaluated by every lane on its own leg / component and selected (the same operations as a branch per kind would do)
        const double ecl = leg == 0 ? ec[0] : (leg == 1 ? ec[1] : (leg == 2 ? ec[2] : ec[3]));
        const double wgt = 1 + (1 - ecl) * 1e3;
        const double y_pos = Rc[0] * f[0] + Rc[1] * f[1] + Rc[2] * f[2];
        const double wx = wv[0], wy = wv[1], wz = wv[2];
        const double sk0 = 0.0 * f[0] + -wz * f[1] + wy * f[2], sk1 = wz * f[0] + 0.0 * f[1] + -wx * f[2], sk2 = -wy * f[0] + wx * f[1] + 0.0 * f[2];
        const double lv0 = -v[0] - sk0, lv1 = -v[1] - sk1, lv2 = -v[2] - sk2;
        const double rl = Rc[0] * lv0 + Rc[1] * lv1 + Rc[2] * lv2;
        const double y_vel = (1.0 - ecl) * xs[3 + cr] + ecl * rl;
        const double y_z = (1.0 - ecl) * (xs[2] + f[2]) + ecl * 0;
        const double y = r < 12 ? y_pos : (r < 24 ? y_vel : y_z);
        const double rd = r < 12 ? wgt * S_PIMU_REL : (r < 24 ? wgt * S_VIMU_REL : (a.flat ? (1 + (1 - ecl) * 1e3) * S_ZFOOT : 1e5));
        double CP[18];   // my row of C Pbar
#pragma unroll
        for (int j = 0; j < 18; ++j) CP[j] = c1 >= 0 ? s0 * Pb[c0 * 18 + j] + s1 * Pb[c1 * 18 + j] : s0 * Pb[c0 * 18 + j];
#pragma unroll
        for (int c = 0; c < 28; ++c) {
            int d0, d1; double t0, t1;
            ekf_c_row(c, d0, t0, d1, t1);
            const double vv = d1 >= 0 ? CP[d0] * t0 + CP[d1] * t1 : CP[d0] * t0;
            M[c] = vv + (c == r ? rd : 0.0);
        }
        zs[r] = y - yhat;   // error_y: column 18 of the right-hand sides, which lane 18 collects below
        // :131  S <- (S + S') / 2.  S[c][l], the entry lane c holds, is recomputed here from Pbar by lane c's own operations (C row of c times Pbar, then my C row)
#pragma unroll
        for (int c = 0; c < 28; ++c) {
            int e0, e1; double u0, u1;
            ekf_c_row(c, e0, u0, e1, u1);
            const double cp0 = e1 >= 0 ? u0 * Pb[e0 * 18 + c0] + u1 * Pb[e1 * 18 + c0] : u0 * Pb[e0 * 18 + c0];
            const double cp1 = c1 >= 0 ? (e1 >= 0 ? u0 * Pb[e0 * 18 + c1] + u1 * Pb[e1 * 18 + c1] : u0 * Pb[e0 * 18 + c1]) : 0.0;
            const double tr = (c1 >= 0 ? cp0 * s0 + cp1 * s1 : cp0 * s0) + 0.0;   // (+ 0.0: lane c added its "not the diagonal" zero)
            M[c] = c == l ? 0.5 * (M[c] + M[c]) : (c > l ? 0.5 * (M[c] + tr) : 0.5 * (tr + M[c]));
        }
    }
    half_sync();
    // the right-hand sides, a COLUMN per lane: B[r] = (C Pbar)[r][l] for l < 18 (row r of C has one or two entries: known at compile time), error_y[r] on lane 18
    double B[28];
    ekf_for<0, 28>([&](auto Rr) {
        constexpr int r = decltype(Rr)::value;
        constexpr int c0 = r < 12 ? r % 3 : (r < 24 ? 3 + (r - 12) % 3 : 6 + (r - 24) * 3 + 2);   // (ekf_c_row, as constants)
        double v;
        if constexpr (r < 12) v = -1.0 * Pb[c0 * 18 + l] + 1.0 * Pb[(6 + r) * 18 + l];
        else v = 1.0 * Pb[c0 * 18 + l];
        B[r] = l < 18 ? v : (l == 18 ? zs[r] : 0.0);
    });
    // ---- L D L' with the right-hand sides riding along (see the header of this section); every lane of the robot executes every instruction
    double D = 0.0;   // 1 / d_r on lane r
    ekf_for<0, 28>([&](auto K) {
        constexpr int k = decltype(K)::value;
        double ua, ub;
        ekf_rows(M[k], ua, ub);                                    // column k of the trailing matrix: a_jk on lane j
        const double pinv = 1.0 / ekf_bcast<k % 16>(k < 16 ? ua : ub);
        D = l == k ? pinv : D;
        if constexpr (k < 27) {
            const double f = M[k] * pinv, t = B[k] * pinv;   // f_i = a_ik / p on lane i (my row's multiplier);  t_c = b_kc / p on lane c (my column of the scaled pivot row)
            ekf_for<k + 1, 28>([&](auto J) { constexpr int j = decltype(J)::value; ekf_fnma<j % 16>(M[j], f, j < 16 ? ua : ub); });   // a_ij -= f_i a_jk
            ekf_for<k + 1, 28>([&](auto I) { constexpr int i = decltype(I)::value; ekf_fnma<i % 16>(B[i], t, i < 16 ? ua : ub); });   // b_ic -= a_ik t_c: the column serves both updates
        }
    });
    // ---- measurement update (:134-140): lane a < 18 owns row a of  Y_P' D^-1 [Y_P | y_e]  (the sums run over r = 0 .. 27 in ascending order); y_rb comes from lane b
    double G[19];
#pragma unroll
    for (int j = 0; j < 19; ++j) G[j] = 0.0;
    {
        double da, db;
        ekf_rows(D, da, db);
        ekf_for<0, 28>([&](auto Rr) {
            constexpr int r = decltype(Rr)::value;
            const double wr = B[r] * ekf_bcast<r % 16>(r < 16 ? da : db);
            double va, vb;
            ekf_rows(B[r], va, vb);
            ekf_for<0, 19>([&](auto Cc) { constexpr int c = decltype(Cc)::value; ekf_fma<c % 16>(G[c], wr, c < 16 ? va : vb); });
        });
    }
    double Tn[18], xnew = 0.0;
    if (l < 18) {
        xnew = xbv + G[18];
#pragma unroll
        for (int j = 0; j < 18; ++j) Tn[j] = Pb[l * 18 + j] - G[j];
    }
    half_sync();  // every lane is done reading Pbar: its region now stages the unsymmetrised update for the transposed read
    double* Pm = Pb;
    if (l < 18)
        for (int j = 0; j < 18; ++j) Pm[l * 18 + j] = Tn[j];
    half_sync();
    const bool live = flag == 1.0;
    if (l == 0 && flag == 2.0) st[18 + 324] = 1.0;   // initialised in this call: an ordinary robot from the next tick on
    if (l < 18 && live) {
        double Pn[18];
        for (int j = 0; j < 18; ++j) Pn[j] = 0.5 * (Tn[j] + Pm[j * 18 + l]);                                       // :140
        const double p00 = 0.5 * (Pm[0] + Pm[0]), p01 = 0.5 * (Pm[1] + Pm[18]), p10 = 0.5 * (Pm[18] + Pm[1]), p11 = 0.5 * (Pm[19] + Pm[19]);
        if (p00 * p11 - p01 * p10 > 1e-6) {                                                                         // :143-147
            for (int j = 0; j < 18; ++j) {
                if (l < 2 && j >= 2) Pn[j] = 0.0;
                if (l >= 2 && j < 2) Pn[j] = 0.0;
                if (l < 2 && j < 2) Pn[j] /= 10.0;
            }
        }
        for (int j = 0; j < 18; ++j) st[18 + l * 18 + j] = Pn[j];
        st[l] = xnew;
        if (l < 3) a.pos_out[b * 3 + l] = xnew; else if (l < 6) a.vel_out[b * 3 + l - 3] = xnew;
    }
    if (l < 4 && live) a.ec_out[b * 4 + l] = ec[l] < 0.5 ? 0 : 1;                                                   // :151-157
}
}  // extern "C++"
__global__ __launch_bounds__(64, 3) void a1mpc_ekf_kernel(const EkfArgs a) {
    __shared__ __attribute__((aligned(16))) double lds[2][kEkfLds];
    const int g = static_cast<int>(threadIdx.x) >> 5;
    ekf_update_robot(a, lds[g], g, static_cast<int>(threadIdx.x) & 31);
}
static void launch_ekf_update(const EkfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(a1mpc_ekf_kernel, dim3(static_cast<unsigned>((a.n + 1) / 2)), dim3(64), 0, s, a);
}
#define EKF_LAUNCH(a) launch_ekf_update(a, 0)   // (tools/ubench/ekf_bench.py cuts this section into a stand-alone timing harness)

a1mpc_status a1mpc_reset_ekf_state(a1mpc_handle h) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->d_ekf_state) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);  // the memsets below must not overtake a launch still running on a caller's stream
    A1_HIP(hipMemsetAsync(h->d_ekf_state, 0, static_cast<size_t>(h->max_batch) * kEkfState * sizeof(double), h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    h->ekf_ready_n = 0;
    return A1MPC_OK;
}
// the handle's filter state, allocated on first use (zero = not initialised: a1mpc_ekf_init_kernel)
static a1mpc_status ensure_ekf_state(a1mpc_handle h, hipStream_t s) {
    if (h->d_ekf_state) return A1MPC_OK;
    A1_HIP(hipMalloc(&h->d_ekf_state, static_cast<size_t>(h->max_batch) * kEkfState * sizeof(double)));
    A1_HIP(hipMemsetAsync(h->d_ekf_state, 0, static_cast<size_t>(h->max_batch) * kEkfState * sizeof(double), s));
    return A1MPC_OK;
}
// the init kernel for robots that have not been through it, then the update kernel (whose launch status is the caller's to read)
static a1mpc_status launch_ekf(a1mpc_handle h, int32_t n, double dt, int32_t assume_flat_ground, const uint8_t* movement_mode, const double* foot_force, const double* R_world,
                               const double* imu_acc, const double* imu_ang_vel, const double* foot_pos_rel, const double* foot_vel_rel, double* root_pos_out,
                               double* root_lin_vel_out, uint8_t* estimated_contacts_out, hipStream_t s) {
    EkfArgs a;
    a.n = n; a.dt = dt; a.flat = assume_flat_ground; a.state = h->d_ekf_state; a.mode = movement_mode; a.ff = foot_force; a.R = R_world; a.acc = imu_acc;
    a.w = imu_ang_vel; a.fk = foot_pos_rel; a.fv = foot_vel_rel; a.pos_out = root_pos_out; a.vel_out = root_lin_vel_out; a.ec_out = estimated_contacts_out;
    if (n > h->ekf_ready_n) {   // (robots 0 .. ekf_ready_n - 1 have been through init_state: nothing for the init kernel to do -- one launch less per tick)
        hipLaunchKernelGGL(a1mpc_ekf_init_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 255) / 256)), dim3(256), 0, s, a);
        if (hipError_t ei = hipGetLastError(); ei != hipSuccess) { h->ekf_ready_n = 0; return fail(A1MPC_ERR_HIP, std::string("a1mpc_ekf_init_kernel: ") + hipGetErrorString(ei)); }
        h->ekf_ready_n = n;   // (only once the launch has been accepted -- ADVICE r5: a failed init launch must not leave the robots marked as initialised)
    }
    launch_ekf_update(a, s);
    return A1MPC_OK;
}
#define A1_LAUNCH_EKF(...) if (a1mpc_status se_ = launch_ekf(__VA_ARGS__); se_ != A1MPC_OK) return se_

a1mpc_status a1mpc_ekf_update_batch(a1mpc_handle h, int32_t n, double dt, int32_t assume_flat_ground, const uint8_t* movement_mode,
                                    const double* foot_force, const double* R_world, const double* imu_acc, const double* imu_ang_vel,
                                    const double* foot_pos_rel, const double* foot_vel_rel, double* root_pos_out, double* root_lin_vel_out,
                                    uint8_t* estimated_contacts_out) {
    A1_STAGE_BEGIN(movement_mode && foot_force && R_world && imu_acc && imu_ang_vel && foot_pos_rel && foot_vel_rel && root_pos_out && root_lin_vel_out &&
                   estimated_contacts_out && dt > 0, "null input/output pointer or dt <= 0", nullptr);
    Staging sg(h, n, s);
    if (a1mpc_status st = ensure_ekf_state(h, s); st != A1MPC_OK) return st;
    const double *d_ff = sg.in(foot_force, 4), *d_R = sg.in(R_world, 9), *d_acc = sg.in(imu_acc, 3), *d_w = sg.in(imu_ang_vel, 3), *d_fk = sg.in(foot_pos_rel, 12);
    const double* d_fv = sg.in(foot_vel_rel, 12);
    const uint8_t* d_mm = sg.in(movement_mode, 1);
    double *d_pos = sg.out(root_pos_out, 3), *d_vel = sg.out(root_lin_vel_out, 3);
    uint8_t* d_ec = sg.out(estimated_contacts_out, 4);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(A1_LAUNCH_EKF(h, n, dt, assume_flat_ground, d_mm, d_ff, d_R, d_acc, d_w, d_fk, d_fv, d_pos, d_vel, d_ec, s));
    return sg.finish();
}

// ---- N3: compute_joint_torques (S/A1RobotControl.cpp:289-319), one lane per (robot, leg); no FMA contraction ---------------------
struct TorqueArgs {
    int32_t n;
    const uint8_t *active, *contacts;
    const double *Jb, *grf, *fkin, *tg;
    double km[3];
    double* tau;
};
__global__ __launch_bounds__(256) void a1mpc_torque_kernel(const TorqueArgs a) {
#pragma clang fp contract(off)
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t b = gid >> 2;
    const int leg = static_cast<int>(gid & 3);
    if (b >= a.n) return;
    double* out = a.tau + b * 12 + 3 * leg;
    if (!a.active[b]) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; return; }   // :294-295
    const double* gr = a.grf + b * 12 + 3 * leg;
    const double* fk = a.fkin + b * 12 + 3 * leg;
    double t[3];
    leg_joint_torque(a.Jb + b * 36 + 9 * leg, a.contacts[b * 4 + leg] != 0, gr[0], gr[1], gr[2], a.km[0] * fk[0], a.km[1] * fk[1], a.km[2] * fk[2], t);   // (a1mpc_solver.hpp: shared with the MPC kernels' output stage)
    const double t0 = t[0], t1 = t[1], t2 = t[2];
    const double* g = a.tg + b * 12 + 3 * leg;
    const double v0 = t0 + g[0], v1 = t1 + g[1], v2 = t2 + g[2];                // :311
    if (!isnan(v0)) out[0] = v0;                                                // :314-317
    if (!isnan(v1)) out[1] = v1;
    if (!isnan(v2)) out[2] = v2;
}

static void launch_torque(int32_t n, const uint8_t* active, const uint8_t* contacts, const double* j_foot_blocks, const double* grf, const double* f_kin, const double* km_foot,
                          const double* torques_gravity, double* joint_torques, hipStream_t s) {
    TorqueArgs a;
    a.n = n; a.active = active; a.contacts = contacts; a.Jb = j_foot_blocks; a.grf = grf; a.fkin = f_kin; a.tg = torques_gravity; a.tau = joint_torques;
    a.km[0] = km_foot[0]; a.km[1] = km_foot[1]; a.km[2] = km_foot[2];
    hipLaunchKernelGGL(a1mpc_torque_kernel, leg_lane_grid(n), dim3(256), 0, s, a);
}

a1mpc_status a1mpc_joint_torques_batch(a1mpc_handle h, int32_t n, const uint8_t* active, const uint8_t* contacts, const double* j_foot_blocks,
                                       const double* grf, const double* f_kin, const double* km_foot, const double* torques_gravity,
                                       double* joint_torques) {
    A1_STAGE_BEGIN(active && contacts && j_foot_blocks && grf && f_kin && km_foot && torques_gravity && joint_torques, "null input/output pointer", nullptr);
    Staging sg(h, n, s);
    const double *d_J = sg.in(j_foot_blocks, 36), *d_grf = sg.in(grf, 12), *d_fk = sg.in(f_kin, 12), *d_tg = sg.in(torques_gravity, 12);
    double* d_tau = sg.inout(joint_torques, 12);   // (in as well: a NaN component leaves the caller's value, :314-317)
    const uint8_t *d_c = sg.in(contacts, 4), *d_act = sg.in(active, 1);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_torque(n, d_act, d_c, d_J, d_grf, d_fk, km_foot, d_tg, d_tau, s));
    return sg.finish();
}

void a1mpc_default_gait_config(a1mpc_gait_config* g) {
    if (!g) return;
    std::memset(g, 0, sizeof *g);
    g->counter_per_gait = 240.0; g->counter_per_swing = 120.0;        // S/A1CtrlStates.h:24-25
    g->control_dt = 0.0025;                                            // MAIN_UPDATE_FREQUENCY 2.5 ms, S/A1CtrlStates.h:332
    g->foot_delta_x_limit = 0.1; g->foot_delta_y_limit = 0.1;          // S/A1Params.h:44-45
    const double dfp[12] = {0.17, 0.15, -0.35, 0.17, -0.15, -0.35, -0.17, 0.15, -0.35, -0.17, -0.15, -0.35};  // S/A1CtrlStates.h:45-47
    std::memcpy(g->default_foot_pos, dfp, sizeof dfp);
    const double rs[4] = {0.0, 120.0, 120.0, 0.0};                     // S/A1CtrlStates.h:324
    std::memcpy(g->gait_counter_reset, rs, sizeof rs);
}

// (rel / abs / world are optional outputs: null = not wanted)
static PlanArgs make_plan_args(const a1mpc_gait_config& gait, int32_t n, const uint8_t* movement_mode, double* gait_counter, const double* gait_counter_speed,
                               const double* root_lin_vel, const double* R_z, const double* R_world, const double* root_pos, const double* root_lin_vel_d,
                               uint8_t* plan_contacts_out, double* rel_out, double* abs_out, double* world_out) {
    PlanArgs a;
    a.g = gait; a.n = n; a.movement_mode = movement_mode; a.gait_counter = gait_counter; a.gait_counter_speed = gait_counter_speed; a.root_lin_vel = root_lin_vel;
    a.Rz = R_z; a.Rw = R_world; a.root_pos = root_pos; a.root_lin_vel_d = root_lin_vel_d; a.plan_contacts = plan_contacts_out; a.rel = rel_out; a.abs_ = abs_out;
    a.world = world_out;
    return a;
}
static void launch_plan(const PlanArgs& a, hipStream_t s) { hipLaunchKernelGGL(a1mpc_plan_kernel, leg_lane_grid(a.n), dim3(256), 0, s, a); }

a1mpc_status a1mpc_update_plan_batch(a1mpc_handle h, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                     double* gait_counter, const double* gait_counter_speed, const double* root_lin_vel,
                                     const double* R_z, const double* R_world, const double* root_pos, const double* root_lin_vel_d,
                                     uint8_t* plan_contacts_out, double* rel_out, double* abs_out, double* world_out) {
    A1_STAGE_BEGIN(gait && movement_mode && gait_counter && gait_counter_speed && root_lin_vel && R_z && R_world && root_pos && root_lin_vel_d && plan_contacts_out,
                   "null config or input/output pointer", nullptr);
    Staging sg(h, n, s);
    double* d_gc = sg.inout(gait_counter, 4);
    const double *d_spd = sg.in(gait_counter_speed, 4), *d_v = sg.in(root_lin_vel, 3), *d_vd = sg.in(root_lin_vel_d, 3), *d_pos = sg.in(root_pos, 3);
    const double *d_Rz = sg.in(R_z, 9), *d_Rw = sg.in(R_world, 9);
    const uint8_t* d_mm = sg.in(movement_mode, 1);
    uint8_t* d_pc = sg.out(plan_contacts_out, 4);
    double *d_rel = sg.out(rel_out, 12), *d_abs = sg.out(abs_out, 12), *d_world = sg.out(world_out, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_plan(make_plan_args(*gait, n, d_mm, d_gc, d_spd, d_v, d_Rz, d_Rw, d_pos, d_vd, d_pc, d_rel, d_abs, d_world), s));
    return sg.finish();
}

// ---- device-pointer variants of the caller-side entry points: every array is device-resident, the call is asynchronous on `hip_stream`
// (NULL = the handle's stream), so a whole control tick -- leg state, EKF, plan, swing legs, contacts / terrain, MPC, joint torques --
// chains on the GPU without a PCIe hop.  Same kernels as the host-pointer entries.
a1mpc_status a1mpc_update_plan_batch_device(a1mpc_handle h, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                            double* gait_counter, const double* gait_counter_speed, const double* root_lin_vel, const double* R_z,
                                            const double* R_world, const double* root_pos, const double* root_lin_vel_d, uint8_t* plan_contacts_out,
                                            double* rel_out, double* abs_out, double* world_out, void* hip_stream) {
    A1_STAGE_BEGIN(gait && movement_mode && gait_counter && gait_counter_speed && root_lin_vel && R_z && R_world && root_pos && root_lin_vel_d && plan_contacts_out,
                   "null config or input/output pointer", hip_stream);
    A1_STAGE_LAUNCH(launch_plan(make_plan_args(*gait, n, movement_mode, gait_counter, gait_counter_speed, root_lin_vel, R_z, R_world, root_pos, root_lin_vel_d, plan_contacts_out,
                                               rel_out, abs_out, world_out), s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_swing_legs_batch_device(a1mpc_handle h, int32_t n, double counter_per_swing, double dt, const double* R_z, const double* foot_pos_abs,
                                           const double* gait_counter, const double* foot_pos_target_rel, const double* kp_foot_host, const double* kd_foot_host,
                                           double* foot_pos_start, double* foot_pos_rel_last_time, double* foot_pos_target_last_time, double* foot_pos_cur_out,
                                           double* foot_forces_kin_out, void* hip_stream) {
    A1_STAGE_BEGIN(R_z && foot_pos_abs && gait_counter && foot_pos_target_rel && kp_foot_host && kd_foot_host && foot_pos_start && foot_pos_rel_last_time &&
                   foot_pos_target_last_time && foot_pos_cur_out && foot_forces_kin_out && dt > 0, "null input/output pointer or dt <= 0", hip_stream);
    A1_STAGE_LAUNCH(launch_swing(make_swing_args(n, counter_per_swing, dt, kp_foot_host, kd_foot_host, R_z, foot_pos_abs, gait_counter, foot_pos_target_rel, foot_pos_start,
                                                 foot_pos_rel_last_time, foot_pos_target_last_time, foot_pos_cur_out, foot_forces_kin_out), s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_contact_terrain_batch_device(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* gait_counter,
                                                const uint8_t* plan_contacts, const double* foot_force, const double* foot_pos_abs, const double* root_pos_z,
                                                double* root_euler_d_pitch, uint8_t* contacts_out, double* foot_pos_recent_contact_out, double* terrain_angle_out,
                                                void* hip_stream) {
    A1_STAGE_BEGIN(cfg && gait_counter && plan_contacts && foot_force && foot_pos_abs && root_pos_z && root_euler_d_pitch && contacts_out &&
                   foot_pos_recent_contact_out && terrain_angle_out, "null config or input/output pointer", hip_stream);
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(launch_contact_terrain(make_contact_args(h, *cfg, n, gait_counter, plan_contacts, foot_force, foot_pos_abs, root_pos_z, root_euler_d_pitch, contacts_out,
                                                             foot_pos_recent_contact_out, terrain_angle_out), s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_leg_state_batch_device(a1mpc_handle h, int32_t n, const double* joint_pos, const double* joint_vel, const double* R_world,
                                          const double* root_pos, const double* root_lin_vel, const double* rho_fix_host, const double* rho_opt_host,
                                          double* foot_pos_rel_out, double* j_foot_blocks_out, double* foot_vel_rel_out, double* foot_pos_abs_out,
                                          double* foot_vel_abs_out, double* foot_pos_world_out, double* foot_vel_world_out, void* hip_stream) {
    A1_STAGE_BEGIN(joint_pos && joint_vel && R_world && root_pos && root_lin_vel && rho_fix_host && rho_opt_host && foot_pos_rel_out && j_foot_blocks_out,
                   "null input/output pointer", hip_stream);
    A1_STAGE_LAUNCH(launch_leg(n, rho_fix_host, rho_opt_host, joint_pos, joint_vel, R_world, root_pos, root_lin_vel, foot_pos_rel_out, j_foot_blocks_out, foot_vel_rel_out,
                               foot_pos_abs_out, foot_vel_abs_out, foot_pos_world_out, foot_vel_world_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_ekf_update_batch_device(a1mpc_handle h, int32_t n, double dt, int32_t assume_flat_ground, const uint8_t* movement_mode,
                                           const double* foot_force, const double* R_world, const double* imu_acc, const double* imu_ang_vel,
                                           const double* foot_pos_rel, const double* foot_vel_rel, double* root_pos_out, double* root_lin_vel_out,
                                           uint8_t* estimated_contacts_out, void* hip_stream) {
    A1_STAGE_BEGIN(movement_mode && foot_force && R_world && imu_acc && imu_ang_vel && foot_pos_rel && foot_vel_rel && root_pos_out && root_lin_vel_out &&
                   estimated_contacts_out && dt > 0, "null input/output pointer or dt <= 0", hip_stream);
    if (a1mpc_status st = ensure_ekf_state(h, s); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(A1_LAUNCH_EKF(h, n, dt, assume_flat_ground, movement_mode, foot_force, R_world, imu_acc, imu_ang_vel, foot_pos_rel, foot_vel_rel, root_pos_out,
                                  root_lin_vel_out, estimated_contacts_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_joint_torques_batch_device(a1mpc_handle h, int32_t n, const uint8_t* active, const uint8_t* contacts, const double* j_foot_blocks,
                                              const double* grf, const double* f_kin, const double* km_foot_host, const double* torques_gravity,
                                              double* joint_torques, void* hip_stream) {
    A1_STAGE_BEGIN(active && contacts && j_foot_blocks && grf && f_kin && km_foot_host && torques_gravity && joint_torques, "null input/output pointer", hip_stream);
    A1_STAGE_LAUNCH(launch_torque(n, active, contacts, j_foot_blocks, grf, f_kin, km_foot_host, torques_gravity, joint_torques, s));
    return A1MPC_OK;
}

// ---- the caller side of the balance-QP stance controller (stance_leg_control_type 0): the contact block alone and the PD wrench ----
// the contact block of generate_swing_legs_ctrl without the terrain fit (S/A1RobotControl.cpp:256-282; :335 skips the terrain block for this controller)
a1mpc_status a1mpc_contacts_batch(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* gait_counter, const uint8_t* plan_contacts,
                                  const double* foot_force, const double* foot_pos_abs, uint8_t* contacts_out, double* foot_pos_recent_contact_out) {
    A1_STAGE_BEGIN(cfg && gait_counter && plan_contacts && foot_force && foot_pos_abs && contacts_out && foot_pos_recent_contact_out,
                   "null config or input/output pointer", nullptr);
    Staging sg(h, n, s);
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    const double *d_gc = sg.in(gait_counter, 4), *d_ff = sg.in(foot_force, 4), *d_fp = sg.in(foot_pos_abs, 12);
    const uint8_t* d_pc = sg.in(plan_contacts, 4);
    uint8_t* d_ct = sg.out(contacts_out, 4);
    double* d_rec = sg.out(foot_pos_recent_contact_out, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_contacts(h, *cfg, n, d_gc, d_pc, d_ff, d_fp, d_ct, d_rec, s));
    return sg.finish();
}
a1mpc_status a1mpc_contacts_batch_device(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* gait_counter, const uint8_t* plan_contacts,
                                         const double* foot_force, const double* foot_pos_abs, uint8_t* contacts_out, double* foot_pos_recent_contact_out,
                                         void* hip_stream) {
    A1_STAGE_BEGIN(cfg && gait_counter && plan_contacts && foot_force && foot_pos_abs && contacts_out && foot_pos_recent_contact_out,
                   "null config or input/output pointer", hip_stream);
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(launch_contacts(h, *cfg, n, gait_counter, plan_contacts, foot_force, foot_pos_abs, contacts_out, foot_pos_recent_contact_out, s));
    return A1MPC_OK;
}

void a1mpc_default_balance_gains(a1mpc_balance_gains* g) {
    if (!g) return;
    const double kpl[3] = {1000.0, 1000.0, 1000.0}, kdl[3] = {200.0, 70.0, 120.0}, kpa[3] = {650.0, 35.0, 1.0}, kda[3] = {4.5, 4.5, 30.0};   // S/A1CtrlStates.h:117-120
    std::memcpy(g->kp_linear, kpl, sizeof kpl); std::memcpy(g->kd_linear, kdl, sizeof kdl);
    std::memcpy(g->kp_angular, kpa, sizeof kpa); std::memcpy(g->kd_angular, kda, sizeof kda);
}
static const char* invalid_balance_gains(const a1mpc_balance_gains* g) {
    if (!g) return "null a1mpc_balance_gains";
    if (!all_finite(g->kp_linear, 3) || !all_finite(g->kd_linear, 3) || !all_finite(g->kp_angular, 3) || !all_finite(g->kd_angular, 3))
        return "non-finite gain in a1mpc_balance_gains";
    return nullptr;
}
static void launch_wrench(a1mpc_handle h, const a1mpc_balance_gains& g, int32_t n, const double* root_pos_d, const double* root_pos, const double* root_lin_vel_d,
                          const double* root_lin_vel, const double* root_euler_d, const double* root_euler, const double* root_ang_vel_d, const double* root_ang_vel,
                          const double* R_world, double* root_acc, hipStream_t s) {
    WrenchArgs a;
    a.n = n; a.mass = h->cfg.mass;
    for (int i = 0; i < 3; ++i) { a.kp_lin[i] = g.kp_linear[i]; a.kd_lin[i] = g.kd_linear[i]; a.kp_ang[i] = g.kp_angular[i]; a.kd_ang[i] = g.kd_angular[i]; }
    a.pos_d = root_pos_d; a.pos = root_pos; a.lin_vel_d = root_lin_vel_d; a.lin_vel = root_lin_vel; a.euler_d = root_euler_d; a.euler = root_euler;
    a.ang_vel_d = root_ang_vel_d; a.ang_vel = root_ang_vel; a.R = R_world; a.root_acc = root_acc;
    hipLaunchKernelGGL(a1mpc_balance_wrench_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 255) / 256)), dim3(256), 0, s, a);
}
// which of the wrench's arrays is null, or null (none)
static const char* null_wrench_array(const double* root_pos_d, const double* root_pos, const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d,
                                     const double* root_euler, const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world, const double* root_acc_out) {
    const struct { const double* p; const char* what; } arrays[] = {{root_pos_d, "null root_pos_d"}, {root_pos, "null root_pos"}, {root_lin_vel_d, "null root_lin_vel_d"},
        {root_lin_vel, "null root_lin_vel"}, {root_euler_d, "null root_euler_d"}, {root_euler, "null root_euler"}, {root_ang_vel_d, "null root_ang_vel_d"},
        {root_ang_vel, "null root_ang_vel"}, {R_world, "null R_world"}, {root_acc_out, "null root_acc_out"}};
    for (const auto& q : arrays) if (!q.p) return q.what;
    return nullptr;
}
#define A1_WRENCH_BEGIN(hip_stream)                                                                                                     \
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");                                                                      \
    if (const char* bad = invalid_balance_gains(gains)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);                                    \
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");                                                                    \
    if (const char* bad = null_wrench_array(root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, \
                                            root_ang_vel, R_world, root_acc_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);          \
    A1_STAGE_DEVICE(hip_stream)
a1mpc_status a1mpc_balance_wrench_batch(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* root_pos_d, const double* root_pos,
                                        const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d, const double* root_euler,
                                        const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world, double* root_acc_out) {
    A1_WRENCH_BEGIN(nullptr);
    Staging sg(h, n, s);
    const double *d_pd = sg.in(root_pos_d, 3), *d_p = sg.in(root_pos, 3), *d_vd = sg.in(root_lin_vel_d, 3), *d_v = sg.in(root_lin_vel, 3), *d_ed = sg.in(root_euler_d, 3),
                 *d_e = sg.in(root_euler, 3), *d_wd = sg.in(root_ang_vel_d, 3), *d_w = sg.in(root_ang_vel, 3), *d_R = sg.in(R_world, 9);
    double* d_acc = sg.out(root_acc_out, 6);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_wrench(h, *gains, n, d_pd, d_p, d_vd, d_v, d_ed, d_e, d_wd, d_w, d_R, d_acc, s));
    return sg.finish();
}
a1mpc_status a1mpc_balance_wrench_batch_device(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* root_pos_d, const double* root_pos,
                                               const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d, const double* root_euler,
                                               const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world, double* root_acc_out, void* hip_stream) {
    A1_WRENCH_BEGIN(hip_stream);
    A1_STAGE_LAUNCH(launch_wrench(h, *gains, n, root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, root_ang_vel, R_world,
                                  root_acc_out, s));
    return A1MPC_OK;
}
#undef A1_WRENCH_BEGIN

// a1mpc_balance_wrench_batch with kp_linear[0:2] per robot (kp_linear_xy, n x 2): what the command stage switches (a1mpc_command_batch)
static void launch_wrench_kp(a1mpc_handle h, const a1mpc_balance_gains& g, int32_t n, const double* kp_linear_xy, const double* root_pos_d, const double* root_pos,
                             const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d, const double* root_euler, const double* root_ang_vel_d,
                             const double* root_ang_vel, const double* R_world, double* root_acc, hipStream_t s) {
    WrenchKpArgs k;
    WrenchArgs& a = k.w;
    a.n = n; a.mass = h->cfg.mass;
    for (int i = 0; i < 3; ++i) { a.kp_lin[i] = g.kp_linear[i]; a.kd_lin[i] = g.kd_linear[i]; a.kp_ang[i] = g.kp_angular[i]; a.kd_ang[i] = g.kd_angular[i]; }
    a.pos_d = root_pos_d; a.pos = root_pos; a.lin_vel_d = root_lin_vel_d; a.lin_vel = root_lin_vel; a.euler_d = root_euler_d; a.euler = root_euler;
    a.ang_vel_d = root_ang_vel_d; a.ang_vel = root_ang_vel; a.R = R_world; a.root_acc = root_acc;
    k.kp_xy = kp_linear_xy;
    hipLaunchKernelGGL(a1mpc_balance_wrench_kp_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 255) / 256)), dim3(256), 0, s, k);
}
#define A1_WRENCH_KP_BEGIN(hip_stream)                                                                                                  \
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");                                                                      \
    if (const char* bad = invalid_balance_gains(gains)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);                                    \
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");                                                                    \
    if (!kp_linear_xy) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null kp_linear_xy");                                                     \
    if (const char* bad = null_wrench_array(root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, \
                                            root_ang_vel, R_world, root_acc_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);          \
    A1_STAGE_DEVICE(hip_stream)
a1mpc_status a1mpc_balance_wrench_kp_batch(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* kp_linear_xy, const double* root_pos_d,
                                           const double* root_pos, const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d,
                                           const double* root_euler, const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world, double* root_acc_out) {
    A1_WRENCH_KP_BEGIN(nullptr);
    Staging sg(h, n, s);
    const double *d_kp = sg.in(kp_linear_xy, 2), *d_pd = sg.in(root_pos_d, 3), *d_p = sg.in(root_pos, 3), *d_vd = sg.in(root_lin_vel_d, 3), *d_v = sg.in(root_lin_vel, 3),
                 *d_ed = sg.in(root_euler_d, 3), *d_e = sg.in(root_euler, 3), *d_wd = sg.in(root_ang_vel_d, 3), *d_w = sg.in(root_ang_vel, 3), *d_R = sg.in(R_world, 9);
    double* d_acc = sg.out(root_acc_out, 6);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_wrench_kp(h, *gains, n, d_kp, d_pd, d_p, d_vd, d_v, d_ed, d_e, d_wd, d_w, d_R, d_acc, s));
    return sg.finish();
}
a1mpc_status a1mpc_balance_wrench_kp_batch_device(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* kp_linear_xy, const double* root_pos_d,
                                                  const double* root_pos, const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d,
                                                  const double* root_euler, const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world,
                                                  double* root_acc_out, void* hip_stream) {
    A1_WRENCH_KP_BEGIN(hip_stream);
    A1_STAGE_LAUNCH(launch_wrench_kp(h, *gains, n, kp_linear_xy, root_pos_d, root_pos, root_lin_vel_d, root_lin_vel, root_euler_d, root_euler, root_ang_vel_d, root_ang_vel,
                                     R_world, root_acc_out, s));
    return A1MPC_OK;
}
#undef A1_WRENCH_KP_BEGIN

// ---- the sensor and command front end (a1mpc_sensor_frontend_batch, a1mpc_command_batch): entries around a1mpc_sensor_frontend_kernel / a1mpc_command_kernel
void a1mpc_default_sensor_config(a1mpc_sensor_config* c) {
    if (!c) return;
    c->imu_window = 5;   // S/GazeboA1ROS.cpp:99-104: MovingWindowFilter(5), six of them
}
void a1mpc_default_command_config(a1mpc_command_config* c) {
    if (!c) return;
    c->body_height_max = 0.32; c->body_height_min = 0.1;   // JOY_CMD_BODY_HEIGHT_MAX / _MIN, S/A1Params.h:16-17
    c->kp_linear_lock_x = 120.0; c->kp_linear_lock_y = 120.0;   // a1_kp_linear_x / _y, S/A1CtrlStates.h:273-274, 298-299
    c->lock_speed = 0.05;                                  // S/GazeboA1ROS.cpp:180
    c->mpc_init_ticks = 10;                                // S/A1RobotControl.cpp:294
}
static const char* invalid_sensor_config(const a1mpc_sensor_config* c) {
    if (!c) return "null a1mpc_sensor_config";
    if (c->imu_window < 1 || c->imu_window > kImuWindowMax) return "a1mpc_sensor_config.imu_window outside 1 .. 64";
    return nullptr;
}
static const char* invalid_command_config(const a1mpc_command_config* c) {
    if (!c) return "null a1mpc_command_config";
    const double v[5] = {c->body_height_max, c->body_height_min, c->kp_linear_lock_x, c->kp_linear_lock_y, c->lock_speed};
    if (!all_finite(v, 5)) return "non-finite value in a1mpc_command_config";
    if (c->body_height_min > c->body_height_max) return "a1mpc_command_config.body_height_min > body_height_max";
    return nullptr;
}
struct SensorIo { const double *quat, *imu_acc_raw, *imu_gyro_raw; double *R_world, *R_z, *root_euler, *imu_acc, *imu_ang_vel, *root_ang_vel; };
struct CommandIo {
    const double* cmd; const uint8_t* mode_toggle; const double* root_pos; double dt;
    double* body_height; uint8_t* ctrl_state; double *root_euler_d, *root_pos_d, *kp_linear_xy; int32_t* mpc_init_counter;
    double *root_lin_vel_d, *root_ang_vel_d; uint8_t *movement_mode, *mpc_active; double* root_pos_d_z;
};
static const char* null_sensor_array(const SensorIo& io) {
    const struct { const void* p; const char* what; } arrays[] = {{io.quat, "null quat"}, {io.imu_acc_raw, "null imu_acc_raw"}, {io.imu_gyro_raw, "null imu_gyro_raw"},
        {io.R_world, "null R_world"}, {io.R_z, "null R_z"}, {io.root_euler, "null root_euler"}, {io.imu_acc, "null imu_acc"}, {io.imu_ang_vel, "null imu_ang_vel"},
        {io.root_ang_vel, "null root_ang_vel"}};
    for (const auto& q : arrays) if (!q.p) return q.what;
    return nullptr;
}
static const char* null_command_array(const CommandIo& io) {
    const struct { const void* p; const char* what; } arrays[] = {{io.cmd, "null cmd"}, {io.mode_toggle, "null mode_toggle"}, {io.root_pos, "null root_pos"},
        {io.body_height, "null body_height"}, {io.ctrl_state, "null ctrl_state"}, {io.root_euler_d, "null root_euler_d"}, {io.root_pos_d, "null root_pos_d"},
        {io.kp_linear_xy, "null kp_linear_xy"}, {io.mpc_init_counter, "null mpc_init_counter"}, {io.root_lin_vel_d, "null root_lin_vel_d"},
        {io.root_ang_vel_d, "null root_ang_vel_d"}, {io.movement_mode, "null movement_mode"}, {io.mpc_active, "null mpc_active"}, {io.root_pos_d_z, "null root_pos_d_z"}};
    for (const auto& q : arrays) if (!q.p) return q.what;
    return nullptr;
}
// every refusal of the two stages that needs no device: the message, or null
static const char* invalid_sensor_call(a1mpc_handle h, const a1mpc_sensor_config* cfg, int32_t n, const SensorIo& io) {
    if (const char* bad = invalid_sensor_config(cfg)) return bad;
    if (n < 0) return "negative n";
    if (const char* bad = null_sensor_array(io)) return bad;
    if (h->sensor_window != 0 && h->sensor_window != cfg->imu_window) return "a1mpc_sensor_config.imu_window differs from the window the filter state was built with (a1mpc_reset_sensor_state first)";
    return nullptr;
}
static const char* invalid_command_call(const a1mpc_command_config* cfg, int32_t n, const CommandIo& io) {
    if (const char* bad = invalid_command_config(cfg)) return bad;
    if (n < 0) return "negative n";
    if (!std::isfinite(io.dt)) return "non-finite dt";
    return null_command_array(io);
}
// the handle's IMU filter state for `window`: [6][window + 2][max_batch] doubles and [2][max_batch] cursors, zero = every filter empty.  A larger window than the
// allocation holds can only arrive after a reset (invalid_sensor_call), which has waited for the previous launches: the old block is free to go
static a1mpc_status ensure_sensor_state(a1mpc_handle h, int32_t window, hipStream_t s) {
    const size_t N = static_cast<size_t>(h->max_batch);
    if (h->d_sensor_filt && h->sensor_alloc_window < window) { A1_HIP(hipFree(h->d_sensor_filt)); h->d_sensor_filt = nullptr; }
    const bool fresh = !h->d_sensor_filt || !h->d_sensor_cursor;
    if (!h->d_sensor_filt) {
        A1_HIP(hipMalloc(&h->d_sensor_filt, N * kImuFilters * (static_cast<size_t>(window) + 2) * sizeof(double)));
        h->sensor_alloc_window = window;
    }
    if (!h->d_sensor_cursor) A1_HIP(hipMalloc(&h->d_sensor_cursor, N * 2 * sizeof(int32_t)));
    if (fresh) {
        A1_HIP(hipMemsetAsync(h->d_sensor_filt, 0, N * kImuFilters * (static_cast<size_t>(h->sensor_alloc_window) + 2) * sizeof(double), s));
        A1_HIP(hipMemsetAsync(h->d_sensor_cursor, 0, N * 2 * sizeof(int32_t), s));
    }
    h->sensor_window = window;
    return A1MPC_OK;
}
static void launch_sensor(a1mpc_handle h, int32_t window, int32_t n, const SensorIo& io, hipStream_t s) {
    SensorArgs a;
    a.n = n; a.window = window; a.stride = h->max_batch;
    a.quat = io.quat; a.acc_raw = io.imu_acc_raw; a.gyro_raw = io.imu_gyro_raw; a.filt = h->d_sensor_filt; a.cursor = h->d_sensor_cursor;
    a.R_world = io.R_world; a.R_z = io.R_z; a.euler = io.root_euler; a.acc = io.imu_acc; a.gyro = io.imu_ang_vel; a.ang_vel = io.root_ang_vel;
    hipLaunchKernelGGL(a1mpc_sensor_frontend_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 255) / 256)), dim3(256), 0, s, a);
}
static void launch_command(const a1mpc_command_config& c, int32_t n, const CommandIo& io, hipStream_t s) {
    CommandArgs a;
    a.n = n; a.init_ticks = c.mpc_init_ticks; a.dt = io.dt; a.height_max = c.body_height_max; a.height_min = c.body_height_min;
    a.lock_x = c.kp_linear_lock_x; a.lock_y = c.kp_linear_lock_y; a.lock_speed = c.lock_speed;
    a.cmd = io.cmd; a.root_pos = io.root_pos; a.toggle = io.mode_toggle; a.body_height = io.body_height; a.euler_d = io.root_euler_d; a.pos_d = io.root_pos_d;
    a.kp_xy = io.kp_linear_xy; a.ctrl_state = io.ctrl_state; a.init_counter = io.mpc_init_counter; a.lin_vel_d = io.root_lin_vel_d; a.ang_vel_d = io.root_ang_vel_d;
    a.pos_d_z = io.root_pos_d_z; a.movement_mode = io.movement_mode; a.mpc_active = io.mpc_active;
    hipLaunchKernelGGL(a1mpc_command_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 255) / 256)), dim3(256), 0, s, a);
}
a1mpc_status a1mpc_reset_sensor_state(a1mpc_handle h) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    h->sensor_window = 0;
    if (!h->d_sensor_filt || !h->d_sensor_cursor) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);  // the memsets below must not overtake a launch still running on a caller's stream
    A1_HIP(hipMemsetAsync(h->d_sensor_filt, 0, static_cast<size_t>(h->max_batch) * kImuFilters * (static_cast<size_t>(h->sensor_alloc_window) + 2) * sizeof(double), h->stream));
    A1_HIP(hipMemsetAsync(h->d_sensor_cursor, 0, static_cast<size_t>(h->max_batch) * 2 * sizeof(int32_t), h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    return A1MPC_OK;
}
#define A1_SENSOR_BEGIN(hip_stream)                                                                                      \
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");                                                       \
    const SensorIo io{quat, imu_acc_raw, imu_gyro_raw, R_world_out, R_z_out, root_euler_out, imu_acc_out, imu_ang_vel_out, root_ang_vel_out}; \
    if (const char* bad = invalid_sensor_call(h, cfg, n, io)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);               \
    A1_STAGE_DEVICE(hip_stream)
a1mpc_status a1mpc_sensor_frontend_batch(a1mpc_handle h, const a1mpc_sensor_config* cfg, int32_t n, const double* quat, const double* imu_acc_raw, const double* imu_gyro_raw,
                                         double* R_world_out, double* R_z_out, double* root_euler_out, double* imu_acc_out, double* imu_ang_vel_out, double* root_ang_vel_out) {
    A1_SENSOR_BEGIN(nullptr);
    Staging sg(h, n, s);
    if (a1mpc_status st = ensure_sensor_state(h, cfg->imu_window, s); st != A1MPC_OK) return st;
    SensorIo d;
    d.quat = sg.in(quat, 4); d.imu_acc_raw = sg.in(imu_acc_raw, 3); d.imu_gyro_raw = sg.in(imu_gyro_raw, 3);
    d.R_world = sg.out(R_world_out, 9); d.R_z = sg.out(R_z_out, 9); d.root_euler = sg.out(root_euler_out, 3); d.imu_acc = sg.out(imu_acc_out, 3);
    d.imu_ang_vel = sg.out(imu_ang_vel_out, 3); d.root_ang_vel = sg.out(root_ang_vel_out, 3);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_sensor(h, cfg->imu_window, n, d, s));
    return sg.finish();
}
a1mpc_status a1mpc_sensor_frontend_batch_device(a1mpc_handle h, const a1mpc_sensor_config* cfg, int32_t n, const double* quat, const double* imu_acc_raw,
                                                const double* imu_gyro_raw, double* R_world_out, double* R_z_out, double* root_euler_out, double* imu_acc_out,
                                                double* imu_ang_vel_out, double* root_ang_vel_out, void* hip_stream) {
    A1_SENSOR_BEGIN(hip_stream);
    if (a1mpc_status st = ensure_sensor_state(h, cfg->imu_window, s); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(launch_sensor(h, cfg->imu_window, n, io, s));
    return A1MPC_OK;
}
#undef A1_SENSOR_BEGIN
#define A1_COMMAND_BEGIN(hip_stream)                                                                                      \
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");                                                       \
    const CommandIo io{cmd, mode_toggle, root_pos, dt, body_height, ctrl_state, root_euler_d, root_pos_d, kp_linear_xy, mpc_init_counter, root_lin_vel_d_out, \
                       root_ang_vel_d_out, movement_mode_out, mpc_active_out, root_pos_d_z_out};                           \
    if (const char* bad = invalid_command_call(cfg, n, io)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);                 \
    A1_STAGE_DEVICE(hip_stream)
a1mpc_status a1mpc_command_batch(a1mpc_handle h, const a1mpc_command_config* cfg, int32_t n, const double* cmd, const uint8_t* mode_toggle, const double* root_pos, double dt,
                                 double* body_height, uint8_t* ctrl_state, double* root_euler_d, double* root_pos_d, double* kp_linear_xy, int32_t* mpc_init_counter,
                                 double* root_lin_vel_d_out, double* root_ang_vel_d_out, uint8_t* movement_mode_out, uint8_t* mpc_active_out, double* root_pos_d_z_out) {
    A1_COMMAND_BEGIN(nullptr);
    Staging sg(h, n, s);
    CommandIo d;
    d.dt = dt;
    d.cmd = sg.in(cmd, 6); d.mode_toggle = sg.in(mode_toggle, 1); d.root_pos = sg.in(root_pos, 3);
    d.body_height = sg.inout(body_height, 1); d.ctrl_state = sg.inout(ctrl_state, 1); d.root_euler_d = sg.inout(root_euler_d, 3); d.root_pos_d = sg.inout(root_pos_d, 3);
    d.kp_linear_xy = sg.inout(kp_linear_xy, 2);
    d.mpc_init_counter = reinterpret_cast<int32_t*>(sg.slice<double>(1));   // (n int32 in a slice of n doubles)
    if (d.mpc_init_counter) {
        sg.hip(hipMemcpyAsync(d.mpc_init_counter, mpc_init_counter, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyHostToDevice, s), "hipMemcpyAsync (staging, host to device)");
        sg.back(mpc_init_counter, static_cast<const int32_t*>(d.mpc_init_counter), 1);
    }
    d.root_lin_vel_d = sg.out(root_lin_vel_d_out, 3); d.root_ang_vel_d = sg.out(root_ang_vel_d_out, 3); d.movement_mode = sg.out(movement_mode_out, 1);
    d.mpc_active = sg.out(mpc_active_out, 1); d.root_pos_d_z = sg.out(root_pos_d_z_out, 1);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_command(*cfg, n, d, s));
    return sg.finish();
}
a1mpc_status a1mpc_command_batch_device(a1mpc_handle h, const a1mpc_command_config* cfg, int32_t n, const double* cmd, const uint8_t* mode_toggle, const double* root_pos,
                                        double dt, double* body_height, uint8_t* ctrl_state, double* root_euler_d, double* root_pos_d, double* kp_linear_xy,
                                        int32_t* mpc_init_counter, double* root_lin_vel_d_out, double* root_ang_vel_d_out, uint8_t* movement_mode_out, uint8_t* mpc_active_out,
                                        double* root_pos_d_z_out, void* hip_stream) {
    A1_COMMAND_BEGIN(hip_stream);
    A1_STAGE_LAUNCH(launch_command(*cfg, n, io, s));
    return A1MPC_OK;
}
#undef A1_COMMAND_BEGIN

const char* a1mpc_status_string(a1mpc_status s) {
    switch (s) {
        case A1MPC_OK: return "ok";
        case A1MPC_ERR_INVALID_ARGUMENT: return "invalid argument";
        case A1MPC_ERR_UNSUPPORTED_HORIZON: return "unsupported horizon";
        case A1MPC_ERR_NO_DEVICE: return "no HIP device";
        case A1MPC_ERR_HIP: return "HIP runtime error";
        case A1MPC_ERR_BATCH_TOO_LARGE: return "batch larger than max_batch";
    }
    return "unknown";
}
const char* a1mpc_last_error(void) { return g_last_error.c_str(); }

// which sources this library is the compilation of (build.py: sha256 over csrc/ + include/a1mpc.h) -- a shipped .so is matched against the sources beside it.
// The string lives in a unit of its own (a1mpc_build_id.cpp, compiled in a second): a change of any source re-stamps the library without recompiling this file.
const char* a1mpc_build_info(void) { return a1mpc_build_id_; }

void a1mpc_destroy(a1mpc_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    void* ptrs[] = {h->d_tab, h->d_tab1, h->d_x0, h->d_xref, h->d_R, h->d_foot, h->d_aux, h->d_Rz, h->d_contact, h->d_grf,
                    h->d_u, h->d_iters, h->d_status, h->d_nfact, h->d_wx, h->d_wy, h->d_rho, h->d_prep, h->d_counter, h->d_in, h->d_out, h->d_order, h->d_cost, h->d_ct_state, h->d_ekf_state, h->d_aux_in, h->d_aux_out, h->d_aux_u8, h->d_episode_ws, h->d_foot_steps, h->d_contact_steps, h->d_prep_gen, h->d_carry, h->d_clk, h->d_tickrec, h->d_pv_sched, h->d_pv_foot, h->d_hs_u, h->d_hs_x, h->d_bal_acc, h->d_sensor_filt, h->d_sensor_cursor};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_pin) (void)hipHostFree(h->h_pin);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_order) (void)hipEventDestroy(h->ev_order);
    if (h->ev_mark) (void)hipEventDestroy(h->ev_mark);
    if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
    if (h->ev_tick0) (void)hipEventDestroy(h->ev_tick0);
    if (h->ev_tick1) (void)hipEventDestroy(h->ev_tick1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// what a1mpc_episode_summary_batch keeps on the device for max_batch rows: its host entry's 20 words, then one partial summary per 64 rows of every level but the last
static size_t episode_ws_doubles(int32_t max_batch) {
    size_t total = kEpSummary;
    for (size_t m = (static_cast<size_t>(max_batch) + 63) / 64; m > 1; m = (m + 63) / 64) total += m * kEpSummary;
    return total;
}
// The small-batch path of the host-pointer entries (pin_inputs): batches of up to A1MPC_ZERO_COPY_MAX QPs (default 8; 0 = always stage through device memory).
// The general path takes it for at most 64 QPs, so that a large setting cannot inflate the pinned block a1mpc_create sizes for it.
static int zero_copy_max() {
    static const int m = [] { const char* e = getenv("A1MPC_ZERO_COPY_MAX"); return e ? atoi(e) : 8; }();
    return m;
}
static size_t small_general_max() { return zero_copy_max() <= 64 ? static_cast<size_t>(std::max(zero_copy_max(), 0)) : 0; }
static bool small_batch(a1mpc_handle h, int32_t n) { return n <= zero_copy_max() && h->d_pin != nullptr; }

a1mpc_status a1mpc_create(const a1mpc_config* cfg, int32_t max_batch, int32_t device, a1mpc_handle* out) {
    if (!cfg || !out || max_batch <= 0 || device < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null config/out or bad batch/device");
    *out = nullptr;
    if (ops_of(cfg->horizon) == nullptr) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "horizon must be " A1MPC_HORIZON_LIST);
    if (const char* why = invalid_config(*cfg)) return fail(A1MPC_ERR_INVALID_ARGUMENT, why);   // (before any device query: a bad configuration is reported as such on every machine)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(A1MPC_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    if (device >= ndev) return fail(A1MPC_ERR_NO_DEVICE, "device ordinal out of range");
    A1_HIP(hipSetDevice(device));
    a1mpc_handle h = new (std::nothrow) a1mpc_handle_s();
    if (!h) return fail(A1MPC_ERR_HIP, "out of host memory");
    h->cfg = *cfg;
    to_device_params(*cfg, &h->dp);
    h->device = device;
    h->max_batch = max_batch;
    const int H = cfg->horizon;
    const size_t n = static_cast<size_t>(max_batch);
#define A1_TRY(call)                                  \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) {                       \
            a1mpc_destroy(h);                         \
            return fail(A1MPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
        }                                             \
    } while (0)
    A1_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    A1_TRY(hipEventCreate(&h->ev0));
    A1_TRY(hipEventCreate(&h->ev1));
    A1_TRY(hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming));
    A1_TRY(hipEventCreateWithFlags(&h->ev_mark, hipEventDisableTiming));
    A1_TRY(hipEventCreate(&h->ev_mid));
    A1_TRY(hipEventCreate(&h->ev_tick0));
    A1_TRY(hipEventCreate(&h->ev_tick1));
    std::vector<double> tab(2 * H * H), tab1(2);
    fill_gamma_beta_table(H, tab.data());
    fill_gamma_beta_table(1, tab1.data());
    A1_TRY(hipMalloc(&h->d_tab, tab.size() * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_tab1, tab1.size() * sizeof(double)));
    A1_TRY(hipMemcpy(h->d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    A1_TRY(hipMemcpy(h->d_tab1, tab1.data(), tab1.size() * sizeof(double), hipMemcpyHostToDevice));
    A1_TRY(hipMalloc(&h->d_x0, n * 13 * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_xref, n * 13 * H * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_R, n * 9 * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_Rz, n * 9 * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_foot, n * 12 * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_aux, n * 6 * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_contact, n * 4));
    A1_TRY(hipMalloc(&h->d_grf, n * 12 * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_u, n * 12 * H * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_iters, n * sizeof(int32_t)));
    A1_TRY(hipMalloc(&h->d_status, n * sizeof(int32_t)));
    A1_TRY(hipMalloc(&h->d_nfact, n * sizeof(int32_t)));
    A1_TRY(hipMalloc(&h->d_wx, n * 12 * H * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_wy, n * 20 * H * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_rho, n * sizeof(double)));
    A1_TRY(hipMemset(h->d_wx, 0, n * 12 * H * sizeof(double)));
    A1_TRY(hipMemset(h->d_wy, 0, n * 20 * H * sizeof(double)));
    A1_TRY(hipMemset(h->d_rho, 0, n * sizeof(double)));
    if (pipeline_mode() != 2) A1_TRY(hipMalloc(&h->d_prep, n * ops_of(H)->prep_stride * sizeof(double)));
    A1_TRY(hipMalloc(&h->d_counter, sizeof(int)));
    A1_TRY(hipMalloc(&h->d_order, n * sizeof(int32_t)));
    A1_TRY(hipMalloc(&h->d_cost, n * sizeof(int32_t)));
    if (const char* e = std::getenv("A1MPC_SCHEDULE")) h->schedule = std::strcmp(e, "index") != 0;
    // pinned block: the input region, which holds every small-batch layout for every n the small path takes (pin_inputs), then the output region
    // [grf | iters | status | u] (host_out_layout).  Per QP: the fast layout -- x0, x_ref, R, feet, contacts; the tick-record and balance layouts are smaller -- for
    // up to max_batch QPs (it is also what a staged launch copies into d_in), the general layout -- x0, x_ref, R, 12H feet, yaw, 4H contacts -- for up to
    // small_general_max() QPs.
    const size_t fast_in = n * ((13 + 13 * H + 9 + 12) * sizeof(double) + 8);
    const size_t gen_in = std::min(n, small_general_max()) * ((13 + 13 * H + 9 + 12 * H + 1) * sizeof(double) + (4 * H + 7) / 8 * 8);
    h->h_pin_in_bytes = std::max(fast_in, gen_in);
    const size_t out_max = n * ((12 + 12 * H) * sizeof(double) + 2 * sizeof(int32_t));
    h->h_pin_bytes = h->h_pin_in_bytes + out_max;
    A1_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_in), fast_in));
    A1_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_out), out_max));
    A1_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_pin), h->h_pin_bytes, hipHostMallocDefault));
    { void* dp = nullptr; if (hipHostGetDevicePointer(&dp, h->h_pin, 0) == hipSuccess) h->d_pin = static_cast<char*>(dp); else (void)hipGetLastError(); }
    // the episode summary's partials (a few bytes per robot): here, so that the first summary of a run allocates nothing; a failure is left to that call to report
    if (hipMalloc(reinterpret_cast<void**>(&h->d_episode_ws), episode_ws_doubles(max_batch) * sizeof(double)) != hipSuccess) { h->d_episode_ws = nullptr; (void)hipGetLastError(); }
    // One-time, per process: the first launches / copies through a fresh HIP runtime cost milliseconds (code-object load, pool set-up);
    // a 400 Hz loop should not pay that on its first tick (measured 5 ms -> 0.4 ms), so the tick's operation mix is exercised here.
    static std::vector<int> runtime_warmed;   // the devices done: a sharded handle (a1mpc_sharded_*) creates one engine handle on every GPU of the node
    std::unique_lock<std::mutex> warm_lock(g_cache_mu);   // (handles may be created from several threads)
    if (std::find(runtime_warmed.begin(), runtime_warmed.end(), device) == runtime_warmed.end()) {
        for (int i = 0; i < 256; ++i) {  // the operation mix of a tick: copies both ways from pinned memory, memset, launches, events
            A1_TRY(hipMemcpyAsync(h->d_x0, h->h_pin, 8, hipMemcpyHostToDevice, h->stream));
            A1_TRY(hipMemsetAsync(h->d_counter, 0, sizeof(int), h->stream));
            A1_TRY(hipEventRecord(h->ev0, h->stream));
            hipLaunchKernelGGL(a1mpc_noop_kernel, dim3(1), dim3(64), 0, h->stream);
            hipLaunchKernelGGL(a1mpc_noop_kernel, dim3(1), dim3(64), 0, h->stream);
            A1_TRY(hipEventRecord(h->ev1, h->stream));
            A1_TRY(hipMemcpyAsync(h->h_pin + 64, h->d_x0, 8, hipMemcpyDeviceToHost, h->stream));
            if ((i & 63) == 63) A1_TRY(hipStreamSynchronize(h->stream));
        }
        A1_TRY(hipStreamSynchronize(h->stream));
        runtime_warmed.push_back(device);
    }
    warm_lock.unlock();
#undef A1_TRY
    *out = h;
    return A1MPC_OK;
}

a1mpc_status a1mpc_update_config(a1mpc_handle h, const a1mpc_config* cfg) {
    if (!h || !cfg) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/config");
    if (cfg->horizon != h->cfg.horizon) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "the horizon of a handle is fixed at a1mpc_create");
    if (const char* why = invalid_config(*cfg)) return fail(A1MPC_ERR_INVALID_ARGUMENT, why);   // (the handle keeps the configuration it had)
    // every constant travels to the kernels by value with each launch: nothing on the device has to change, launches already
    // queued keep the values they were issued with, the carried warm start stays
    if (cfg->warm_start != h->cfg.warm_start && h->d_carry) {
        // leaving or entering the update path: ticks solved in another mode do not refresh its carry (previous scalings / gradient / z), so what is there is stale
        A1_HIP(hipSetDevice(h->device));
        A1_ORDER(h, h->stream);
        A1_HIP(hipMemsetAsync(h->d_carry, 0, static_cast<size_t>(h->max_batch) * carry_stride(h->cfg.horizon) * sizeof(double), h->stream));
        A1_MARK(h, h->stream);
    }
    h->cfg = *cfg;
    to_device_params(*cfg, &h->dp);
    return A1MPC_OK;
}

a1mpc_status a1mpc_warm_start(a1mpc_handle h, int32_t n, const double* x, const double* y, const double* rho) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0 || (!x && !y && !rho)) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);
    const size_t N = n, H = h->cfg.horizon;
    if (x) A1_HIP(hipMemcpyAsync(h->d_wx, x, N * 12 * H * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (y) A1_HIP(hipMemcpyAsync(h->d_wy, y, N * 20 * H * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (rho) A1_HIP(hipMemcpyAsync(h->d_rho, rho, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // warm_start = 2: the injected state is re-expressed on the update path's workspace the way osqp_warm_start_x / _y do it on the reference's persistent solver:
    // x and y replace the carried (unscaled) iterates above, z becomes A x (osqp_warm_start_x: z = A x), the previous tick's scalings, gradient and pattern stay --
    // the next tick follows the update path from there.  (Until round 4 the carry was cleared: that tick was a fresh set-up.)
    std::vector<double> zbuf;
    if (h->d_carry && x) {
        const size_t cs = carry_stride(h->cfg.horizon);
        const double mu = h->cfg.mu;
        zbuf.resize(N * 24 * H);
        for (size_t b = 0; b < N; ++b)
            for (size_t t = 0; t < H; ++t)
                for (int leg = 0; leg < 4; ++leg) {
                    const double* f = x + (b * H + t) * 12 + 3 * leg;
                    double* z0 = zbuf.data() + b * 24 * H + t * 12 + 3 * leg;   // [Z0: 12H | Z1: 12H] of Carry<H>, per lane (leg, comp)
                    double* z1 = z0 + 12 * H;
                    z0[0] = std::fma(mu, f[2], f[0]); z0[1] = std::fma(mu, f[2], f[1]); z0[2] = f[2];
                    z1[0] = std::fma(-mu, f[2], f[0]); z1[1] = std::fma(-mu, f[2], f[1]); z1[2] = 0.0;
                }
        A1_HIP(hipMemcpy2DAsync(h->d_carry + (1 + 48 * H), cs * sizeof(double), zbuf.data(), 24 * H * sizeof(double), 24 * H * sizeof(double), N, hipMemcpyHostToDevice, h->stream));
    }
    A1_HIP(hipStreamSynchronize(h->stream));
    return A1MPC_OK;
}

a1mpc_status a1mpc_get_warm_start(a1mpc_handle h, int32_t n, double* x_out, double* y_out, double* rho_out) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);
    const size_t N = n, H = h->cfg.horizon;
    if (x_out) A1_HIP(hipMemcpyAsync(x_out, h->d_wx, N * 12 * H * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (y_out) A1_HIP(hipMemcpyAsync(y_out, h->d_wy, N * 20 * H * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (rho_out) A1_HIP(hipMemcpyAsync(rho_out, h->d_rho, N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    return A1MPC_OK;
}

a1mpc_status a1mpc_set_timing(a1mpc_handle h, int32_t on) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    h->timing = on != 0;
    if (!h->timing) { h->timed = false; h->tick_timed = false; h->staged = false; }
    return A1MPC_OK;
}
a1mpc_status a1mpc_set_profiling(a1mpc_handle h, int32_t on) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    h->profiling = on != 0;
    return A1MPC_OK;
}
a1mpc_status a1mpc_last_stage_cycles(a1mpc_handle h, double* cycles3_out, int32_t* qps_out) {
    if (!h || !cycles3_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / output");
    cycles3_out[0] = cycles3_out[1] = cycles3_out[2] = 0.0;
    if (qps_out) *qps_out = h->clk_n;
    if (h->clk_n == 0 || !h->d_clk) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);
    std::vector<long long> c(static_cast<size_t>(h->clk_n) * kTickStages);
    A1_HIP(hipMemcpyAsync(c.data(), h->d_clk, c.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    for (int b = 0; b < h->clk_n; ++b) for (int k = 0; k < 3; ++k) cycles3_out[k] += static_cast<double>(c[static_cast<size_t>(b) * kTickStages + kClkFactor + k]);
    return A1MPC_OK;
}
a1mpc_status a1mpc_last_tick_stage_cycles(a1mpc_handle h, double* cycles8_out, int32_t* qps_out) {
    if (!h || !cycles8_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / output");
    for (int k = 0; k < kTickStages; ++k) cycles8_out[k] = 0.0;
    const int32_t nq = h->clk_tick ? h->clk_n : 0;
    if (qps_out) *qps_out = nq;
    if (nq == 0 || !h->d_clk) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);
    std::vector<long long> c(static_cast<size_t>(nq) * kTickStages);
    A1_HIP(hipMemcpyAsync(c.data(), h->d_clk, c.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    for (int b = 0; b < nq; ++b) for (int k = 0; k < kTickStages; ++k) cycles8_out[k] += static_cast<double>(c[static_cast<size_t>(b) * kTickStages + k]);
    return A1MPC_OK;
}

a1mpc_status a1mpc_last_warm_start_mode(a1mpc_handle h, int32_t* mode_out) {
    if (!h || !mode_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / output");
    *mode_out = h->last_ws_mode;
    return A1MPC_OK;
}

// one Carry<H> record -> 20H rows: lane (leg, comp) holds rows r0 (Z0) and, for fx / fy, r1 (Z1) of its leg's block
static void unpack_carry_z(int H, const double* rec, double* z) {
    const int Z0 = 1 + 48 * H, Z1 = 1 + 60 * H;
    static_assert(Carry<10>::Z0 == 1 + 48 * 10 && Carry<10>::Z1 == 1 + 60 * 10 && Carry<20>::Z0 == 1 + 48 * 20 && Carry<20>::Z1 == 1 + 60 * 20, "Carry<H> layout");
    for (int t = 0; t < H; ++t)
        for (int ci = 0; ci < 12; ++ci) {
            const int leg = ci / 3, comp = ci % 3;
            const int r0 = comp == 0 ? 0 : (comp == 1 ? 2 : 4), r1 = comp == 0 ? 1 : 3;
            z[t * 20 + 5 * leg + r0] = rec[Z0 + t * 12 + ci];
            if (comp < 2) z[t * 20 + 5 * leg + r1] = rec[Z1 + t * 12 + ci];
        }
}
a1mpc_status a1mpc_get_workspace_z(a1mpc_handle h, int32_t n, double* z_out) {
    if (!h || !z_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / output");
    if (n < 0 || n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    const size_t cs = carry_stride(h->cfg.horizon);
    if (h->cfg.warm_start != 2 || cs == 0 || !h->d_carry) return fail(A1MPC_ERR_INVALID_ARGUMENT, "no update-path carry (warm_start = 2, horizon > 1, after the first tick)");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);
    std::vector<double> rec(static_cast<size_t>(n) * cs);
    A1_HIP(hipMemcpyAsync(rec.data(), h->d_carry, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    const size_t H = h->cfg.horizon;
    for (int b = 0; b < n; ++b) {
        const double* r = rec.data() + static_cast<size_t>(b) * cs;
        double* z = z_out + static_cast<size_t>(b) * 20 * H;
        unpack_carry_z(h->cfg.horizon, r, z);
    }
    return A1MPC_OK;
}

a1mpc_status a1mpc_get_workspace_scaling(a1mpc_handle h, int32_t n, double* D_out, double* E_out, double* c_out) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    const size_t cs = carry_stride(h->cfg.horizon);
    if (h->cfg.warm_start != 2 || cs == 0 || !h->d_carry) return fail(A1MPC_ERR_INVALID_ARGUMENT, "no update-path carry (warm_start = 2, horizon > 1, after the first tick)");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);
    std::vector<double> rec(static_cast<size_t>(n) * cs);
    A1_HIP(hipMemcpyAsync(rec.data(), h->d_carry, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    const int H = h->cfg.horizon;
    const int oD = 1, oE0 = 1 + 12 * H, oE1 = 1 + 24 * H;   // Carry<H>::D, E0, E1
    static_assert(Carry<10>::D == 1 && Carry<10>::E0 == 1 + 120 && Carry<10>::E1 == 1 + 240 && Carry<16>::E1 == 1 + 24 * 16, "Carry<H> layout");
    for (int b = 0; b < n; ++b) {
        const double* r = rec.data() + static_cast<size_t>(b) * cs;
        if (c_out) c_out[b] = r[0];
        for (int t = 0; t < H; ++t)
            for (int ci = 0; ci < 12; ++ci) {
                const int leg = ci / 3, comp = ci % 3;
                const int r0 = comp == 0 ? 0 : (comp == 1 ? 2 : 4), r1 = comp == 0 ? 1 : 3;
                if (D_out) D_out[(static_cast<size_t>(b) * H + t) * 12 + ci] = r[oD + t * 12 + ci];
                if (E_out) {
                    double* e = E_out + (static_cast<size_t>(b) * H + t) * 20 + 5 * leg;
                    e[r0] = r[oE0 + t * 12 + ci];
                    if (comp < 2) e[r1] = r[oE1 + t * 12 + ci];
                }
            }
    }
    return A1MPC_OK;
}

a1mpc_status a1mpc_reset_warm_start(a1mpc_handle h) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    A1_HIP(hipSetDevice(h->device));
    A1_ORDER(h, h->stream);  // the memsets below must not overtake a launch still running on a caller's stream
    const size_t n = h->max_batch, H = h->cfg.horizon;
    A1_HIP(hipMemsetAsync(h->d_wx, 0, n * 12 * H * sizeof(double), h->stream));
    A1_HIP(hipMemsetAsync(h->d_wy, 0, n * 20 * H * sizeof(double), h->stream));
    A1_HIP(hipMemsetAsync(h->d_rho, 0, n * sizeof(double), h->stream));
    if (h->d_carry) A1_HIP(hipMemsetAsync(h->d_carry, 0, n * carry_stride(h->cfg.horizon) * sizeof(double), h->stream));
    A1_HIP(hipStreamSynchronize(h->stream));
    h->hint_n = 0;
    return A1MPC_OK;
}

a1mpc_status a1mpc_set_schedule(a1mpc_handle h, int32_t history) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    h->schedule = history != 0;
    h->hint_n = 0;
    return A1MPC_OK;
}

// N3 in the MPC kernels' output stage (a1mpc_control_tick_device): the device arrays compute_joint_torques reads and writes; `fused` reports whether the launch that
// solve_device_impl chose carries the stage (the fused / latency kernels do; the split pipeline's persistent rows do not -- the caller then launches the torque kernel)
struct TorqueFuse {
    const uint8_t* active;
    const double *J, *fkin, *tg, *km;
    double* tau;
    bool fused;
};
// A1MPC_WARM_ORDER=1: launch the fused kernel of a warm-started tick in the order of the previous tick's per-QP cost (longest first).  OFF by default: measured and
// lost (profiles/r05_warm_tick_order.txt: 4096 x h10 ticks 0.335 -> 0.348 ms, update path 0.362 -> 0.373) -- a warm tick has no tail worth ordering for (3 of 4096
// QPs need a second 25-iteration segment and the two rounds of the resident rows absorb them), and the order kernel in front of the tick costs its ~12 us.
// Round 6 experiment switch (profiles/r06_control_tick_timeline.md): with the handle's timing events OFF, record a no-timing marker event where a timing event would have been
// -- bit 0: in front of the MPC launch (ev0), bit 1: at the start of a control tick (ev_tick0), bit 2: behind the MPC launch (ev1), bit 3: at the end of a tick (ev_tick1)
static int tick_markers() {
    static const int m = [] { const char* e = getenv("A1MPC_TICK_MARKERS"); return e ? atoi(e) : 0; }();
    return m;
}
static bool warm_order_enabled() {
    static const bool on = [] { const char* e = getenv("A1MPC_WARM_ORDER"); return e && !strcmp(e, "1"); }();
    return on;
}
static a1mpc_status solve_device_impl(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_x0, const double* d_x_ref,
                                      const double* d_R_world, const double* d_foot_abs, const uint8_t* d_contact,
                                      double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out,
                                      void* hip_stream, int32_t foot_stride = 0, int32_t contact_stride = 0, const double* d_yaw_A = nullptr, TorqueFuse* tq = nullptr) {
    if (tq) tq->fused = false;
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || (!d_tick && (!d_x0 || !d_x_ref)) || !d_R_world || !d_foot_abs || !d_contact || !d_grf_body_out)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream;
    A1_ORDER(h, s);
    h->clk_n = 0; h->clk_tick = false;   // (set again below when this solve runs a profiling instantiation)
    const HorizonOps& ops = *ops_of(h->cfg.horizon);   // (a handle's horizon is compiled in: a1mpc_create)
    KernelArgs a;
    std::memset(&a, 0, sizeof a);
    a.P = h->dp; a.tab = h->d_tab; a.n = n;
    a.tick = d_tick; a.x0 = d_x0; a.xref = d_x_ref; a.R = d_R_world; a.foot = d_foot_abs; a.contact = d_contact;
    a.grf = d_grf_body_out; a.u_full = d_u_full_out; a.iters = d_iters_out; a.status = d_status_out; a.nfact = h->d_nfact;
    if (h->cfg.warm_start) { a.warm_x = h->d_wx; a.warm_y = h->d_wy; a.rho = h->d_rho; }
    if (h->cfg.warm_start == 2 && carry_stride(h->cfg.horizon) != 0) {   // the reference's update path on ticks >= 2 (a1mpc.h): what its persistent OSQP workspace carries
        if (!h->d_carry) {
            const size_t bytes = static_cast<size_t>(h->max_batch) * carry_stride(h->cfg.horizon) * sizeof(double);
            A1_HIP(hipMalloc(&h->d_carry, bytes));
            A1_HIP(hipMemsetAsync(h->d_carry, 0, bytes, s));
        }
        a.carry = h->d_carry;
    }
    h->last_ws_mode = (h->cfg.warm_start == 2 && a.carry == nullptr) ? 1 : h->cfg.warm_start;   // (the general path's split pipeline revises this below)
    a.contact_stride = contact_stride;  // a per-step contact schedule alone (feet step-invariant) stays on the fast path: contacts only change bounds and equality rows
    if (foot_stride != 0 || d_yaw_A != nullptr) {  // general path: per-step B_d (and / or its own A_c yaw), with or without a contact schedule
        // (tick records too -- a1mpc_solve_batch_ticks_strided: RowSolver::setup builds x0 / x_ref from the record in the GEN instantiations as on the fast path, and
        // a1mpc_predict_kernel reads either form; nothing else of the general path touches x0 / x_ref)
        a.foot_stride = foot_stride; a.contact_stride = contact_stride; a.yaw_A = d_yaw_A;
        // a batch beyond the resident rows of the general path's ADMM kernel runs its split pipeline (set-up kernel + persistent rows on a queue, like the
        // fast path); its hand-off records (B~w_t of every step included) live in a buffer of their own, allocated on first use
        int rows_gen = 0;
        if (a1mpc_status st0 = resident_rows_gen(ops, &rows_gen); st0 != A1MPC_OK) return st0;
        bool split_gen = pipeline_mode() != 2 && rows_gen > 0 && (pipeline_mode() == 1 || n > rows_gen) && h->d_counter != nullptr;
        // warm_start = 2: the FUSED general kernels follow the update path like the fast path's (round 5: batches within the resident rows).  Round 6: every batch size --
        // an update-path batch beyond the resident rows runs the fused kernel as well, in as many rounds as it takes (the hardware dispatches the grid's workgroups as
        // LDS frees up).  Ticks on the update path are warm-started and all alike (25 iterations once the loop is closed): there is nothing for a queue to balance, which
        // is why the fast path's warm ticks of a known batch take the fused kernel too (solve_device_impl below); only the very first tick of a fleet (cold, no
        // history) pays a tail for it.  The general path's split pipeline itself has no update-path hand-off and keeps serving modes 0 / 1.
        if (a.carry != nullptr && split_gen && pipeline_mode() != 1) split_gen = false;
        if (a.carry != nullptr && split_gen) {   // (A1MPC_PIPELINE=split forced: warm_start = 1 semantics, visibly -- the carry is marked "no previous tick" so that a later
                                                 // update-path tick does not pair stale scalings with fresh iterates)
            A1_HIP(hipMemset2DAsync(h->d_carry, carry_stride(h->cfg.horizon) * sizeof(double), 0, sizeof(double), static_cast<size_t>(n), s));
            a.carry = nullptr;
            h->last_ws_mode = 1;
        }
        if (split_gen && !h->d_prep_gen) {
            A1_HIP(hipMalloc(&h->d_prep_gen, static_cast<size_t>(h->max_batch) * ops.prep_stride_gen * sizeof(double)));
        }
        const bool hints_gen = h->schedule && split_gen && n >= kScheduleMinBatch && h->d_order != nullptr && h->d_cost != nullptr;
        a.order = hints_gen ? h->d_order : nullptr;
        a.cost = hints_gen ? h->d_cost : nullptr;
        a.predict = (hints_gen && h->hint_n != -n) ? 1 : 0;  // (the history of a general-path batch is remembered as -n: never mixed up with a fast-path batch of the same size)
        h->staged = split_gen && h->timing;
        if (h->timing) A1_HIP(hipEventRecord(h->ev0, s));
        if (split_gen) {
            static const bool pipe_hint = [] { const char* e = getenv("A1MPC_GEN_PIPE_ONE_WAVE"); return !(e && !strcmp(e, "0")); }();
            g_gen_prefer_one_wave = pipe_hint && h->pipeline_depth == 2;
            const a1mpc_status stg = ops.launch_gen_split(a, h->d_prep_gen, h->d_counter, s, h->timing ? h->ev_mid : nullptr);   // (split_gen: the horizon has a general path)
            g_gen_prefer_one_wave = false;
            if (stg != A1MPC_OK) return stg;
            if (hints_gen) h->hint_n = -n;   // the cost buffer now holds this batch's costs: the next general-path solve of this size is ordered by them
        } else {
            if (a1mpc_status stg = ops.launch_gen ? ops.launch_gen(a, s) : no_general_path(); stg != A1MPC_OK) return stg;
        }
        if (h->timing) A1_HIP(hipEventRecord(h->ev1, s));
        h->timed = h->timing;
        A1_MARK(h, s);
        return A1MPC_OK;
    }
    // Straggler-aware queue order: batches beyond the resident rows are issued longest-first by the cost each QP had in the previous solve of
    // this handle (the same robots tick after tick); the first solve of a batch size is ordered by the set-up kernel's cost guess
    // (RowSolver::predict_cost).  Scheduling only.
    bool split = false;
    if (a1mpc_status st0 = use_split_pipeline(ops, n, h->d_prep != nullptr, &split); st0 != A1MPC_OK) return st0;
    // Warm-started ticks of the same robots (the closed-loop regime: second and later ticks of a batch size) take ~25 iterations each, all alike: nothing is left
    // for the queue to balance, and the fused kernel -- set-up and solve in one launch, no hand-off through memory, no kernel boundary for the rows to idle at --
    // wins up to a few rounds of the resident rows (4096 x h10: 0.397 -> 0.350 ms per tick, 8192: 0.665 -> 0.652; profiles/r04_warm_ticks_fused_vs_split.txt).
    // Same results bit for bit (the pipelines are tested against each other).  A1MPC_WARM_FUSED=0 keeps the split pipeline (A/B runs).
    bool warm_fused = false;
    if (split && h->cfg.warm_start != 0 && h->hint_n == n && pipeline_mode() == 0 && warm_fused_enabled() && n <= warm_fused_max(h->cfg.horizon)) { split = false; warm_fused = true; }
    const bool hints = h->schedule && split && n >= kScheduleMinBatch;
    a.order = hints ? h->d_order : nullptr;
    a.cost = hints ? h->d_cost : nullptr;
    a.predict = (hints && h->hint_n != n) ? 1 : 0;  // first solve of this batch size: order by the set-up kernel's guess instead
    if (h->timing) A1_HIP(hipEventRecord(h->ev0, s)); else if (tick_markers() & 1) A1_HIP(hipEventRecord(h->ev_mark, s));
    // Round 5 trial (opt-in, see warm_order_enabled): the fused kernel of a warm-started tick launches its workgroups in the order of the previous tick's per-QP
    // cost, longest first (the cost buffer holds it: hint_n == n; the fused kernel records this tick's).  Scheduling only: every result is bit-identical in any order.
    if (warm_fused && h->schedule && n >= kScheduleMinBatch && n > coop_max_batch() && warm_order_enabled()) {
        RoctxRange range("a1mpc order");
        launch_order_kernel(static_cast<int>(n), static_cast<const int32_t*>(h->d_cost), h->d_order, s);
        A1_HIP(hipGetLastError());
        a.order = h->d_order; a.cost = h->d_cost;
    }
    if (tq != nullptr && !split && h->cfg.horizon > 1) {   // the fused / latency kernels write the joint torques in their output stage
        a.tq_active = tq->active; a.tq_J = tq->J; a.tq_fkin = tq->fkin; a.tq_tg = tq->tg; a.tq_km = tq->km; a.tq_tau = tq->tau;
        tq->fused = true;
    }
    h->staged = split && h->timing;
    h->clk_n = 0; h->clk_tick = false;
    if (h->profiling && h->cfg.horizon > 1 && a.contact_stride == 0) {
        if (!h->d_clk) A1_HIP(hipMalloc(&h->d_clk, static_cast<size_t>(h->max_batch) * kTickStages * sizeof(long long)));
        A1_HIP(hipMemsetAsync(h->d_clk, 0, static_cast<size_t>(n) * kTickStages * sizeof(long long), s));
        a.clk = h->d_clk;
    }
    g_clk_ran = false;
    a1mpc_status st = launch_mpc(ops, a, h->d_prep, h->d_counter, s, split, h->timing ? h->ev_mid : nullptr);
    if (st != A1MPC_OK) return st;
    if (a.clk != nullptr && g_clk_ran) { h->clk_n = n; h->clk_tick = !split; }   // (a kernel without stamps ran: the record stays "not profiled")
    if (hints) h->hint_n = n;   // the cost buffer now holds this batch's costs: the next solve of this size is ordered by them (sorted in front of its ADMM kernel)
    if (h->timing) A1_HIP(hipEventRecord(h->ev1, s)); else if (tick_markers() & 4) A1_HIP(hipEventRecord(h->ev_mark, s));
    h->timed = h->timing;
    A1_MARK(h, s);
    return A1MPC_OK;
}

a1mpc_status a1mpc_solve_batch_device(a1mpc_handle h, int32_t n, const double* d_x0, const double* d_x_ref, const double* d_R_world,
                                      const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out,
                                      double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream) {
    if (!d_x0 || !d_x_ref) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return solve_device_impl(h, n, nullptr, d_x0, d_x_ref, d_R_world, d_foot_abs, d_contact, d_grf_body_out, d_u_full_out, d_iters_out,
                             d_status_out, hip_stream);
}
a1mpc_status a1mpc_solve_batch_ticks_device(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_R_world,
                                            const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out,
                                            double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream) {
    if (!d_tick) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return solve_device_impl(h, n, d_tick, nullptr, nullptr, d_R_world, d_foot_abs, d_contact, d_grf_body_out, d_u_full_out, d_iters_out,
                             d_status_out, hip_stream);
}

static bool strides_ok(int32_t foot_stride, int32_t contact_stride) {
    return (foot_stride == 0 || foot_stride == 12) && (contact_stride == 0 || contact_stride == 4);
}
// Tick records joined with the strides of a1mpc_solve_batch_strided: (0, 0, NULL) is a1mpc_solve_batch_ticks_device, (0, 4, NULL) the fast kernels with a schedule,
// per-step feet / a yaw_A the general kernels -- all of them build x0 / x_ref from the record in their set-up (RowSolver::setup)
a1mpc_status a1mpc_solve_batch_ticks_strided_device(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_R_world, const double* d_foot_abs,
                                                    int32_t foot_stride, const uint8_t* d_contact, int32_t contact_stride, const double* d_yaw_A,
                                                    double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream) {
    if (!d_tick) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (!strides_ok(foot_stride, contact_stride)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    if (h && h->cfg.horizon < 2) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "tick records need horizon >= 2");
    return solve_device_impl(h, n, d_tick, nullptr, nullptr, d_R_world, d_foot_abs, d_contact, d_grf_body_out, d_u_full_out, d_iters_out, d_status_out, hip_stream,
                             foot_stride, contact_stride, d_yaw_A);
}

// ---- the gait-aware horizon: a1mpc_horizon_preview_kernel behind the C ABI
void a1mpc_default_preview_config(a1mpc_preview_config* c) {
    if (!c) return;
    c->contact_schedule = 1; c->foot_preview = 0; c->ticks_per_step = 1;
}
// what a1mpc_horizon_preview_batch(_device) and a1mpc_control_tick_preview_device refuse, or null
static const char* invalid_preview(a1mpc_handle h, const a1mpc_preview_config* pv) {
    if (!h) return "null handle";
    if (!pv) return "null a1mpc_preview_config";
    if (pv->ticks_per_step < 1 || pv->ticks_per_step > 64) return "a1mpc_preview_config.ticks_per_step must be 1..64";
    if (pv->foot_preview < 0 || pv->foot_preview > 2) return "a1mpc_preview_config.foot_preview must be 0, 1 or 2";
    if (pv->contact_schedule < 0 || pv->contact_schedule > 1) return "a1mpc_preview_config.contact_schedule must be 0 or 1";
    if (h->cfg.horizon < 2) return "a horizon preview needs horizon >= 2 (a1mpc_config.horizon)";
    return nullptr;
}
// the launch alone (arguments validated by the caller, which also orders and marks the stream)
static void launch_preview(a1mpc_handle h, const a1mpc_preview_config& pv, double counter_per_gait, double counter_per_swing, int32_t n, const uint8_t* movement_mode,
                           const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts, const double* foot_pos_abs, const double* R_world,
                           const double* root_lin_vel_d, uint8_t* sched_out, double* foot_steps_out, hipStream_t s, const double* foot_target_abs = nullptr) {
    PreviewArgs a;
    a.n = n; a.H = h->cfg.horizon; a.ticks_per_step = pv.ticks_per_step; a.sched_mode = pv.contact_schedule; a.foot_mode = pv.foot_preview;
    a.counter_per_gait = counter_per_gait; a.counter_per_swing = counter_per_swing; a.dt = h->cfg.dt;
    a.movement_mode = movement_mode; a.contacts = contacts; a.gait_counter = gait_counter; a.gait_counter_speed = gait_counter_speed;
    a.foot_pos_abs = foot_pos_abs; a.Rw = R_world; a.root_lin_vel_d = root_lin_vel_d;
    a.sched = reinterpret_cast<uint32_t*>(sched_out); a.foot_steps = foot_steps_out;
    // the footholds replace a foot only at a touchdown, and only a schedule has one: without target, feet or schedule the existing kernel IS the rule
    a.foot_target_abs = foot_steps_out != nullptr && pv.contact_schedule == 1 ? foot_target_abs : nullptr;
    if (a.foot_target_abs) hipLaunchKernelGGL(a1mpc_horizon_preview_footholds_kernel, leg_lane_grid(n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(a1mpc_horizon_preview_kernel, leg_lane_grid(n), dim3(256), 0, s, a);
}
// pointer rules shared by the two preview entries: each output needs its inputs
static const char* invalid_preview_io(const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, const uint8_t* movement_mode, const double* gait_counter,
                                      const double* gait_counter_speed, const uint8_t* contacts, const double* foot_pos_abs, const double* R_world,
                                      const double* root_lin_vel_d, const uint8_t* sched_out, const double* foot_steps_out, bool device) {
    if (!gait) return "null a1mpc_gait_config";
    if (!(gait->counter_per_gait > 0)) return "a1mpc_gait_config.counter_per_gait <= 0";
    if (!sched_out && !foot_steps_out) return "null input/output pointer";
    if (sched_out && (!contacts || (pv->contact_schedule == 1 && (!movement_mode || !gait_counter || !gait_counter_speed)))) return "null input/output pointer";
    if (foot_steps_out && pv->foot_preview == 0) return "foot_steps_out needs a1mpc_preview_config.foot_preview 1 or 2";
    if (foot_steps_out && (!foot_pos_abs || !root_lin_vel_d || (pv->foot_preview == 2 && !R_world))) return "null input/output pointer";
    if (device && (reinterpret_cast<uintptr_t>(sched_out) & 3u)) return "contact_sched_out must be 4-byte aligned (it is written one horizon step, four contact bytes, at a time)";
    return nullptr;
}
// what the foothold entries refuse beyond invalid_preview_io, or null: feet without their target, and -- the footholds read the schedule -- feet under contact_schedule 1
// without the schedule's inputs, whether or not the schedule itself is an output
static const char* invalid_footholds_io(const a1mpc_preview_config* pv, const uint8_t* movement_mode, const double* gait_counter, const double* gait_counter_speed,
                                        const uint8_t* contacts, const double* foot_pos_target_abs, const double* foot_steps_out) {
    if (!foot_steps_out) return nullptr;
    if (!foot_pos_target_abs) return "foot_steps_out needs foot_pos_target_abs (null)";
    if (pv->contact_schedule != 1) return nullptr;
    if (!movement_mode) return "null movement_mode: the footholds read the schedule (contact_schedule 1)";
    if (!gait_counter) return "null gait_counter: the footholds read the schedule (contact_schedule 1)";
    if (!gait_counter_speed) return "null gait_counter_speed: the footholds read the schedule (contact_schedule 1)";
    if (!contacts) return "null contacts: the footholds read the schedule (contact_schedule 1)";
    return nullptr;
}
static a1mpc_status preview_device_impl(a1mpc_handle h, const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                        const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts, const double* foot_pos_abs,
                                        const double* R_world, const double* root_lin_vel_d, bool footholds, const double* foot_pos_target_abs, uint8_t* sched_out,
                                        double* foot_steps_out, void* hip_stream) {
    if (const char* bad = invalid_preview(h, pv)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");
    if (const char* bad = invalid_preview_io(pv, gait, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world, root_lin_vel_d, sched_out, foot_steps_out, true))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (footholds)
        if (const char* bad = invalid_footholds_io(pv, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_target_abs, foot_steps_out))
            return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_preview(h, *pv, gait->counter_per_gait, gait->counter_per_swing, n, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world,
                                   root_lin_vel_d, sched_out, foot_steps_out, s, footholds ? foot_pos_target_abs : nullptr));
    return A1MPC_OK;
}
a1mpc_status a1mpc_horizon_preview_batch_device(a1mpc_handle h, const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, int32_t n,
                                                const uint8_t* movement_mode, const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts,
                                                const double* foot_pos_abs, const double* R_world, const double* root_lin_vel_d, uint8_t* sched_out,
                                                double* foot_steps_out, void* hip_stream) {
    return preview_device_impl(h, pv, gait, n, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world, root_lin_vel_d, false, nullptr, sched_out,
                               foot_steps_out, hip_stream);
}
// a1mpc_horizon_preview_batch_device with the foothold rule: a leg that the schedule puts down inside the horizon stands at foot_pos_target_abs from that step on
a1mpc_status a1mpc_horizon_preview_footholds_batch_device(a1mpc_handle h, const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, int32_t n,
                                                          const uint8_t* movement_mode, const double* gait_counter, const double* gait_counter_speed,
                                                          const uint8_t* contacts, const double* foot_pos_abs, const double* R_world, const double* root_lin_vel_d,
                                                          const double* foot_pos_target_abs, uint8_t* sched_out, double* foot_steps_out, void* hip_stream) {
    return preview_device_impl(h, pv, gait, n, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world, root_lin_vel_d, true, foot_pos_target_abs,
                               sched_out, foot_steps_out, hip_stream);
}
// the handle's per-step staging (a1mpc_solve_batch_strided's too): n x 12H feet, n x 4H contact bytes
static a1mpc_status ensure_step_staging(a1mpc_handle h) {
    if (h->d_foot_steps) return A1MPC_OK;
    const size_t H = h->cfg.horizon;
    A1_HIP(hipMalloc(&h->d_foot_steps, static_cast<size_t>(h->max_batch) * 12 * H * sizeof(double)));
    A1_HIP(hipMalloc(&h->d_contact_steps, static_cast<size_t>(h->max_batch) * 4 * H));
    return A1MPC_OK;
}
static a1mpc_status preview_host_impl(a1mpc_handle h, const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                      const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts, const double* foot_pos_abs,
                                      const double* R_world, const double* root_lin_vel_d, bool footholds, const double* foot_pos_target_abs, uint8_t* sched_out,
                                      double* foot_steps_out) {
    if (const char* bad = invalid_preview(h, pv)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");
    if (const char* bad = invalid_preview_io(pv, gait, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world, root_lin_vel_d, sched_out, foot_steps_out,
                                             false)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);   // (a host array for the schedule may sit at any address: it is staged)
    if (footholds)
        if (const char* bad = invalid_footholds_io(pv, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_target_abs, foot_steps_out))
            return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    const bool with_target = footholds && foot_steps_out != nullptr;   // (without feet to produce the call IS the existing entry: the target is not read, not even staged)
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    if (a1mpc_status st = ensure_step_staging(h); st != A1MPC_OK) return st;
    // (an input that the configured preview does not read may be null: its slice is handed to the kernel unfilled.)  Out: the handle's per-step buffers
    const double *d_gc = sg.in(gait_counter, 4), *d_spd = sg.in(gait_counter_speed, 4), *d_fp = sg.in(foot_pos_abs, 12), *d_R = sg.in(R_world, 9), *d_vd = sg.in(root_lin_vel_d, 3);
    const uint8_t *d_mm = sg.in(movement_mode, 1), *d_ct = sg.in(contacts, 4);
    const double* d_tg = with_target ? sg.in(foot_pos_target_abs, 12) : nullptr;
    const size_t H = h->cfg.horizon;
    sg.back(sched_out, h->d_contact_steps, 4 * H);
    sg.back(foot_steps_out, h->d_foot_steps, 12 * H);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_preview(h, *pv, gait->counter_per_gait, gait->counter_per_swing, n, d_mm, d_gc, d_spd, d_ct, d_fp, d_R, d_vd, sched_out ? h->d_contact_steps : nullptr,
                                   foot_steps_out ? h->d_foot_steps : nullptr, s, d_tg));
    return sg.finish();
}
a1mpc_status a1mpc_horizon_preview_batch(a1mpc_handle h, const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                         const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts, const double* foot_pos_abs,
                                         const double* R_world, const double* root_lin_vel_d, uint8_t* sched_out, double* foot_steps_out) {
    return preview_host_impl(h, pv, gait, n, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world, root_lin_vel_d, false, nullptr, sched_out,
                             foot_steps_out);
}
a1mpc_status a1mpc_horizon_preview_footholds_batch(a1mpc_handle h, const a1mpc_preview_config* pv, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                                   const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts, const double* foot_pos_abs,
                                                   const double* R_world, const double* root_lin_vel_d, const double* foot_pos_target_abs, uint8_t* sched_out,
                                                   double* foot_steps_out) {
    return preview_host_impl(h, pv, gait, n, movement_mode, gait_counter, gait_counter_speed, contacts, foot_pos_abs, R_world, root_lin_vel_d, true, foot_pos_target_abs,
                             sched_out, foot_steps_out);
}

// ---- predicted horizon states and cost of a force plan: a1mpc_horizon_states_kernel behind the C ABI
// what the four entries refuse, or null (all before the first HIP call).  `state` is x0 or, for the tick entries, the tick record
static const char* invalid_horizon_states(a1mpc_handle h, int32_t n, bool ticks, const double* state, const double* x_ref, const double* R_world, const double* foot_abs,
                                          int32_t foot_stride, const double* x_pred_out, const double* cost_out) {
    if (!h) return "null handle";
    if (n < 0) return "negative n";
    if (n > h->max_batch) return "n > max_batch given to a1mpc_create";
    if (foot_stride != 0 && foot_stride != 12) return "foot_stride must be 0 or 12";
    if (!x_pred_out && !cost_out) return "x_pred_out and cost_out are both null";
    if (!ticks && cost_out && !x_ref) return "cost_out needs x_ref (null)";
    if (!state) return ticks ? "null tick" : "null x0";
    if (!R_world) return "null R_world";
    if (!foot_abs) return "null foot_abs";
    if (h->cfg.horizon < 2) return "the predicted horizon states need horizon >= 2 (a1mpc_config.horizon)";
    return nullptr;
}
// the launch alone: device pointers, validated by the caller, which also orders and marks the stream.  One wavefront per workgroup, 16 QPs each
static void launch_horizon_states(a1mpc_handle h, int32_t n, bool ticks, const double* state, const double* x_ref, const double* R_world, const double* foot_abs,
                                  int32_t foot_stride, const double* yaw_A, const double* u_full, double* x_pred_out, double* cost_out, hipStream_t s) {
    HorizonStatesArgs a;
    const a1mpc_config& c = h->cfg;
    a.n = n; a.H = c.horizon; a.foot_stride = foot_stride; a.dt = c.dt; a.mass = c.mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = c.inertia_body[i];
    for (int i = 0; i < 12; ++i) { a.q[i] = c.q[i]; a.r[i] = c.r[i]; }
    a.x0 = ticks ? nullptr : state; a.tick = ticks ? state : nullptr; a.xref = ticks ? nullptr : x_ref;
    a.R = R_world; a.foot = foot_abs; a.yaw_A = yaw_A; a.u = u_full; a.x_pred = x_pred_out; a.cost = cost_out;
    hipLaunchKernelGGL(a1mpc_horizon_states_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, a);
}
static a1mpc_status horizon_states_device_impl(a1mpc_handle h, int32_t n, bool ticks, const double* d_state, const double* d_x_ref, const double* d_R_world,
                                               const double* d_foot_abs, int32_t foot_stride, const double* d_yaw_A, const double* d_u_full, double* d_x_pred_out,
                                               double* d_cost_out, void* hip_stream) {
    if (const char* bad = invalid_horizon_states(h, n, ticks, d_state, d_x_ref, d_R_world, d_foot_abs, foot_stride, d_x_pred_out, d_cost_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_horizon_states(h, n, ticks, d_state, d_x_ref, d_R_world, d_foot_abs, foot_stride, d_yaw_A, d_u_full, d_x_pred_out, d_cost_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_horizon_states_batch_device(a1mpc_handle h, int32_t n, const double* d_x0, const double* d_x_ref, const double* d_R_world, const double* d_foot_abs,
                                               int32_t foot_stride, const double* d_yaw_A, const double* d_u_full, double* d_x_pred_out, double* d_cost_out,
                                               void* hip_stream) {
    return horizon_states_device_impl(h, n, false, d_x0, d_x_ref, d_R_world, d_foot_abs, foot_stride, d_yaw_A, d_u_full, d_x_pred_out, d_cost_out, hip_stream);
}
a1mpc_status a1mpc_horizon_states_ticks_batch_device(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_R_world, const double* d_foot_abs,
                                                     int32_t foot_stride, const double* d_yaw_A, const double* d_u_full, double* d_x_pred_out, double* d_cost_out,
                                                     void* hip_stream) {
    return horizon_states_device_impl(h, n, true, d_tick, nullptr, d_R_world, d_foot_abs, foot_stride, d_yaw_A, d_u_full, d_x_pred_out, d_cost_out, hip_stream);
}
// the host-pointer entries: the per-QP arrays go through Staging, the per-step ones (13H / 12H doubles per QP, more than its slices hold) through the handle's
// per-step buffers -- d_xref and d_foot_steps, which the solve entries' host paths fill anew at every call, and two of this stage's own
static a1mpc_status horizon_states_host_impl(a1mpc_handle h, int32_t n, bool ticks, const double* state, const double* x_ref, const double* R_world, const double* foot_abs,
                                             int32_t foot_stride, const double* yaw_A, const double* u_full, double* x_pred_out, double* cost_out) {
    if (const char* bad = invalid_horizon_states(h, n, ticks, state, x_ref, R_world, foot_abs, foot_stride, x_pred_out, cost_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const size_t H = h->cfg.horizon, N = static_cast<size_t>(n), cap = static_cast<size_t>(h->max_batch);
    if (foot_stride)
        if (a1mpc_status st = ensure_step_staging(h); st != A1MPC_OK) return st;
    if (u_full && !h->d_hs_u) A1_HIP(hipMalloc(&h->d_hs_u, cap * 12 * H * sizeof(double)));
    if (x_pred_out && !h->d_hs_x) A1_HIP(hipMalloc(&h->d_hs_x, cap * 13 * H * sizeof(double)));
    const double *d_state = sg.in(state, ticks ? 22 : 13), *d_R = sg.in(R_world, 9), *d_yaw = yaw_A ? sg.in(yaw_A, 1) : nullptr;
    const double* d_foot = foot_stride ? h->d_foot_steps : sg.in(foot_abs, 12);
    const bool with_ref = !ticks && x_ref && cost_out;   // (x_ref is read by the cost alone)
    if (with_ref) sg.hip(hipMemcpyAsync(h->d_xref, x_ref, N * 13 * H * sizeof(double), hipMemcpyHostToDevice, s), "hipMemcpyAsync (x_ref)");
    if (foot_stride) sg.hip(hipMemcpyAsync(h->d_foot_steps, foot_abs, N * 12 * H * sizeof(double), hipMemcpyHostToDevice, s), "hipMemcpyAsync (per-step feet)");
    if (u_full) sg.hip(hipMemcpyAsync(h->d_hs_u, u_full, N * 12 * H * sizeof(double), hipMemcpyHostToDevice, s), "hipMemcpyAsync (u_full)");
    double* d_cost = sg.out(cost_out, 2);
    sg.back(x_pred_out, h->d_hs_x, 13 * H);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_horizon_states(h, n, ticks, d_state, with_ref ? h->d_xref : nullptr, d_R, d_foot, foot_stride, d_yaw, u_full ? h->d_hs_u : nullptr,
                                          x_pred_out ? h->d_hs_x : nullptr, d_cost, s));
    return sg.finish();
}
a1mpc_status a1mpc_horizon_states_batch(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world, const double* foot_abs, int32_t foot_stride,
                                        const double* yaw_A, const double* u_full, double* x_pred_out, double* cost_out) {
    return horizon_states_host_impl(h, n, false, x0, x_ref, R_world, foot_abs, foot_stride, yaw_A, u_full, x_pred_out, cost_out);
}
a1mpc_status a1mpc_horizon_states_ticks_batch(a1mpc_handle h, int32_t n, const double* tick, const double* R_world, const double* foot_abs, int32_t foot_stride,
                                              const double* yaw_A, const double* u_full, double* x_pred_out, double* cost_out) {
    return horizon_states_host_impl(h, n, true, tick, nullptr, R_world, foot_abs, foot_stride, yaw_A, u_full, x_pred_out, cost_out);
}
// ---- the plant step behind the C ABI: a1mpc_plant_step_kernel, no handle state
void a1mpc_default_plant_config(a1mpc_plant_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->dt = 0.0025; c->substeps = 1; c->gravity_z = -9.8;
}
// what the two entries refuse, or null (all before the first HIP call)
static const char* invalid_plant_step(a1mpc_handle h, const a1mpc_plant_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                      const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* state_out, const double* R_world_out,
                                      const double* foot_abs_out) {
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_plant_config";
    if (cfg->substeps < 1 || cfg->substeps > 64) return "a1mpc_plant_config.substeps outside 1 .. 64";
    if (!(cfg->dt > 0.0) || !std::isfinite(cfg->dt)) return "a1mpc_plant_config.dt must be positive and finite";
    if (!std::isfinite(cfg->gravity_z)) return "a1mpc_plant_config.gravity_z must be finite";
    if (state_stride != 12 && state_stride != 13 && state_stride != 22) return "state_stride must be 12, 13 or 22";
    if (n < 0) return "negative n";
    if (n > h->max_batch) return "n > max_batch given to a1mpc_create";
    if (!state_in) return "null state_in";
    if (!R_world) return "null R_world";
    if (!foot_abs) return "null foot_abs";
    if (!grf_body) return "null grf_body";
    if (!contacts) return "null contacts";
    if (!state_out) return "null state_out";
    if (!R_world_out) return "null R_world_out";
    if (!foot_abs_out) return "null foot_abs_out";
    return nullptr;
}
// the launch alone: device pointers, validated by the caller, which also orders and marks the stream.  One wavefront per workgroup, 16 robots each
static void launch_plant_step(a1mpc_handle h, const a1mpc_plant_config& cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                              const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, double* state_out, double* R_world_out,
                              double* foot_abs_out, hipStream_t s) {
    PlantArgs a;
    a.n = n; a.stride = state_stride; a.substeps = cfg.substeps; a.dt = cfg.dt; a.gravity = cfg.gravity_z; a.mass = h->cfg.mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = h->cfg.inertia_body[i];
    a.state = state_in; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.state_out = state_out; a.R_out = R_world_out; a.foot_out = foot_abs_out;
    hipLaunchKernelGGL(a1mpc_plant_step_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, a);
}
a1mpc_status a1mpc_plant_step_batch_device(a1mpc_handle h, const a1mpc_plant_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                           const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                           const double* d_ext_wrench, double* d_state_out, double* d_R_world_out, double* d_foot_abs_out, void* hip_stream) {
    if (const char* bad = invalid_plant_step(h, cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_state_out, d_R_world_out, d_foot_abs_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_plant_step(h, *cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, d_state_out, d_R_world_out,
                                      d_foot_abs_out, s));
    return A1MPC_OK;
}
// the host-pointer entry: every array through Staging.  The device step runs IN PLACE on the staged inputs; where a state row is wider than the 12 words the kernel
// writes and state_out is another array than state_in, state_out's own rows are staged in as well, so that the words the step does not write go back as they came
a1mpc_status a1mpc_plant_step_batch(a1mpc_handle h, const a1mpc_plant_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                    const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, double* state_out,
                                    double* R_world_out, double* foot_abs_out) {
    if (const char* bad = invalid_plant_step(h, cfg, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, state_out, R_world_out, foot_abs_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const size_t W = static_cast<size_t>(state_stride);
    double *d_state = sg.in(state_in, W), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12);
    const double *d_grf = sg.in(grf_body, 12), *d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr;
    const uint8_t* d_ct = sg.in(contacts, 4);
    double* d_out = (W == 12 || state_out == state_in) ? d_state : sg.in(static_cast<const double*>(state_out), W);
    sg.back(state_out, d_out, W); sg.back(R_world_out, d_R, 9); sg.back(foot_abs_out, d_foot, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_plant_step(h, *cfg, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, d_out, d_R, d_foot, s));
    return sg.finish();
}
// ---- sensor synthesis behind the C ABI: a1mpc_sensor_synthesis_kernel, no handle state
// what the two entries refuse, or null (all before the first HIP call; n > max_batch is A1_STAGE_DEVICE's)
static const char* invalid_sensor_synthesis(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                            const double* grf_body, const uint8_t* contacts, const double* rho_fix, const double* rho_opt, const double* quat_out,
                                            const double* imu_acc_raw_out, const double* imu_gyro_raw_out, const double* joint_pos_out, const double* joint_vel_out,
                                            const double* foot_force_out, const uint8_t* reach_out) {
    if (!h) return "null handle";
    if (state_stride != 12 && state_stride != 13 && state_stride != 22) return "state_stride must be 12, 13 or 22";
    if (n < 0) return "negative n";
    if (!state) return "null state";
    if (!R_world) return "null R_world";
    if (!foot_abs) return "null foot_abs";
    if (!grf_body) return "null grf_body";
    if (!contacts) return "null contacts";
    if (!rho_fix) return "null rho_fix";
    if (!rho_opt) return "null rho_opt";
    if (!quat_out) return "null quat_out";
    if (!imu_acc_raw_out) return "null imu_acc_raw_out";
    if (!imu_gyro_raw_out) return "null imu_gyro_raw_out";
    if (!joint_pos_out) return "null joint_pos_out";
    if (!joint_vel_out) return "null joint_vel_out";
    if (!foot_force_out) return "null foot_force_out";
    if (!reach_out) return "null reach_out";
    for (int k = 0; k < 20; ++k) if (!std::isfinite(rho_fix[k])) return "rho_fix holds a value that is not finite";
    for (int k = 0; k < 12; ++k) if (!std::isfinite(rho_opt[k])) return "rho_opt holds a value that is not finite";
    for (int l = 0; l < 4; ++l) {
        const double lt = rho_fix[5 * l + 3], al = rho_fix[5 * l + 4] - rho_opt[3 * l + 2], r0 = rho_opt[3 * l];
        if (!(lt > 0.0)) return "rho_fix: the upper leg length must be positive";
        if (al * al + r0 * r0 == 0.0) return "rho_fix / rho_opt: the lower leg has no length";
    }
    return nullptr;
}
// the launch alone: device pointers (the geometry: host), validated by the caller, which also orders and marks the stream.  One wavefront per workgroup, 16 robots each
static void launch_sensor_synthesis(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                    const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* rho_fix, const double* rho_opt, double* quat_out,
                                    double* imu_acc_raw_out, double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out, double* foot_force_out,
                                    uint8_t* reach_out, double* foot_pos_rel_out, double* foot_vel_rel_out, hipStream_t s) {
    SynthArgs a;
    a.n = n; a.stride = state_stride; a.mass = h->cfg.mass;
    std::memcpy(a.rho_fix, rho_fix, sizeof a.rho_fix); std::memcpy(a.rho_opt, rho_opt, sizeof a.rho_opt);
    a.state = state; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.quat = quat_out; a.acc = imu_acc_raw_out; a.gyro = imu_gyro_raw_out; a.jpos = joint_pos_out; a.jvel = joint_vel_out; a.fforce = foot_force_out;
    a.prel = foot_pos_rel_out; a.vrel = foot_vel_rel_out; a.reach = reach_out;
    hipLaunchKernelGGL(a1mpc_sensor_synthesis_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, a);
}
a1mpc_status a1mpc_sensor_synthesis_batch_device(a1mpc_handle h, int32_t n, const double* d_state, int32_t state_stride, const double* d_R_world, const double* d_foot_abs,
                                                 const double* d_grf_body, const uint8_t* d_contacts, const double* d_ext_wrench, const double* rho_fix,
                                                 const double* rho_opt, double* d_quat_out, double* d_imu_acc_raw_out, double* d_imu_gyro_raw_out, double* d_joint_pos_out,
                                                 double* d_joint_vel_out, double* d_foot_force_out, uint8_t* d_reach_out, double* d_foot_pos_rel_out,
                                                 double* d_foot_vel_rel_out, void* hip_stream) {
    if (const char* bad = invalid_sensor_synthesis(h, n, d_state, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, rho_fix, rho_opt, d_quat_out, d_imu_acc_raw_out,
                                                   d_imu_gyro_raw_out, d_joint_pos_out, d_joint_vel_out, d_foot_force_out, d_reach_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_sensor_synthesis(h, n, d_state, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, rho_fix, rho_opt, d_quat_out,
                                            d_imu_acc_raw_out, d_imu_gyro_raw_out, d_joint_pos_out, d_joint_vel_out, d_foot_force_out, d_reach_out, d_foot_pos_rel_out,
                                            d_foot_vel_rel_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_sensor_synthesis_batch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                          const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* rho_fix, const double* rho_opt,
                                          double* quat_out, double* imu_acc_raw_out, double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out,
                                          double* foot_force_out, uint8_t* reach_out, double* foot_pos_rel_out, double* foot_vel_rel_out) {
    if (const char* bad = invalid_sensor_synthesis(h, n, state, state_stride, R_world, foot_abs, grf_body, contacts, rho_fix, rho_opt, quat_out, imu_acc_raw_out,
                                                   imu_gyro_raw_out, joint_pos_out, joint_vel_out, foot_force_out, reach_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const double *d_state = sg.in(state, static_cast<size_t>(state_stride)), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12), *d_grf = sg.in(grf_body, 12);
    const double* d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr;
    const uint8_t* d_ct = sg.in(contacts, 4);
    double *d_quat = sg.out(quat_out, 4), *d_acc = sg.out(imu_acc_raw_out, 3), *d_gyro = sg.out(imu_gyro_raw_out, 3), *d_jp = sg.out(joint_pos_out, 12);
    double *d_jv = sg.out(joint_vel_out, 12), *d_ff = sg.out(foot_force_out, 4), *d_pr = sg.out(foot_pos_rel_out, 12), *d_vr = sg.out(foot_vel_rel_out, 12);
    uint8_t* d_reach = sg.out(reach_out, 4);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_sensor_synthesis(h, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, rho_fix, rho_opt, d_quat, d_acc, d_gyro, d_jp, d_jv, d_ff, d_reach,
                                            d_pr, d_vr, s));
    return sg.finish();
}
// ---- the walking plant behind the C ABI: a1mpc_walk_step_kernel and a1mpc_walk_sensors_kernel, no handle state
void a1mpc_default_walk_config(a1mpc_walk_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    a1mpc_default_plant_config(&c->plant);
    c->swing_track = 1.0; c->flat_ground = 0; c->ground_z = 0.0;
}
// what the two step entries refuse, or null (all before the first HIP call): the plant step's refusals, then the walk's own
static const char* invalid_walk_step(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                     const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* R_z, const double* foot_target,
                                     const double* state_out, const double* R_world_out, const double* foot_abs_out, const double* foot_vel_body_out) {
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_walk_config";
    if (const char* bad = invalid_plant_step(h, &cfg->plant, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, state_out, R_world_out, foot_abs_out)) return bad;
    if (!foot_vel_body_out) return "null foot_vel_body_out";
    if (!std::isfinite(cfg->swing_track) || cfg->swing_track < 0.0 || cfg->swing_track > 1.0) return "a1mpc_walk_config.swing_track outside 0 .. 1";
    if (cfg->flat_ground && !std::isfinite(cfg->ground_z)) return "a1mpc_walk_config.ground_z must be finite with flat_ground set";
    if (cfg->swing_track > 0.0 && !R_z) return "null R_z with swing_track > 0";
    if (cfg->swing_track > 0.0 && !foot_target) return "null foot_target with swing_track > 0";
    return nullptr;
}
static void launch_walk_step(a1mpc_handle h, const a1mpc_walk_config& cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                             const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z, const double* foot_target,
                             double* state_out, double* R_world_out, double* foot_abs_out, double* foot_vel_body_out, hipStream_t s) {
    WalkArgs w;
    PlantArgs& a = w.p;
    a.n = n; a.stride = state_stride; a.substeps = cfg.plant.substeps; a.dt = cfg.plant.dt; a.gravity = cfg.plant.gravity_z; a.mass = h->cfg.mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = h->cfg.inertia_body[i];
    a.state = state_in; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.state_out = state_out; a.R_out = R_world_out; a.foot_out = foot_abs_out;
    const bool track = cfg.swing_track != 0.0;   // (-0 is no tracking either)
    w.track = track ? cfg.swing_track : 0.0; w.ground_z = cfg.ground_z; w.flat_ground = cfg.flat_ground;
    w.Rz = track ? R_z : nullptr; w.target = track ? foot_target : nullptr; w.vel_out = foot_vel_body_out;
    hipLaunchKernelGGL(a1mpc_walk_step_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, w);
}
a1mpc_status a1mpc_walk_step_batch_device(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                          const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                          const double* d_ext_wrench, const double* d_R_z, const double* d_foot_target, double* d_state_out, double* d_R_world_out,
                                          double* d_foot_abs_out, double* d_foot_vel_body_out, void* hip_stream) {
    if (const char* bad = invalid_walk_step(h, cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_R_z, d_foot_target, d_state_out,
                                            d_R_world_out, d_foot_abs_out, d_foot_vel_body_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_walk_step(h, *cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, d_R_z, d_foot_target, d_state_out,
                                     d_R_world_out, d_foot_abs_out, d_foot_vel_body_out, s));
    return A1MPC_OK;
}
// the host-pointer entry: staged like a1mpc_plant_step_batch (in place on the staged inputs; a wider state_out staged in as well)
a1mpc_status a1mpc_walk_step_batch(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                   const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                   const double* foot_target, double* state_out, double* R_world_out, double* foot_abs_out, double* foot_vel_body_out) {
    if (const char* bad = invalid_walk_step(h, cfg, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, R_z, foot_target, state_out, R_world_out, foot_abs_out,
                                            foot_vel_body_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const size_t W = static_cast<size_t>(state_stride);
    const bool track = cfg->swing_track != 0.0;
    double *d_state = sg.in(state_in, W), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12);
    const double *d_grf = sg.in(grf_body, 12), *d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr;
    const double *d_Rz = track ? sg.in(R_z, 9) : nullptr, *d_tg = track ? sg.in(foot_target, 12) : nullptr;
    const uint8_t* d_ct = sg.in(contacts, 4);
    double* d_out = (W == 12 || state_out == state_in) ? d_state : sg.in(static_cast<const double*>(state_out), W);
    double* d_vel = sg.out(foot_vel_body_out, 12);
    sg.back(state_out, d_out, W); sg.back(R_world_out, d_R, 9); sg.back(foot_abs_out, d_foot, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_walk_step(h, *cfg, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, d_Rz, d_tg, d_out, d_R, d_foot, d_vel, s));
    return sg.finish();
}
static void launch_walk_sensors(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs, const double* grf_body,
                                const uint8_t* contacts, const double* ext_wrench, const double* foot_vel_body, const double* rho_fix, const double* rho_opt,
                                double* quat_out, double* imu_acc_raw_out, double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out, double* foot_force_out,
                                uint8_t* reach_out, double* foot_pos_rel_out, double* foot_vel_rel_out, hipStream_t s) {
    WalkSensorArgs w;
    SynthArgs& a = w.s;
    a.n = n; a.stride = state_stride; a.mass = h->cfg.mass;
    std::memcpy(a.rho_fix, rho_fix, sizeof a.rho_fix); std::memcpy(a.rho_opt, rho_opt, sizeof a.rho_opt);
    a.state = state; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.quat = quat_out; a.acc = imu_acc_raw_out; a.gyro = imu_gyro_raw_out; a.jpos = joint_pos_out; a.jvel = joint_vel_out; a.fforce = foot_force_out;
    a.prel = foot_pos_rel_out; a.vrel = foot_vel_rel_out; a.reach = reach_out;
    w.vel = foot_vel_body;
    hipLaunchKernelGGL(a1mpc_walk_sensors_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, w);
}
a1mpc_status a1mpc_walk_sensors_batch_device(a1mpc_handle h, int32_t n, const double* d_state, int32_t state_stride, const double* d_R_world, const double* d_foot_abs,
                                             const double* d_grf_body, const uint8_t* d_contacts, const double* d_ext_wrench, const double* d_foot_vel_body,
                                             const double* rho_fix, const double* rho_opt, double* d_quat_out, double* d_imu_acc_raw_out, double* d_imu_gyro_raw_out,
                                             double* d_joint_pos_out, double* d_joint_vel_out, double* d_foot_force_out, uint8_t* d_reach_out, double* d_foot_pos_rel_out,
                                             double* d_foot_vel_rel_out, void* hip_stream) {
    if (const char* bad = invalid_sensor_synthesis(h, n, d_state, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, rho_fix, rho_opt, d_quat_out, d_imu_acc_raw_out,
                                                   d_imu_gyro_raw_out, d_joint_pos_out, d_joint_vel_out, d_foot_force_out, d_reach_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_walk_sensors(h, n, d_state, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, d_foot_vel_body, rho_fix, rho_opt, d_quat_out,
                                        d_imu_acc_raw_out, d_imu_gyro_raw_out, d_joint_pos_out, d_joint_vel_out, d_foot_force_out, d_reach_out, d_foot_pos_rel_out,
                                        d_foot_vel_rel_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_walk_sensors_batch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                      const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* foot_vel_body, const double* rho_fix,
                                      const double* rho_opt, double* quat_out, double* imu_acc_raw_out, double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out,
                                      double* foot_force_out, uint8_t* reach_out, double* foot_pos_rel_out, double* foot_vel_rel_out) {
    if (const char* bad = invalid_sensor_synthesis(h, n, state, state_stride, R_world, foot_abs, grf_body, contacts, rho_fix, rho_opt, quat_out, imu_acc_raw_out,
                                                   imu_gyro_raw_out, joint_pos_out, joint_vel_out, foot_force_out, reach_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const double *d_state = sg.in(state, static_cast<size_t>(state_stride)), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12), *d_grf = sg.in(grf_body, 12);
    const double *d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr, *d_vel = foot_vel_body ? sg.in(foot_vel_body, 12) : nullptr;
    const uint8_t* d_ct = sg.in(contacts, 4);
    double *d_quat = sg.out(quat_out, 4), *d_acc = sg.out(imu_acc_raw_out, 3), *d_gyro = sg.out(imu_gyro_raw_out, 3), *d_jp = sg.out(joint_pos_out, 12);
    double *d_jv = sg.out(joint_vel_out, 12), *d_ff = sg.out(foot_force_out, 4), *d_pr = sg.out(foot_pos_rel_out, 12), *d_vr = sg.out(foot_vel_rel_out, 12);
    uint8_t* d_reach = sg.out(reach_out, 4);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_walk_sensors(h, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, d_vel, rho_fix, rho_opt, d_quat, d_acc, d_gyro, d_jp, d_jv, d_ff, d_reach,
                                        d_pr, d_vr, s));
    return sg.finish();
}
// ---- sloped ground and sensed touchdowns behind the C ABI: a1mpc_walk_step_ground_kernel and a1mpc_walk_sensors_touch_kernel, no handle state
// what the two ground-step entries refuse, or null: the walk step's refusals (with `ground` given, cfg's own plane is not read and so not checked), then a null touch_out
static const char* invalid_walk_step_ground(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                            const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* R_z, const double* foot_target,
                                            const double* ground, const double* state_out, const double* R_world_out, const double* foot_abs_out,
                                            const double* foot_vel_body_out, const uint8_t* touch_out) {
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_walk_config";
    a1mpc_walk_config c = *cfg;
    if (ground) { c.flat_ground = 0; c.ground_z = 0.0; }
    if (const char* bad = invalid_walk_step(h, &c, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, R_z, foot_target, state_out, R_world_out, foot_abs_out,
                                            foot_vel_body_out))
        return bad;
    if (!touch_out) return "null touch_out";
    return nullptr;
}
static void launch_walk_step_ground(a1mpc_handle h, const a1mpc_walk_config& cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                    const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                    const double* foot_target, const double* ground, double* state_out, double* R_world_out, double* foot_abs_out,
                                    double* foot_vel_body_out, uint8_t* touch_out, hipStream_t s) {
    WalkGroundArgs g;
    WalkArgs& w = g.w;
    PlantArgs& a = w.p;
    a.n = n; a.stride = state_stride; a.substeps = cfg.plant.substeps; a.dt = cfg.plant.dt; a.gravity = cfg.plant.gravity_z; a.mass = h->cfg.mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = h->cfg.inertia_body[i];
    a.state = state_in; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.state_out = state_out; a.R_out = R_world_out; a.foot_out = foot_abs_out;
    const bool track = cfg.swing_track != 0.0;   // (-0 is no tracking either)
    w.track = track ? cfg.swing_track : 0.0;
    w.ground_z = ground ? 0.0 : cfg.ground_z; w.flat_ground = ground ? 0 : cfg.flat_ground;   // (with `ground` given cfg's plane is not read)
    w.Rz = track ? R_z : nullptr; w.target = track ? foot_target : nullptr; w.vel_out = foot_vel_body_out;
    g.ground = ground; g.touch = touch_out;
    hipLaunchKernelGGL(a1mpc_walk_step_ground_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, g);
}
a1mpc_status a1mpc_ground_step_batch_device(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                                 const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                                 const double* d_ext_wrench, const double* d_R_z, const double* d_foot_target, const double* d_ground,
                                                 double* d_state_out, double* d_R_world_out, double* d_foot_abs_out, double* d_foot_vel_body_out, uint8_t* d_touch_out,
                                                 void* hip_stream) {
    if (const char* bad = invalid_walk_step_ground(h, cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_R_z, d_foot_target, d_ground,
                                                   d_state_out, d_R_world_out, d_foot_abs_out, d_foot_vel_body_out, d_touch_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_walk_step_ground(h, *cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, d_R_z, d_foot_target, d_ground,
                                            d_state_out, d_R_world_out, d_foot_abs_out, d_foot_vel_body_out, d_touch_out, s));
    return A1MPC_OK;
}
// the host-pointer entry: staged like a1mpc_walk_step_batch
a1mpc_status a1mpc_ground_step_batch(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                          const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                          const double* foot_target, const double* ground, double* state_out, double* R_world_out, double* foot_abs_out,
                                          double* foot_vel_body_out, uint8_t* touch_out) {
    if (const char* bad = invalid_walk_step_ground(h, cfg, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, R_z, foot_target, ground, state_out,
                                                   R_world_out, foot_abs_out, foot_vel_body_out, touch_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const size_t W = static_cast<size_t>(state_stride);
    const bool track = cfg->swing_track != 0.0;
    double *d_state = sg.in(state_in, W), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12);
    const double *d_grf = sg.in(grf_body, 12), *d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr;
    const double *d_Rz = track ? sg.in(R_z, 9) : nullptr, *d_tg = track ? sg.in(foot_target, 12) : nullptr, *d_gr = ground ? sg.in(ground, 3) : nullptr;
    const uint8_t* d_ct = sg.in(contacts, 4);
    double* d_out = (W == 12 || state_out == state_in) ? d_state : sg.in(static_cast<const double*>(state_out), W);
    double* d_vel = sg.out(foot_vel_body_out, 12);
    uint8_t* d_touch = sg.out(touch_out, 4);
    sg.back(state_out, d_out, W); sg.back(R_world_out, d_R, 9); sg.back(foot_abs_out, d_foot, 12);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_walk_step_ground(h, *cfg, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, d_Rz, d_tg, d_gr, d_out, d_R, d_foot, d_vel, d_touch, s));
    return sg.finish();
}
static const char* invalid_touch_force(double touch_force) {
    return std::isfinite(touch_force) && touch_force >= 0.0 ? nullptr : "touch_force must be finite and not negative";
}
static void launch_walk_sensors_touch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                      const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* foot_vel_body, const uint8_t* touch,
                                      double touch_force, const double* rho_fix, const double* rho_opt, double* quat_out, double* imu_acc_raw_out, double* imu_gyro_raw_out,
                                      double* joint_pos_out, double* joint_vel_out, double* foot_force_out, uint8_t* reach_out, double* foot_pos_rel_out,
                                      double* foot_vel_rel_out, hipStream_t s) {
    WalkTouchArgs t;
    SynthArgs& a = t.w.s;
    a.n = n; a.stride = state_stride; a.mass = h->cfg.mass;
    std::memcpy(a.rho_fix, rho_fix, sizeof a.rho_fix); std::memcpy(a.rho_opt, rho_opt, sizeof a.rho_opt);
    a.state = state; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.quat = quat_out; a.acc = imu_acc_raw_out; a.gyro = imu_gyro_raw_out; a.jpos = joint_pos_out; a.jvel = joint_vel_out; a.fforce = foot_force_out;
    a.prel = foot_pos_rel_out; a.vrel = foot_vel_rel_out; a.reach = reach_out;
    t.w.vel = foot_vel_body; t.touch = touch; t.touch_force = touch_force == 0.0 ? 0.0 : touch_force;   // (-0 reports +0, the walk sensors' bits)
    hipLaunchKernelGGL(a1mpc_walk_sensors_touch_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, t);
}
a1mpc_status a1mpc_touch_sensors_batch_device(a1mpc_handle h, int32_t n, const double* d_state, int32_t state_stride, const double* d_R_world, const double* d_foot_abs,
                                                   const double* d_grf_body, const uint8_t* d_contacts, const double* d_ext_wrench, const double* d_foot_vel_body,
                                                   const uint8_t* d_touch, double touch_force, const double* rho_fix, const double* rho_opt, double* d_quat_out,
                                                   double* d_imu_acc_raw_out, double* d_imu_gyro_raw_out, double* d_joint_pos_out, double* d_joint_vel_out,
                                                   double* d_foot_force_out, uint8_t* d_reach_out, double* d_foot_pos_rel_out, double* d_foot_vel_rel_out, void* hip_stream) {
    const char* bad = invalid_sensor_synthesis(h, n, d_state, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, rho_fix, rho_opt, d_quat_out, d_imu_acc_raw_out,
                                               d_imu_gyro_raw_out, d_joint_pos_out, d_joint_vel_out, d_foot_force_out, d_reach_out);
    if (!bad) bad = invalid_touch_force(touch_force);
    if (bad) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_walk_sensors_touch(h, n, d_state, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, d_foot_vel_body, d_touch, touch_force,
                                              rho_fix, rho_opt, d_quat_out, d_imu_acc_raw_out, d_imu_gyro_raw_out, d_joint_pos_out, d_joint_vel_out, d_foot_force_out,
                                              d_reach_out, d_foot_pos_rel_out, d_foot_vel_rel_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_touch_sensors_batch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                            const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* foot_vel_body, const uint8_t* touch,
                                            double touch_force, const double* rho_fix, const double* rho_opt, double* quat_out, double* imu_acc_raw_out,
                                            double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out, double* foot_force_out, uint8_t* reach_out,
                                            double* foot_pos_rel_out, double* foot_vel_rel_out) {
    const char* bad = invalid_sensor_synthesis(h, n, state, state_stride, R_world, foot_abs, grf_body, contacts, rho_fix, rho_opt, quat_out, imu_acc_raw_out,
                                               imu_gyro_raw_out, joint_pos_out, joint_vel_out, foot_force_out, reach_out);
    if (!bad) bad = invalid_touch_force(touch_force);
    if (bad) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const double *d_state = sg.in(state, static_cast<size_t>(state_stride)), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12), *d_grf = sg.in(grf_body, 12);
    const double *d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr, *d_vel = foot_vel_body ? sg.in(foot_vel_body, 12) : nullptr;
    const uint8_t *d_ct = sg.in(contacts, 4), *d_touch = touch ? sg.in(touch, 4) : nullptr;
    double *d_quat = sg.out(quat_out, 4), *d_acc = sg.out(imu_acc_raw_out, 3), *d_gyro = sg.out(imu_gyro_raw_out, 3), *d_jp = sg.out(joint_pos_out, 12);
    double *d_jv = sg.out(joint_vel_out, 12), *d_ff = sg.out(foot_force_out, 4), *d_pr = sg.out(foot_pos_rel_out, 12), *d_vr = sg.out(foot_vel_rel_out, 12);
    uint8_t* d_reach = sg.out(reach_out, 4);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_walk_sensors_touch(h, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, d_vel, d_touch, touch_force, rho_fix, rho_opt, d_quat, d_acc,
                                              d_gyro, d_jp, d_jv, d_ff, d_reach, d_pr, d_vr, s));
    return sg.finish();
}
// ---- height-field terrain behind the C ABI: a1mpc_walk_step_heightfield_kernel and a1mpc_heightfield_sample_kernel, no handle state
void a1mpc_default_heightfield(a1mpc_heightfield* f) {
    if (!f) return;
    std::memset(f, 0, sizeof *f);
    f->nx = 0; f->ny = 0; f->x0 = 0.0; f->y0 = 0.0; f->dx = 1.0; f->dy = 1.0; f->interp = 0; f->height = nullptr;
}
constexpr int32_t kHfMaxNodesPerAxis = 32768;
constexpr int64_t kHfMaxStagedNodes = int64_t{1} << 20;   // what a host-pointer entry stages per call
// what every heightfield entry refuses of its field, or null.  Checked FIRST, in front of the handle, so that a bad field is reported whether or not a GPU is present
static const char* invalid_heightfield(const a1mpc_heightfield* f) {
    if (!f) return "null a1mpc_heightfield";
    if (f->interp != 0 && f->interp != 1) return "a1mpc_heightfield.interp must be 0 or 1";
    const int32_t least = f->interp ? 2 : 1;
    if (f->nx < least) return "a1mpc_heightfield.nx below 1 (interp 0) or 2 (interp 1)";
    if (f->ny < least) return "a1mpc_heightfield.ny below 1 (interp 0) or 2 (interp 1)";
    if (f->nx > kHfMaxNodesPerAxis) return "a1mpc_heightfield.nx above 32768";
    if (f->ny > kHfMaxNodesPerAxis) return "a1mpc_heightfield.ny above 32768";
    if (!std::isfinite(f->dx) || !(f->dx > 0.0)) return "a1mpc_heightfield.dx must be positive and finite";
    if (!std::isfinite(f->dy) || !(f->dy > 0.0)) return "a1mpc_heightfield.dy must be positive and finite";
    if (!std::isfinite(f->x0)) return "a1mpc_heightfield.x0 must be finite";
    if (!std::isfinite(f->y0)) return "a1mpc_heightfield.y0 must be finite";
    if (!std::isfinite(1.0 / f->dx)) return "a1mpc_heightfield.dx: 1 / dx is not finite";
    if (!std::isfinite(1.0 / f->dy)) return "a1mpc_heightfield.dy: 1 / dy is not finite";
    if (!f->height) return "null a1mpc_heightfield.height";
    return nullptr;
}
static HfField make_hf_field(const a1mpc_heightfield& f, const double* d_height) {
    HfField k;
    k.H = d_height; k.x0 = f.x0; k.y0 = f.y0; k.inv_dx = 1.0 / f.dx; k.inv_dy = 1.0 / f.dy; k.nx = f.nx; k.ny = f.ny; k.interp = f.interp;
    return k;
}
// a host-pointer entry's copy of the field on the device: allocated, filled on `s` and freed within the call (the handle gets no state; these entries are for tests and
// small fields).  The free waits for the device, so it is safe behind a launch that failed half way as well
extern "C++" {
struct HfStaged {
    double* d = nullptr;
    ~HfStaged() { if (d) (void)hipFree(d); }
    a1mpc_status fill(const a1mpc_heightfield& f, hipStream_t s) {
        const size_t bytes = static_cast<size_t>(f.nx) * static_cast<size_t>(f.ny) * sizeof(double);
        A1_HIP(hipMalloc(&d, bytes));
        A1_HIP(hipMemcpyAsync(d, f.height, bytes, hipMemcpyHostToDevice, s));
        return A1MPC_OK;
    }
};
}  // extern "C++"
static const char* too_large_to_stage(const a1mpc_heightfield& f) {
    return static_cast<int64_t>(f.nx) * f.ny > kHfMaxStagedNodes ? "a1mpc_heightfield of more than 2^20 nodes given to a host-pointer entry: use the _device entry" : nullptr;
}
// what the two step entries refuse, or null: the field's refusals, then the ground step's (cfg's own plane is not read and so not checked)
static const char* invalid_heightfield_step(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                            const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* R_z, const double* foot_target,
                                            const a1mpc_heightfield* field, const double* state_out, const double* R_world_out, const double* foot_abs_out,
                                            const double* foot_vel_body_out, const uint8_t* touch_out) {
    if (const char* bad = invalid_heightfield(field)) return bad;
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_walk_config";
    a1mpc_walk_config c = *cfg;
    c.flat_ground = 0; c.ground_z = 0.0;
    if (const char* bad = invalid_walk_step(h, &c, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, R_z, foot_target, state_out, R_world_out, foot_abs_out,
                                            foot_vel_body_out))
        return bad;
    if (!touch_out) return "null touch_out";
    return nullptr;
}
static void launch_heightfield_step(a1mpc_handle h, const a1mpc_walk_config& cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                    const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                    const double* foot_target, const HfField& field, const double* origin, double* state_out, double* R_world_out, double* foot_abs_out,
                                    double* foot_vel_body_out, uint8_t* touch_out, double* ground_out, hipStream_t s) {
    WalkHeightfieldArgs g;
    WalkArgs& w = g.w;
    PlantArgs& a = w.p;
    a.n = n; a.stride = state_stride; a.substeps = cfg.plant.substeps; a.dt = cfg.plant.dt; a.gravity = cfg.plant.gravity_z; a.mass = h->cfg.mass;
    for (int i = 0; i < 9; ++i) a.inertia[i] = h->cfg.inertia_body[i];
    a.state = state_in; a.R = R_world; a.foot = foot_abs; a.grf = grf_body; a.ext = ext_wrench; a.contacts = contacts;
    a.state_out = state_out; a.R_out = R_world_out; a.foot_out = foot_abs_out;
    const bool track = cfg.swing_track != 0.0;   // (-0 is no tracking either)
    w.track = track ? cfg.swing_track : 0.0; w.ground_z = 0.0; w.flat_ground = 0;   // (cfg's plane is not read)
    w.Rz = track ? R_z : nullptr; w.target = track ? foot_target : nullptr; w.vel_out = foot_vel_body_out;
    g.f = field; g.origin = origin; g.touch = touch_out; g.ground_out = ground_out;
    hipLaunchKernelGGL(a1mpc_walk_step_heightfield_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, g);
}
a1mpc_status a1mpc_heightfield_step_batch_device(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                                 const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                                 const double* d_ext_wrench, const double* d_R_z, const double* d_foot_target, const a1mpc_heightfield* field,
                                                 const double* d_origin, double* d_state_out, double* d_R_world_out, double* d_foot_abs_out, double* d_foot_vel_body_out,
                                                 uint8_t* d_touch_out, double* d_ground_out, void* hip_stream) {
    if (const char* bad = invalid_heightfield_step(h, cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_R_z, d_foot_target, field,
                                                   d_state_out, d_R_world_out, d_foot_abs_out, d_foot_vel_body_out, d_touch_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_heightfield_step(h, *cfg, n, d_state_in, state_stride, d_R_world, d_foot_abs, d_grf_body, d_contacts, d_ext_wrench, d_R_z, d_foot_target,
                                            make_hf_field(*field, field->height), d_origin, d_state_out, d_R_world_out, d_foot_abs_out, d_foot_vel_body_out, d_touch_out,
                                            d_ground_out, s));
    return A1MPC_OK;
}
// the host-pointer entry: staged like a1mpc_ground_step_batch, and the whole field with it
a1mpc_status a1mpc_heightfield_step_batch(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                          const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                          const double* foot_target, const a1mpc_heightfield* field, const double* origin, double* state_out, double* R_world_out,
                                          double* foot_abs_out, double* foot_vel_body_out, uint8_t* touch_out, double* ground_out) {
    if (const char* bad = invalid_heightfield_step(h, cfg, n, state_in, state_stride, R_world, foot_abs, grf_body, contacts, R_z, foot_target, field, state_out,
                                                   R_world_out, foot_abs_out, foot_vel_body_out, touch_out))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (const char* big = too_large_to_stage(*field)) return fail(A1MPC_ERR_BATCH_TOO_LARGE, big);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    HfStaged hf;
    const size_t W = static_cast<size_t>(state_stride);
    const bool track = cfg->swing_track != 0.0;
    double *d_state = sg.in(state_in, W), *d_R = sg.in(R_world, 9), *d_foot = sg.in(foot_abs, 12);
    const double *d_grf = sg.in(grf_body, 12), *d_ext = ext_wrench ? sg.in(ext_wrench, 6) : nullptr;
    const double *d_Rz = track ? sg.in(R_z, 9) : nullptr, *d_tg = track ? sg.in(foot_target, 12) : nullptr, *d_or = origin ? sg.in(origin, 3) : nullptr;
    const uint8_t* d_ct = sg.in(contacts, 4);
    double* d_out = (W == 12 || state_out == state_in) ? d_state : sg.in(static_cast<const double*>(state_out), W);
    double *d_vel = sg.out(foot_vel_body_out, 12), *d_go = sg.out(ground_out, 3);
    uint8_t* d_touch = sg.out(touch_out, 4);
    sg.back(state_out, d_out, W); sg.back(R_world_out, d_R, 9); sg.back(foot_abs_out, d_foot, 12);
    A1_STAGED(sg);
    if (a1mpc_status st = hf.fill(*field, s); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(launch_heightfield_step(h, *cfg, n, d_state, state_stride, d_R, d_foot, d_grf, d_ct, d_ext, d_Rz, d_tg, make_hf_field(*field, hf.d), d_or, d_out, d_R,
                                            d_foot, d_vel, d_touch, d_go, s));
    return sg.finish();
}
static const char* invalid_heightfield_sample(a1mpc_handle h, const a1mpc_heightfield* field, int32_t n, const double* xy, const double* height_out) {
    if (const char* bad = invalid_heightfield(field)) return bad;
    if (!h) return "null handle";
    if (n < 0) return "negative n";
    if (!xy) return "null xy";
    if (!height_out) return "null height_out";
    return nullptr;
}
static void launch_heightfield_sample(int32_t n, const HfField& field, const double* xy, const double* origin, double* height_out, hipStream_t s) {
    HfSampleArgs a;
    a.f = field; a.n = n; a.xy = xy; a.origin = origin; a.out = height_out;
    hipLaunchKernelGGL(a1mpc_heightfield_sample_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 63) / 64)), dim3(64), 0, s, a);
}
a1mpc_status a1mpc_heightfield_sample_batch_device(a1mpc_handle h, const a1mpc_heightfield* field, int32_t n, const double* d_xy, const double* d_origin,
                                                   double* d_height_out, void* hip_stream) {
    if (const char* bad = invalid_heightfield_sample(h, field, n, d_xy, d_height_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_heightfield_sample(n, make_hf_field(*field, field->height), d_xy, d_origin, d_height_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_heightfield_sample_batch(a1mpc_handle h, const a1mpc_heightfield* field, int32_t n, const double* xy, const double* origin, double* height_out) {
    if (const char* bad = invalid_heightfield_sample(h, field, n, xy, height_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (const char* big = too_large_to_stage(*field)) return fail(A1MPC_ERR_BATCH_TOO_LARGE, big);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    HfStaged hf;
    const double *d_xy = sg.in(xy, 2), *d_or = origin ? sg.in(origin, 3) : nullptr;
    double* d_out = sg.out(height_out, 1);
    A1_STAGED(sg);
    if (a1mpc_status st = hf.fill(*field, s); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(launch_heightfield_sample(n, make_hf_field(*field, hf.d), d_xy, d_or, d_out, s));
    return sg.finish();
}
// ---- sensor noise and IMU bias behind the C ABI: a1mpc_sensor_noise_kernel, no handle state
void a1mpc_default_noise_config(a1mpc_noise_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);   // seed 0 and every sigma +0: off
}
// what the two entries refuse, or null (all before the first HIP call).  arr: quat, imu_acc_raw, imu_gyro_raw, joint_pos, joint_vel, foot_force, imu_bias, z_out
constexpr size_t kNoiseWidths[8] = {4, 3, 3, 12, 12, 4, 6, kNoiseZ};
static const char* invalid_sensor_noise(a1mpc_handle h, const a1mpc_noise_config* cfg, int32_t n, uint64_t robot0, const double* const* arr) {
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_noise_config";
    if (n < 0) return "negative n";
    const struct { double v; const char* what; } levels[8] = {
        {cfg->gyro_sigma, "a1mpc_noise_config.gyro_sigma must be finite and not negative"}, {cfg->acc_sigma, "a1mpc_noise_config.acc_sigma must be finite and not negative"},
        {cfg->gyro_bias_walk, "a1mpc_noise_config.gyro_bias_walk must be finite and not negative"},
        {cfg->acc_bias_walk, "a1mpc_noise_config.acc_bias_walk must be finite and not negative"}, {cfg->att_sigma, "a1mpc_noise_config.att_sigma must be finite and not negative"},
        {cfg->joint_pos_sigma, "a1mpc_noise_config.joint_pos_sigma must be finite and not negative"},
        {cfg->joint_vel_sigma, "a1mpc_noise_config.joint_vel_sigma must be finite and not negative"},
        {cfg->foot_force_sigma, "a1mpc_noise_config.foot_force_sigma must be finite and not negative"}};
    for (const auto& lv : levels)
        if (!std::isfinite(lv.v) || lv.v < 0.0) return lv.what;
    if ((cfg->gyro_bias_walk > 0.0 || cfg->acc_bias_walk > 0.0) && !arr[6]) return "null imu_bias with a bias walk > 0";
    if (robot0 > (uint64_t{1} << 32) - static_cast<uint64_t>(n)) return "robot0 + n beyond 2^32";
    for (int i = 0; i < 8; ++i)
        for (int k = i + 1; k < 8; ++k) {
            if (!arr[i] || !arr[k]) continue;
            const uintptr_t pi = reinterpret_cast<uintptr_t>(arr[i]), pk = reinterpret_cast<uintptr_t>(arr[k]);
            const uintptr_t bi = static_cast<uintptr_t>(n) * kNoiseWidths[i] * sizeof(double), bk = static_cast<uintptr_t>(n) * kNoiseWidths[k] * sizeof(double);
            if (pi < pk + bk && pk < pi + bi) return "two of the arrays overlap";
        }
    return nullptr;
}
static void launch_sensor_noise(const a1mpc_noise_config& cfg, int32_t n, uint64_t robot0, uint64_t tick, double* quat, double* imu_acc_raw, double* imu_gyro_raw,
                                double* joint_pos, double* joint_vel, double* foot_force, double* imu_bias, double* z_out, hipStream_t s) {
    NoiseArgs a;
    a.n = n; a.key0 = static_cast<uint32_t>(cfg.seed); a.key1 = static_cast<uint32_t>(cfg.seed >> 32);
    a.tick_lo = static_cast<uint32_t>(tick); a.tick_hi = static_cast<uint32_t>(tick >> 32); a.robot0 = robot0;
    a.gyro_sigma = imu_gyro_raw ? cfg.gyro_sigma : 0.0; a.acc_sigma = imu_acc_raw ? cfg.acc_sigma : 0.0;
    a.gyro_walk = imu_bias ? cfg.gyro_bias_walk : 0.0; a.acc_walk = imu_bias ? cfg.acc_bias_walk : 0.0;
    a.att_sigma = quat ? cfg.att_sigma : 0.0; a.jpos_sigma = joint_pos ? cfg.joint_pos_sigma : 0.0; a.jvel_sigma = joint_vel ? cfg.joint_vel_sigma : 0.0;
    a.fforce_sigma = foot_force ? cfg.foot_force_sigma : 0.0;
    a.quat = quat; a.acc = imu_acc_raw; a.gyro = imu_gyro_raw; a.jpos = joint_pos; a.jvel = joint_vel; a.fforce = foot_force; a.bias = imu_bias; a.z = z_out;
    // the draws somebody reads: all of them with z_out, else those of the channels that are on (z[2 j], z[2 j + 1] are draw j's)
    uint64_t zs = 0;
    const auto on = [&zs](double level, int z0, int count) { if (level != 0.0) zs |= ((uint64_t{1} << count) - 1) << z0; };
    on(a.gyro_sigma, 0, 3); on(a.acc_sigma, 3, 3); on(a.gyro_walk, 6, 3); on(a.acc_walk, 9, 3); on(a.att_sigma, 12, 3); on(a.jpos_sigma, 16, 12); on(a.jvel_sigma, 28, 12);
    on(a.fforce_sigma, 40, 4);
    a.draws = 0;
    for (int j = 0; j < kNoiseDraws; ++j)
        if (z_out || ((zs >> (2 * j)) & 3u)) a.draws |= 1u << j;
    hipLaunchKernelGGL(a1mpc_sensor_noise_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, a);
}
a1mpc_status a1mpc_sensor_noise_batch_device(a1mpc_handle h, const a1mpc_noise_config* cfg, int32_t n, uint64_t robot0, uint64_t tick, double* d_quat,
                                             double* d_imu_acc_raw, double* d_imu_gyro_raw, double* d_joint_pos, double* d_joint_vel, double* d_foot_force,
                                             double* d_imu_bias, double* d_z_out, void* hip_stream) {
    const double* const arr[8] = {d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_joint_pos, d_joint_vel, d_foot_force, d_imu_bias, d_z_out};
    if (const char* bad = invalid_sensor_noise(h, cfg, n, robot0, arr)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_sensor_noise(*cfg, n, robot0, tick, d_quat, d_imu_acc_raw, d_imu_gyro_raw, d_joint_pos, d_joint_vel, d_foot_force, d_imu_bias, d_z_out, s));
    return A1MPC_OK;
}
// the host-pointer entry: every array the caller gives is staged in and back (in place on the staged copy), z_out back alone
a1mpc_status a1mpc_sensor_noise_batch(a1mpc_handle h, const a1mpc_noise_config* cfg, int32_t n, uint64_t robot0, uint64_t tick, double* quat, double* imu_acc_raw,
                                      double* imu_gyro_raw, double* joint_pos, double* joint_vel, double* foot_force, double* imu_bias, double* z_out) {
    const double* const arr[8] = {quat, imu_acc_raw, imu_gyro_raw, joint_pos, joint_vel, foot_force, imu_bias, z_out};
    if (const char* bad = invalid_sensor_noise(h, cfg, n, robot0, arr)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const auto io = [&sg](double* host, size_t w) { return host ? sg.inout(host, w) : nullptr; };
    double *d_quat = io(quat, 4), *d_acc = io(imu_acc_raw, 3), *d_gyro = io(imu_gyro_raw, 3), *d_jp = io(joint_pos, 12), *d_jv = io(joint_vel, 12), *d_ff = io(foot_force, 4);
    double *d_bias = io(imu_bias, 6), *d_z = sg.out(z_out, kNoiseZ);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_sensor_noise(*cfg, n, robot0, tick, d_quat, d_acc, d_gyro, d_jp, d_jv, d_ff, d_bias, d_z, s));
    return sg.finish();
}
// ---- episode record and batch summary behind the C ABI: a1mpc_episode_update_kernel and a1mpc_episode_reduce_kernel; the records are the caller's, the handle holds the
// summary's partials alone
void a1mpc_default_episode_config(a1mpc_episode_config* c) {
    if (!c) return;
    c->min_up = 0.5; c->min_height = 0.12;
}
constexpr uint64_t kEpisodeTickEnd = (uint64_t{1} << 53) - 1;   // tick + 1 stays an exact double below it
struct EpisodeIn {   // the inputs of an update beside state and R_world, in the entries' order
    const double *root_pos, *root_lin_vel, *root_lin_vel_d, *root_pos_d_z, *ground, *grf_body;
    const uint8_t* contacts;
    const int32_t* status;
    const uint8_t* reach;
};
// what the two update entries refuse, or null (all before the first HIP call; n > max_batch is A1_STAGE_DEVICE's)
static const char* invalid_episode_update(a1mpc_handle h, const a1mpc_episode_config* cfg, int32_t n, uint64_t tick, const double* state, int32_t stride, const double* R_world,
                                          const EpisodeIn& in, const double* episode) {
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_episode_config";
    if (!state || !R_world) return "null state or R_world";
    if (!episode) return "null episode";
    if (stride != 12 && stride != 13 && stride != 22) return "state_stride must be 12, 13 or 22";
    if (n < 0) return "negative n";
    if (!std::isfinite(cfg->min_up) || cfg->min_up < -1.0 || cfg->min_up > 1.0) return "a1mpc_episode_config.min_up must be in [-1, 1]";
    if (!std::isfinite(cfg->min_height)) return "a1mpc_episode_config.min_height must be finite";
    if (tick >= kEpisodeTickEnd) return "tick must be below 2^53 - 1";
    if ((in.root_pos == nullptr) != (in.root_lin_vel == nullptr)) return "root_pos and root_lin_vel are given together or not at all";
    if ((in.grf_body == nullptr) != (in.contacts == nullptr)) return "grf_body and contacts are given together or not at all";
    const struct { const void* p; size_t bytes; } ins[11] = {
        {state, static_cast<size_t>(stride) * sizeof(double)}, {R_world, 9 * sizeof(double)}, {in.root_pos, 3 * sizeof(double)}, {in.root_lin_vel, 3 * sizeof(double)},
        {in.root_lin_vel_d, 3 * sizeof(double)}, {in.root_pos_d_z, sizeof(double)}, {in.ground, 3 * sizeof(double)}, {in.grf_body, 12 * sizeof(double)}, {in.contacts, 4},
        {in.status, sizeof(int32_t)}, {in.reach, 4}};
    const uintptr_t pe = reinterpret_cast<uintptr_t>(episode), be = static_cast<uintptr_t>(n) * kEpWords * sizeof(double);
    for (const auto& x : ins) {
        if (!x.p) continue;
        const uintptr_t pi = reinterpret_cast<uintptr_t>(x.p), bi = static_cast<uintptr_t>(n) * x.bytes;
        if (pi < pe + be && pe < pi + bi) return "episode overlaps an input";
    }
    return nullptr;
}
static void launch_episode_update(const a1mpc_episode_config& cfg, int32_t n, uint64_t tick, const double* state, int32_t stride, const double* R_world, const EpisodeIn& in,
                                  double* episode, hipStream_t s) {
    EpisodeArgs a;
    a.n = n; a.stride = stride; a.min_up = cfg.min_up; a.min_height = cfg.min_height; a.tick_p1 = static_cast<double>(tick + 1);
    a.state = state; a.R = R_world; a.est_pos = in.root_pos; a.est_vel = in.root_lin_vel; a.cmd = in.root_lin_vel_d; a.pos_d_z = in.root_pos_d_z; a.ground = in.ground;
    a.grf = in.grf_body; a.contacts = in.contacts; a.reach = in.reach; a.status = in.status; a.episode = episode;
    hipLaunchKernelGGL(a1mpc_episode_update_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 15) / 16)), dim3(64), 0, s, a);
}
a1mpc_status a1mpc_episode_update_batch_device(a1mpc_handle h, const a1mpc_episode_config* cfg, int32_t n, uint64_t tick, const double* d_state, int32_t state_stride,
                                               const double* d_R_world, const double* d_root_pos, const double* d_root_lin_vel, const double* d_root_lin_vel_d,
                                               const double* d_root_pos_d_z, const double* d_ground, const double* d_grf_body, const uint8_t* d_contacts,
                                               const int32_t* d_status, const uint8_t* d_reach, double* d_episode, void* hip_stream) {
    const EpisodeIn in{d_root_pos, d_root_lin_vel, d_root_lin_vel_d, d_root_pos_d_z, d_ground, d_grf_body, d_contacts, d_status, d_reach};
    if (const char* bad = invalid_episode_update(h, cfg, n, tick, d_state, state_stride, d_R_world, in, d_episode)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    A1_STAGE_LAUNCH(launch_episode_update(*cfg, n, tick, d_state, state_stride, d_R_world, in, d_episode, s));
    return A1MPC_OK;
}
// the host-pointer entry: the inputs given are staged in, the records in and back (status: four bytes per robot of the byte staging, whose slices start 8-byte aligned)
a1mpc_status a1mpc_episode_update_batch(a1mpc_handle h, const a1mpc_episode_config* cfg, int32_t n, uint64_t tick, const double* state, int32_t state_stride,
                                        const double* R_world, const double* root_pos, const double* root_lin_vel, const double* root_lin_vel_d, const double* root_pos_d_z,
                                        const double* ground, const double* grf_body, const uint8_t* contacts, const int32_t* status, const uint8_t* reach, double* episode) {
    const EpisodeIn in{root_pos, root_lin_vel, root_lin_vel_d, root_pos_d_z, ground, grf_body, contacts, status, reach};
    if (const char* bad = invalid_episode_update(h, cfg, n, tick, state, state_stride, R_world, in, episode)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const auto opt = [&sg](const double* host, size_t w) -> const double* { return host ? sg.in(host, w) : nullptr; };
    const auto opt8 = [&sg](const uint8_t* host, size_t w) -> const uint8_t* { return host ? sg.in(host, w) : nullptr; };
    const double *d_state = sg.in(state, static_cast<size_t>(state_stride)), *d_R = sg.in(R_world, 9);
    EpisodeIn d;
    d.root_pos = opt(root_pos, 3); d.root_lin_vel = opt(root_lin_vel, 3); d.root_lin_vel_d = opt(root_lin_vel_d, 3); d.root_pos_d_z = opt(root_pos_d_z, 1);
    d.ground = opt(ground, 3); d.grf_body = opt(grf_body, 12); d.contacts = opt8(contacts, 4); d.reach = opt8(reach, 4);
    d.status = reinterpret_cast<const int32_t*>(opt8(reinterpret_cast<const uint8_t*>(status), sizeof(int32_t)));
    double* d_episode = sg.inout(episode, kEpWords);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_episode_update(*cfg, n, tick, d_state, state_stride, d_R, d, d_episode, s));
    return sg.finish();
}
static const char* invalid_episode_summary(a1mpc_handle h, int32_t n, const double* episode, const double* summary_out) {
    if (!h) return "null handle";
    if (!episode) return "null episode";
    if (!summary_out) return "null summary_out";
    if (n < 0) return "negative n";
    const uintptr_t pe = reinterpret_cast<uintptr_t>(episode), be = static_cast<uintptr_t>(n) * kEpWords * sizeof(double), po = reinterpret_cast<uintptr_t>(summary_out);
    if (po < pe + be && pe < po + kEpSummary * sizeof(double)) return "summary_out overlaps episode";
    return nullptr;
}
static a1mpc_status ensure_episode_ws(a1mpc_handle h) {   // (a1mpc_create's allocation failed: once more, and this time the failure is the call's)
    if (!h->d_episode_ws) A1_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_episode_ws), episode_ws_doubles(h->max_batch) * sizeof(double)));
    return A1MPC_OK;
}
// the levels of the tree, 64 rows per workgroup: n records -> ceil(n / 64) partials -> ... -> the summary; 1, 2 or 3 launches up to 64, 4096, 262 144 rows
static void launch_episode_summary(a1mpc_handle h, int32_t n, const double* episode, double* summary_out, hipStream_t s) {
    EpisodeReduceArgs a;
    a.in = episode; a.rows = n; a.records = 1;
    double* ws = h->d_episode_ws + kEpSummary;
    for (;;) {
        const int64_t groups = (a.rows + 63) / 64;
        a.last = groups == 1; a.out = a.last ? summary_out : ws;
        hipLaunchKernelGGL(a1mpc_episode_reduce_kernel, dim3(static_cast<unsigned>(groups)), dim3(64), 0, s, a);
        if (a.last) return;
        a.in = ws; a.rows = groups; a.records = 0; ws += groups * kEpSummary;
    }
}
a1mpc_status a1mpc_episode_summary_batch_device(a1mpc_handle h, int32_t n, const double* d_episode, double* d_summary_out, void* hip_stream) {
    if (const char* bad = invalid_episode_summary(h, n, d_episode, d_summary_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    if (a1mpc_status st = ensure_episode_ws(h); st != A1MPC_OK) return st;
    A1_STAGE_LAUNCH(launch_episode_summary(h, n, d_episode, d_summary_out, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_episode_summary_batch(a1mpc_handle h, int32_t n, const double* episode, double* summary_out) {
    if (const char* bad = invalid_episode_summary(h, n, episode, summary_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    if (a1mpc_status st = ensure_episode_ws(h); st != A1MPC_OK) return st;
    Staging sg(h, n, s);
    const double* d_episode = sg.in(episode, kEpWords);
    A1_STAGED(sg);
    A1_STAGE_LAUNCH(launch_episode_summary(h, n, d_episode, h->d_episode_ws, s));
    A1_HIP(hipMemcpyAsync(summary_out, h->d_episode_ws, kEpSummary * sizeof(double), hipMemcpyDeviceToHost, s));
    return sg.finish();
}

// ---- respawn behind the C ABI: a1mpc_respawn_kernel and a1mpc_respawn_rows_kernel.  The launcher turns the handle's state blocks into the kernel's table of regions: the
// bytes of robot b that the whole-handle reset of each A1MPC_RESPAWN_* bit zeroes, and no others; a block that is not allocated yet gives no region
void a1mpc_default_respawn_config(a1mpc_respawn_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->codes = 0xEu; c->max_ticks = 0; c->hold_ticks = 10; c->what = A1MPC_RESPAWN_EKF | A1MPC_RESPAWN_CONTACT | A1MPC_RESPAWN_SENSOR | A1MPC_RESPAWN_WARM;
}
static int respawn_regions(a1mpc_handle h, uint32_t what, RespawnRegion* g) {
    const int64_t N = h->max_batch, D = sizeof(double);
    int k = 0;
    auto block = [&](void* base, int64_t bytes) { g[k++] = RespawnRegion{static_cast<char*>(base), bytes, 0, static_cast<int32_t>(bytes), 1}; };
    auto slots = [&](void* base, int64_t word, int32_t runs) { g[k++] = RespawnRegion{static_cast<char*>(base), word, word * N, static_cast<int32_t>(word), runs}; };
    if ((what & A1MPC_RESPAWN_EKF) && h->d_ekf_state) block(h->d_ekf_state, kEkfState * D);
    if ((what & A1MPC_RESPAWN_CONTACT) && h->d_ct_state) {   // (make_contact_args: records, leg rings, terrain rings)
        char* const rec = reinterpret_cast<char*>(h->d_ct_state);
        char* const leg = rec + N * static_cast<int64_t>(sizeof(CtRecord));
        block(rec, sizeof(CtRecord));
        block(leg, kCtLegRing * D);
        slots(leg + N * static_cast<int64_t>(kCtLegRing) * D, D, kTerrainWindow);
    }
    if ((what & A1MPC_RESPAWN_SENSOR) && h->d_sensor_filt && h->d_sensor_cursor) {   // (every slot the allocation holds, as a1mpc_reset_sensor_state)
        slots(h->d_sensor_filt, D, kImuFilters * (h->sensor_alloc_window + 2));
        slots(h->d_sensor_cursor, sizeof(int32_t), 2);
    }
    if (what & A1MPC_RESPAWN_WARM) {
        const int64_t H = h->cfg.horizon;
        block(h->d_wx, 12 * H * D); block(h->d_wy, 20 * H * D); block(h->d_rho, D);
        if (h->d_carry) block(h->d_carry, static_cast<int64_t>(carry_stride(h->cfg.horizon)) * D);
    }
    static_assert(kRespawnRegions >= 10, "one region per block above");
    return k;
}
static bool respawn_overlap(const void* p, size_t bp, const void* q, size_t bq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + bq && b < a + bp;
}
static const char* invalid_respawn_reset(a1mpc_handle h, int32_t n, const uint8_t* mask, uint32_t what) {
    if (!h) return "null handle";
    if (!mask) return "null mask";
    if (n < 0) return "negative n";
    if (what & ~0xFu) return "what has bits that are no A1MPC_RESPAWN_* block";
    return nullptr;
}
static const char* invalid_respawn(a1mpc_handle h, const a1mpc_respawn_config* cfg, int32_t n, const double* episode, const int32_t* life, const double* finished_out,
                                   const uint8_t* mask_out) {
    if (!h) return "null handle";
    if (!cfg) return "null a1mpc_respawn_config";
    if (!episode) return "null episode";
    if (!life) return "null life";
    if (!mask_out) return "null mask_out";
    if (n < 0) return "negative n";
    if (cfg->what & ~0xFu) return "a1mpc_respawn_config.what has bits that are no A1MPC_RESPAWN_* block";
    if (cfg->codes & ~0xEu) return "a1mpc_respawn_config.codes has bits that are no end code (1 .. 3)";
    if (cfg->hold_ticks < 0) return "a1mpc_respawn_config.hold_ticks must not be negative";
    if (cfg->max_ticks >= (1ull << 53)) return "a1mpc_respawn_config.max_ticks must be below 2^53";
    const size_t N = static_cast<size_t>(n), be = N * kRespawnWords * sizeof(double);
    if (finished_out && respawn_overlap(finished_out, be, episode, be)) return "finished_out overlaps episode";
    if (respawn_overlap(mask_out, N, episode, be)) return "mask_out overlaps episode";
    return nullptr;
}
static void launch_respawn(a1mpc_handle h, RespawnArgs& a, uint32_t what, hipStream_t s) {
    a.n_regions = respawn_regions(h, what, a.region);
    if ((what & A1MPC_RESPAWN_EKF) != 0) h->ekf_ready_n = 0;   // (the next EKF launch runs the init kernel again; it returns at once for a robot whose flag word is not zero)
    if (a.mask && a.n_regions == 0) return;
    hipLaunchKernelGGL(a1mpc_respawn_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(a.n) + 63) / 64)), dim3(64), 0, s, a);
}
static RespawnArgs respawn_args(int32_t n, const uint8_t* mask, const a1mpc_respawn_config* cfg, double* episode, int32_t* life, double* finished_out, uint8_t* mask_out) {
    RespawnArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.mask = mask; a.record = episode; a.life = life; a.finished = finished_out; a.mask_out = mask_out;
    if (cfg) { a.codes = cfg->codes; a.hold_ticks = cfg->hold_ticks; a.max_ticks = static_cast<double>(cfg->max_ticks); }
    return a;
}
a1mpc_status a1mpc_respawn_reset_batch_device(a1mpc_handle h, int32_t n, const uint8_t* d_mask, uint32_t what, void* hip_stream) {
    if (const char* bad = invalid_respawn_reset(h, n, d_mask, what)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    RespawnArgs a = respawn_args(n, d_mask, nullptr, nullptr, nullptr, nullptr, nullptr);
    A1_STAGE_LAUNCH(launch_respawn(h, a, what, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_respawn_reset_batch(a1mpc_handle h, int32_t n, const uint8_t* mask, uint32_t what) {
    if (const char* bad = invalid_respawn_reset(h, n, mask, what)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    const uint8_t* d_mask = sg.in(mask, 1);
    A1_STAGED(sg);
    RespawnArgs a = respawn_args(n, d_mask, nullptr, nullptr, nullptr, nullptr, nullptr);
    A1_STAGE_LAUNCH(launch_respawn(h, a, what, s));
    return sg.finish();
}
a1mpc_status a1mpc_respawn_batch_device(a1mpc_handle h, const a1mpc_respawn_config* cfg, int32_t n, double* d_episode, int32_t* d_life, double* d_finished_out,
                                        uint8_t* d_mask_out, void* hip_stream) {
    if (const char* bad = invalid_respawn(h, cfg, n, d_episode, d_life, d_finished_out, d_mask_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(hip_stream);
    RespawnArgs a = respawn_args(n, nullptr, cfg, d_episode, d_life, d_finished_out, d_mask_out);
    A1_STAGE_LAUNCH(launch_respawn(h, a, cfg->what, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_respawn_batch(a1mpc_handle h, const a1mpc_respawn_config* cfg, int32_t n, double* episode, int32_t* life, double* finished_out, uint8_t* mask_out) {
    if (const char* bad = invalid_respawn(h, cfg, n, episode, life, finished_out, mask_out)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    A1_STAGE_DEVICE(nullptr);
    Staging sg(h, n, s);
    double* d_episode = sg.inout(episode, kRespawnWords);
    double* d_life = sg.inout(reinterpret_cast<double*>(life), 1);   // (two int32 per robot: one staging word)
    double* d_finished = finished_out ? sg.inout(finished_out, kRespawnWords) : nullptr;   // (in as well: a row the call does not write keeps its bits)
    uint8_t* d_mask = sg.out(mask_out, 1);
    A1_STAGED(sg);
    RespawnArgs a = respawn_args(n, nullptr, cfg, d_episode, reinterpret_cast<int32_t*>(d_life), d_finished, d_mask);
    A1_STAGE_LAUNCH(launch_respawn(h, a, cfg->what, s));
    return sg.finish();
}
a1mpc_status a1mpc_respawn_rows_device(a1mpc_handle h, int32_t n, const uint8_t* d_mask, const a1mpc_respawn_rows* rows, int32_t n_rows, void* hip_stream) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!d_mask) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null mask");
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");
    if (n_rows < 0 || n_rows > A1MPC_RESPAWN_ROWS_MAX) return fail(A1MPC_ERR_INVALID_ARGUMENT, "n_rows outside 0 .. A1MPC_RESPAWN_ROWS_MAX");
    if (!rows) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null rows");
    RespawnRowsArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.n_rows = n_rows; a.mask = d_mask;
    for (int k = 0; k < n_rows; ++k) {
        const a1mpc_respawn_rows& r = rows[k];
        const std::string at = "a1mpc_respawn_rows[" + std::to_string(k) + "].";
        if (!r.dst) return fail(A1MPC_ERR_INVALID_ARGUMENT, at + "dst is null");
        if (!r.src) return fail(A1MPC_ERR_INVALID_ARGUMENT, at + "src is null");
        if (r.row_bytes < 1 || r.row_bytes > 4096) return fail(A1MPC_ERR_INVALID_ARGUMENT, at + "row_bytes outside 1 .. 4096");
        if (r.src_rows != 1 && r.src_rows < n) return fail(A1MPC_ERR_INVALID_ARGUMENT, at + "src_rows is neither 1 nor >= n");
        if (r.when == 0 || (r.when & ~3u)) return fail(A1MPC_ERR_INVALID_ARGUMENT, at + "when must be 1, 2 or 3");
        const bool broadcast = r.src_rows == 1;
        const size_t rb = static_cast<size_t>(r.row_bytes), N = static_cast<size_t>(n);
        if (respawn_overlap(r.dst, N * rb, r.src, (broadcast ? 1 : N) * rb)) return fail(A1MPC_ERR_INVALID_ARGUMENT, at + "dst overlaps src");
        const bool wide = ((reinterpret_cast<uintptr_t>(r.dst) | reinterpret_cast<uintptr_t>(r.src) | static_cast<uintptr_t>(r.row_bytes)) & 7) == 0;
        a.row[k] = RespawnRow{static_cast<char*>(r.dst), static_cast<const char*>(r.src), r.row_bytes, broadcast ? 1 : 0, static_cast<int32_t>(r.when), wide ? 1 : 0};
    }
    A1_STAGE_DEVICE(hip_stream);
    if (n_rows == 0) return A1MPC_OK;
    A1_STAGE_LAUNCH(hipLaunchKernelGGL(a1mpc_respawn_rows_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + 63) / 64)), dim3(64), 0, s, a));
    return A1MPC_OK;
}
#undef A1_STAGE_BEGIN
#undef A1_STAGE_DEVICE
#undef A1_STAGE_LAUNCH
#undef A1_STAGED

void a1mpc_default_tick_params(a1mpc_tick_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    a1mpc_default_gait_config(&p->gait);
    a1mpc_default_contact_config(&p->contact);
    p->control_dt = 0.0025; p->assume_flat_ground = 1;
    const double kp[3] = {300.0, 400.0, 400.0}, kd[3] = {8.0, 8.0, 8.0}, km[3] = {0.1, 0.1, 0.04};   // kp_foot / kd_foot / km_foot of the Gazebo parameter set (config/gazebo_a1_mpc.yaml)
    std::memcpy(p->kp_foot, kp, sizeof kp); std::memcpy(p->kd_foot, kd, sizeof kd); std::memcpy(p->km_foot, km, sizeof km);
    const double ox = 0.1805, oy = 0.047, d = 0.0838, lt = 0.21, lc = 0.21;   // A1 leg geometry, S/GazeboA1ROS.cpp:20-50 (leg_offset_x/y, motor_offset, upper / lower leg length)
    const double sx[4] = {1, 1, -1, -1}, sy[4] = {1, -1, 1, -1};
    for (int i = 0; i < 4; ++i) { double* f = p->rho_fix + 5 * i; f[0] = sx[i] * ox; f[1] = sy[i] * oy; f[2] = sy[i] * d; f[3] = lt; f[4] = lc; }
}

// One control tick of n robots in ONE call, device-resident: the reference's chain  joint-state callback (leg FK / Jacobians, S/GazeboA1ROS.cpp:264-279)
// -> A1BasicEKF::update_estimation (S/A1BasicEKF.cpp:70-163) -> update_plan (S/A1RobotControl.cpp:148-202) -> generate_swing_legs_ctrl (:204-287, with the contact logic and
// the terrain fit of compute_grf :335-376) -> compute_grf (:446-562) -> compute_joint_torques (:289-319), as driven by S/MainGazebo.cpp:47-119 -- six kernels, the tick-record
// pack and the MPC launch back to back on one stream, no host round trip, and N3 inside the MPC kernel's output stage whenever the tick runs the fused / latency kernel
// (every warm-started tick of a known batch).  Bit-identical to chaining the seven *_device entry points.
// pv: the gait-aware horizon (a1mpc_control_tick_preview_device), or null / {0, 0, *}: the plain tick -- the same launches as before the preview existed
// every refusal of a control tick, none of which needs the device: shared by control_tick_impl and by a1mpc_control_tick_sensors_device, which must have made them all
// before its front end launches
static a1mpc_status invalid_tick_call(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_preview_config* pv, const a1mpc_tick_buffers* bf, int32_t n, bool footholds) {
    if (!h || !p || !bf) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / params / buffers");
    const bool pv_sched = pv != nullptr && pv->contact_schedule == 1, pv_feet = pv != nullptr && pv->foot_preview != 0;
    if ((pv_sched || pv_feet) && !(p->gait.counter_per_gait > 0)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "a1mpc_gait_config.counter_per_gait <= 0");
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (h->cfg.horizon < 2) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "tick records need horizon >= 2");
    const void* need[] = {bf->joint_pos, bf->joint_vel, bf->R_world, bf->R_z, bf->root_euler, bf->root_ang_vel, bf->imu_acc, bf->imu_ang_vel, bf->foot_force, bf->movement_mode,
                          bf->mpc_active, bf->root_lin_vel_d, bf->root_ang_vel_d, bf->root_pos_d_z, bf->gait_counter_speed, bf->torques_gravity, bf->gait_counter, bf->foot_pos_start,
                          bf->foot_pos_rel_last_time, bf->foot_pos_target_last_time, bf->root_euler_d, bf->joint_torques, bf->root_pos, bf->root_lin_vel, bf->estimated_contacts,
                          bf->plan_contacts, bf->contacts, bf->foot_pos_rel, bf->j_foot_blocks, bf->foot_vel_rel, bf->foot_pos_abs, bf->foot_pos_target_rel, bf->foot_pos_cur,
                          bf->foot_forces_kin, bf->foot_pos_recent_contact, bf->terrain_angle, bf->grf};
    for (const void* q : need) if (!q) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null device pointer in a1mpc_tick_buffers (only the optional outputs may be null)");
    if (footholds && pv_feet && !bf->foot_pos_target_abs)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null a1mpc_tick_buffers.foot_pos_target_abs: the foothold preview reads it (foot_preview != 0)");
    if (!(p->control_dt > 0)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "control_dt <= 0");
    return A1MPC_OK;
}
static a1mpc_status control_tick_impl(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_preview_config* pv, const a1mpc_tick_buffers* bf, int32_t n, void* hip_stream,
                                      bool footholds = false) {
    if (a1mpc_status st = invalid_tick_call(h, p, pv, bf, n, footholds); st != A1MPC_OK) return st;
    const bool pv_sched = pv != nullptr && pv->contact_schedule == 1, pv_feet = pv != nullptr && pv->foot_preview != 0;
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream;
    A1_ORDER(h, s);
    if (!h->d_tickrec) A1_HIP(hipMalloc(&h->d_tickrec, (static_cast<size_t>(h->max_batch) * 22 + 3) * sizeof(double)));
    if (pv_sched && !h->d_pv_sched) A1_HIP(hipMalloc(&h->d_pv_sched, static_cast<size_t>(h->max_batch) * h->cfg.horizon * sizeof(uint32_t)));
    if (pv_feet && !h->d_pv_foot) A1_HIP(hipMalloc(&h->d_pv_foot, static_cast<size_t>(h->max_batch) * 12 * h->cfg.horizon * sizeof(double)));
    if (a1mpc_status st = ensure_ekf_state(h, s); st != A1MPC_OK) return st;
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    if (!h->timing && (tick_markers() & 2)) A1_HIP(hipEventRecord(h->ev_mark, s));
    if (h->timing) A1_HIP(hipEventRecord(h->ev_tick0, s));   // (ev_tick0 .. ev_tick1 = the whole tick; ev0 .. ev1 = the MPC launch, as after every solve)
    // 1. leg state (uses the previous estimate of root_pos / root_lin_vel for the world-frame outputs, like the reference's callback)
    launch_leg(n, p->rho_fix, p->rho_opt, bf->joint_pos, bf->joint_vel, bf->R_world, bf->root_pos, bf->root_lin_vel, bf->foot_pos_rel, bf->j_foot_blocks, bf->foot_vel_rel,
               bf->foot_pos_abs, bf->foot_vel_abs, bf->foot_pos_world, bf->foot_vel_world, s);
    // 2. EKF
    A1_LAUNCH_EKF(h, n, p->control_dt, p->assume_flat_ground, bf->movement_mode, bf->foot_force, bf->R_world, bf->imu_acc, bf->imu_ang_vel, bf->foot_pos_rel, bf->foot_vel_rel,
                  bf->root_pos, bf->root_lin_vel, bf->estimated_contacts, s);
    // 3. update_plan + 4. swing legs, one launch (a1mpc_plan_swing_kernel).  (Round 5 trial: the swing block as its own launch on a second stream beside stage 5 --
    //    both only need the plan's outputs -- joined in front of the MPC launch: the two cross-stream event waits cost more than the 5 us kernel they hide,
    //    0.490 -> 0.503 ms per tick at 4096 robots; profiles/r05_control_tick.txt)
    hipLaunchKernelGGL(a1mpc_plan_swing_kernel, leg_lane_grid(n), dim3(256), 0, s,
                       make_plan_args(p->gait, n, bf->movement_mode, bf->gait_counter, bf->gait_counter_speed, bf->root_lin_vel, bf->R_z, bf->R_world, bf->root_pos, bf->root_lin_vel_d,
                                      bf->plan_contacts, bf->foot_pos_target_rel, bf->foot_pos_target_abs, bf->foot_pos_target_world),
                       make_swing_args(n, p->gait.counter_per_swing, p->control_dt, p->kp_foot, p->kd_foot, bf->R_z, bf->foot_pos_abs, bf->gait_counter, bf->foot_pos_target_rel,
                                       bf->foot_pos_start, bf->foot_pos_rel_last_time, bf->foot_pos_target_last_time, bf->foot_pos_cur, bf->foot_forces_kin));
    {   // 5. contacts / terrain: root_pos[2] and root_euler_d[1] are read / written in place (strides of 3); 6. the tick record, by the same lanes
        ContactArgs a = make_contact_args(h, p->contact, n, bf->gait_counter, bf->plan_contacts, bf->foot_force, bf->foot_pos_abs, bf->root_pos + 2, bf->root_euler_d + 1, bf->contacts,
                                          bf->foot_pos_recent_contact, bf->terrain_angle);
        a.z_stride = 3; a.pitch_stride = 3;
        a.pk_euler = bf->root_euler; a.pk_pos = bf->root_pos; a.pk_ang_vel = bf->root_ang_vel; a.pk_lin_vel = bf->root_lin_vel; a.pk_euler_d = bf->root_euler_d;
        a.pk_lin_vel_d = bf->root_lin_vel_d; a.pk_ang_vel_d = bf->root_ang_vel_d; a.pk_pos_d_z = bf->root_pos_d_z; a.pk_tick = h->d_tickrec;
        launch_contact_terrain(a, s);
    }
    A1_HIP(hipGetLastError());
    double* d_km = h->d_tickrec + static_cast<size_t>(h->max_batch) * 22;
    if (std::memcmp(h->tick_km, p->km_foot, sizeof h->tick_km) != 0 || !h->tick_km_set) {   // km_foot travels once (and again when it changes): the output stage reads it from device memory
        std::memcpy(h->tick_km, p->km_foot, sizeof h->tick_km); h->tick_km_set = true;
        std::memcpy(h->h_pin, p->km_foot, 3 * sizeof(double));   // (a pinned source; the handle's pinned block is free: this entry point takes no host arrays)
        A1_HIP(hipMemcpyAsync(d_km, h->h_pin, 3 * sizeof(double), hipMemcpyHostToDevice, s));
        A1_HIP(hipStreamSynchronize(s));   // (once: the pinned words may be overwritten by a later host-pointer call)
    }
    // 6b. the gait-aware horizon: the contact schedule (step 0 = the contacts stage 5 has just written) and / or the per-step feet, into the handle's buffers
    const double* mpc_foot = bf->foot_pos_abs; const uint8_t* mpc_contact = bf->contacts;
    if (pv_sched || pv_feet) {
        launch_preview(h, *pv, p->gait.counter_per_gait, p->gait.counter_per_swing, n, bf->movement_mode, bf->gait_counter, bf->gait_counter_speed, bf->contacts, bf->foot_pos_abs,
                       bf->R_world, bf->root_lin_vel_d, pv_sched ? reinterpret_cast<uint8_t*>(h->d_pv_sched) : nullptr, pv_feet ? h->d_pv_foot : nullptr, s,
                       footholds ? bf->foot_pos_target_abs : nullptr);   // (stage 3 of this tick wrote it)
        A1_HIP(hipGetLastError());
        if (pv_sched) mpc_contact = reinterpret_cast<const uint8_t*>(h->d_pv_sched);
        if (pv_feet) mpc_foot = h->d_pv_foot;
    }
    // 7. MPC from the tick records + N3 in its output stage (fast kernels: with a schedule that stage reads step 0, the actual contacts; the general kernels -- per-step
    //    feet -- have no such stage and leave `fused` false)
    TorqueFuse tq{bf->mpc_active, bf->j_foot_blocks, bf->foot_forces_kin, bf->torques_gravity, d_km, bf->joint_torques, false};
    if (a1mpc_status st = solve_device_impl(h, n, h->d_tickrec, nullptr, nullptr, bf->R_world, mpc_foot, mpc_contact, bf->grf, nullptr, bf->iters, bf->status, s, pv_feet ? 12 : 0,
                                            pv_sched ? 4 : 0, nullptr, &tq);
        st != A1MPC_OK) return st;
    if (!tq.fused) {   // the split pipeline solved this tick (a first tick, a batch beyond the fused kernel's range): N3 as its own launch
        launch_torque(n, bf->mpc_active, bf->contacts, bf->j_foot_blocks, bf->grf, bf->foot_forces_kin, p->km_foot, bf->torques_gravity, bf->joint_torques, s);
        A1_HIP(hipGetLastError());
    }
    h->tick_fused = tq.fused;
    if (h->timing) A1_HIP(hipEventRecord(h->ev_tick1, s)); else if (tick_markers() & 8) A1_HIP(hipEventRecord(h->ev_mark, s));
    h->tick_timed = h->timing;
    A1_MARK(h, s);
    return A1MPC_OK;
}
#undef A1_LAUNCH_EKF
a1mpc_status a1mpc_control_tick_device(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_tick_buffers* bf, int32_t n, void* hip_stream) {
    return control_tick_impl(h, p, nullptr, bf, n, hip_stream);
}
// The control tick from raw inputs: the sensor stage, the command stage, then exactly a1mpc_control_tick_device, back to back on one stream.  Every refusal of the three
// is made before the first launch (the tick's own by invalid_tick_call, the function control_tick_impl makes them with)
a1mpc_status a1mpc_control_tick_sensors_device(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_tick_sensors* sn, const a1mpc_tick_buffers* bf, int32_t n, void* hip_stream) {
    if (!h || !p || !sn || !bf) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / params / sensors / buffers");
    // the eleven fields the front end produces are inputs of the tick: the caller's storage, written here (a1mpc_tick_buffers declares them const for the tick's sake)
    const SensorIo si{sn->quat, sn->imu_acc_raw, sn->imu_gyro_raw, const_cast<double*>(bf->R_world), const_cast<double*>(bf->R_z), const_cast<double*>(bf->root_euler),
                      const_cast<double*>(bf->imu_acc), const_cast<double*>(bf->imu_ang_vel), const_cast<double*>(bf->root_ang_vel)};
    const CommandIo ci{sn->cmd, sn->mode_toggle, bf->root_pos, p->control_dt, sn->body_height, sn->ctrl_state, bf->root_euler_d, sn->root_pos_d, sn->kp_linear_xy,
                       sn->mpc_init_counter, const_cast<double*>(bf->root_lin_vel_d), const_cast<double*>(bf->root_ang_vel_d), const_cast<uint8_t*>(bf->movement_mode),
                       const_cast<uint8_t*>(bf->mpc_active), const_cast<double*>(bf->root_pos_d_z)};
    if (const char* bad = invalid_sensor_call(h, &sn->sensor, n, si)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (const char* bad = invalid_command_call(&sn->command, n, ci)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (a1mpc_status st = invalid_tick_call(h, p, nullptr, bf, n, false); st != A1MPC_OK) return st;   // the tick's own refusals, before the front end launches
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream;
    A1_ORDER(h, s);
    if (a1mpc_status st = ensure_sensor_state(h, sn->sensor.imu_window, s); st != A1MPC_OK) return st;
    launch_sensor(h, sn->sensor.imu_window, n, si, s);
    launch_command(sn->command, n, ci, s);
    A1_HIP(hipGetLastError());
    A1_MARK(h, s);
    return control_tick_impl(h, p, nullptr, bf, n, hip_stream);
}
// a1mpc_control_tick_device with the preview kernel between the contacts / terrain stage and the MPC launch; {0, 0, *} is a1mpc_control_tick_device
a1mpc_status a1mpc_control_tick_preview_device(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_preview_config* pv, const a1mpc_tick_buffers* bf, int32_t n, void* hip_stream) {
    if (const char* bad = invalid_preview(h, pv)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    return control_tick_impl(h, p, pv, bf, n, hip_stream);
}
// ... with the feet of a leg that lands inside the horizon at this tick's Raibert foothold, buffers->foot_pos_target_abs; foot_preview 0 IS a1mpc_control_tick_preview_device
a1mpc_status a1mpc_control_tick_preview_footholds_device(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_preview_config* pv, const a1mpc_tick_buffers* bf, int32_t n,
                                                         void* hip_stream) {
    if (const char* bad = invalid_preview(h, pv)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    return control_tick_impl(h, p, pv, bf, n, hip_stream, true);
}
a1mpc_status a1mpc_last_control_tick_ms(a1mpc_handle h, float* ms_out, int32_t* torques_fused_out) {
    if (!h || !ms_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/out");
    if (!h->tick_timed) return fail(A1MPC_ERR_INVALID_ARGUMENT, "no control tick has been launched through this handle");
    A1_HIP(hipSetDevice(h->device));
    A1_HIP(hipEventSynchronize(h->ev_tick1));
    A1_HIP(hipEventElapsedTime(ms_out, h->ev_tick0, h->ev_tick1));
    if (torques_fused_out) *torques_fused_out = h->tick_fused ? 1 : 0;
    return A1MPC_OK;
}

// ---- the small-batch transport of the host-pointer entries.  A handful of QPs (the drop-in's calls are n = 1) is not staged through device memory: the caller's
// arrays are packed into the handle's PINNED block (device-mapped host memory: 1.3 KB in, ~100 B out per QP over PCIe, a few transactions), the kernel reads its
// inputs from and writes its results to that block itself, and the host polls the output words -- the staging copies each cost more on the GPU's timeline than
// the bytes they move.  Same kernels, same bits.  Each entry states its layout and its launch: pin_inputs, arm_outputs, launch, wait_outputs, host_collect.
//
// Every output word is its own completion flag.  The bytes the kernel is about to write are filled with a bit pattern no result has (a quiet NaN with a payload as a
// double -- forces are finite or exactly zero, a failed solve's u is the payload-free NaN --, 0x7ff85a5a as an int32: no iteration count, no status), and the host
// polls until no word holds it any more instead of waiting in hipStreamSynchronize(): it is awake 5 us earlier (p99: 9 us; tools/ubench/completion_wake_ubench.hip).
// No ordering between the kernel's stores is assumed: polling `status` alone, stored last behind a system-scope release, saw the forces arrive AFTER it on 2 of
// 10 000 ticks (posted writes over PCIe with relaxed ordering).
constexpr unsigned long long kInFlightWord = 0x7ff85a5a7ff85a5aull;

// The output region of N QPs from `base` (the pinned block's, as the host or the device sees it, or d_out for a staged launch): [grf | iters | status | u], u_width
// doubles of u per QP -- 12H for the MPC entries, 12 (f_world) for the balance QP, 0 where the caller passed no such array (u = null).  bytes: what a launch writes.
struct HostOut { double* grf; int32_t *iters, *status; double* u; size_t bytes; };
static HostOut host_out_layout(char* base, size_t N, size_t u_width) {
    const size_t q_it = N * 12 * sizeof(double), q_st = q_it + N * sizeof(int32_t), q_u = q_st + N * sizeof(int32_t);
    return {reinterpret_cast<double*>(base), reinterpret_cast<int32_t*>(base + q_it), reinterpret_cast<int32_t*>(base + q_st),
            u_width ? reinterpret_cast<double*>(base + q_u) : nullptr, q_u + N * u_width * sizeof(double)};
}

// The caller's arrays packed, in the order given, into the pinned block's input region (the double arrays first, the byte arrays last, each at an 8-byte aligned
// offset; a null array takes no room and has a null address).  f64(i), u8(i): array i as the device sees it from `base` -- d_pin, or d_in after a staged copy of `bytes`.
struct PinIn { const void* src; size_t bytes; };
struct PinnedIn {
    static constexpr size_t kNone = ~size_t(0);
    const char* base; size_t off[6]; size_t bytes;   // (six arrays at most: the general path's layout)
    const char* at(int i) const { return off[i] == kNone ? nullptr : base + off[i]; }
    const double* f64(int i) const { return reinterpret_cast<const double*>(at(i)); }
    const uint8_t* u8(int i) const { return reinterpret_cast<const uint8_t*>(at(i)); }
};
static PinnedIn pin_inputs(a1mpc_handle h, std::initializer_list<PinIn> arrays) {
    PinnedIn p{h->d_pin, {}, 0};
    int i = 0;
    for (const PinIn& a : arrays) {
        const size_t o = (p.bytes + 7) / 8 * 8;
        p.off[i++] = a.src ? o : PinnedIn::kNone;
        if (a.src) { std::memcpy(h->h_pin + o, a.src, a.bytes); p.bytes = o + a.bytes; }
    }
    return p;
}

// Arms the output region for a small-batch launch of N QPs (every word it will write holds kInFlightWord) and returns it as the device sees it
static HostOut arm_outputs(a1mpc_handle h, size_t N, size_t u_width) {
    const HostOut o = host_out_layout(h->d_pin + h->h_pin_in_bytes, N, u_width);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(h->h_pin + h->h_pin_in_bytes);
    for (size_t i = 0; i < o.bytes / 8; ++i) w[i] = kInFlightWord;
    std::atomic_thread_fence(std::memory_order_release);
    return o;
}

// Has the kernel written every armed word?  [12N grf doubles | 2N iters, status int32 | u doubles up to `armed` bytes]
static bool outputs_landed(const char* hout, size_t N, size_t armed) {
    const volatile unsigned long long* w64 = reinterpret_cast<const volatile unsigned long long*>(hout);
    const volatile uint32_t* w32 = reinterpret_cast<const volatile uint32_t*>(hout);
    for (size_t i = 24 * N; i < 26 * N; ++i) if (w32[i] == static_cast<uint32_t>(kInFlightWord)) return false;   // (written last by the kernel: the cheap test first)
    for (size_t i = 0; i < 12 * N; ++i) if (w64[i] == kInFlightWord) return false;
    for (size_t i = 13 * N; i < armed / 8; ++i) if (w64[i] == kInFlightWord) return false;
    return true;
}

// Waits for the launch just queued on the handle's stream: polls the `armed` bytes of the output region (and the stream now and then: a launch that failed never
// writes them), or synchronises the stream where nothing was armed (a staged launch).  A word still in flight once the stream has finished is an error, never a result.
static a1mpc_status wait_outputs(a1mpc_handle h, size_t N, size_t armed, const char* path) {
    if (armed == 0) { A1_HIP(hipStreamSynchronize(h->stream)); return A1MPC_OK; }
    const char* hout = h->h_pin + h->h_pin_in_bytes;
    for (unsigned spin = 1; !outputs_landed(hout, N, armed); ++spin) {
        if ((spin & 0xffff) == 0 && hipStreamQuery(h->stream) != hipErrorNotReady) {   // (about once a millisecond) finished -- the words arrive with it -- or failed
            A1_HIP(hipStreamSynchronize(h->stream));
            if (!outputs_landed(hout, N, armed)) return fail(A1MPC_ERR_HIP, std::string(path) + ": the launch finished with output words still in flight");
            break;
        }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return A1MPC_OK;
}

// The pinned block's output region (after wait_outputs, or after the stream has copied a staged launch's outputs into it) into the caller's arrays
static void host_collect(a1mpc_handle h, size_t N, size_t u_width, double* grf_body_out, double* u_out, int32_t* iters_out, int32_t* status_out) {
    const HostOut o = host_out_layout(h->h_pin + h->h_pin_in_bytes, N, u_width);
    std::memcpy(grf_body_out, o.grf, N * 12 * sizeof(double));
    if (u_out) std::memcpy(u_out, o.u, N * u_width * sizeof(double));
    if (iters_out) std::memcpy(iters_out, o.iters, N * sizeof(int32_t));
    if (status_out) std::memcpy(status_out, o.status, N * sizeof(int32_t));
}

a1mpc_status a1mpc_solve_batch_ticks(a1mpc_handle h, int32_t n, const double* tick, const double* R_world, const double* foot_abs,
                                     const uint8_t* contact, double* grf_body_out, double* u_full_out, int32_t* iters_out,
                                     int32_t* status_out) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || !tick || !R_world || !foot_abs || !contact || !grf_body_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    const size_t N = n, H = h->cfg.horizon;
    if (H < 2) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "tick records need horizon >= 2");
    if (small_batch(h, n)) {   // a handful of ticks (the drop-in's compute_grf is n = 1)
        const PinnedIn in = pin_inputs(h, {{tick, N * 22 * sizeof(double)}, {R_world, N * 9 * sizeof(double)}, {foot_abs, N * 12 * sizeof(double)}, {contact, N * 4}});
        const HostOut o = arm_outputs(h, N, u_full_out ? 12 * H : 0);
        if (a1mpc_status st = a1mpc_solve_batch_ticks_device(h, n, in.f64(0), in.f64(1), in.f64(2), in.u8(3), o.grf, o.u, o.iters, o.status,
                                                             h->stream); st != A1MPC_OK) return st;
        if (a1mpc_status st = wait_outputs(h, N, o.bytes, "a1mpc_solve_batch_ticks"); st != A1MPC_OK) return st;
        host_collect(h, N, 12 * H, grf_body_out, u_full_out, iters_out, status_out);
        return A1MPC_OK;
    }
    hipStream_t s = h->stream;
    A1_ORDER(h, s);
    // 22 + 9 + 12 doubles + 4 bytes per QP: the tick record rides in the x_ref staging buffer (13H >= 22 for H >= 2; H = 1 has its own room: 13 + 13)
    double* d_tick = (H >= 2) ? h->d_xref : h->d_x0;
    A1_HIP(hipMemcpyAsync(d_tick, tick, N * 22 * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_R, R_world, N * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_foot, foot_abs, N * 12 * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_contact, contact, N * 4, hipMemcpyHostToDevice, s));
    a1mpc_status st = solve_device_impl(h, n, d_tick, nullptr, nullptr, h->d_R, h->d_foot, h->d_contact, h->d_grf,
                                        u_full_out ? h->d_u : nullptr, h->d_iters, h->d_status, s);
    if (st != A1MPC_OK) return st;
    A1_HIP(hipMemcpyAsync(grf_body_out, h->d_grf, N * 12 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (u_full_out) A1_HIP(hipMemcpyAsync(u_full_out, h->d_u, N * 12 * H * sizeof(double), hipMemcpyDeviceToHost, s));
    if (iters_out) A1_HIP(hipMemcpyAsync(iters_out, h->d_iters, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (status_out) A1_HIP(hipMemcpyAsync(status_out, h->d_status, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    A1_HIP(hipStreamSynchronize(s));
    return A1MPC_OK;
}

// The host-pointer MPC entry in two halves, so that a pipeline slot can leave a batch in flight (a1mpc_pipeline_submit):
//   host_submit   snapshot the caller's arrays into the pinned block (the caller's program mutates them concurrently) laid out exactly like the device
//                 block; a small batch is launched on the pinned block itself (*armed: the output bytes armed), a larger one is staged -- one H2D copy,
//                 the launches, one D2H copy into the pinned mirror (*armed = 0) -- all queued on the handle's stream, nothing waited for;
//   host_collect  (after wait_outputs) the pinned mirror into the caller's output arrays.
static a1mpc_status host_submit(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world, const double* foot_abs,
                                const uint8_t* contact, bool want_u, size_t* armed) {
    A1_HIP(hipSetDevice(h->device));
    const size_t N = n, H = h->cfg.horizon;
    PinnedIn in = pin_inputs(h, {{x0, N * 13 * sizeof(double)}, {x_ref, N * 13 * H * sizeof(double)}, {R_world, N * 9 * sizeof(double)},
                                 {foot_abs, N * 12 * sizeof(double)}, {contact, N * 4}});
    hipStream_t s = h->stream;
    A1_ORDER(h, s);
    *armed = 0;
    if (small_batch(h, n)) {
        const HostOut o = arm_outputs(h, N, want_u ? 12 * H : 0);
        *armed = o.bytes;
        return a1mpc_solve_batch_device(h, n, in.f64(0), in.f64(1), in.f64(2), in.f64(3), in.u8(4), o.grf, o.u, o.iters, o.status, s);
    }
    A1_HIP(hipMemcpyAsync(h->d_in, h->h_pin, in.bytes, hipMemcpyHostToDevice, s));
    in.base = h->d_in;
    const HostOut o = host_out_layout(h->d_out, N, want_u ? 12 * H : 0);
    a1mpc_status st = a1mpc_solve_batch_device(h, n, in.f64(0), in.f64(1), in.f64(2), in.f64(3), in.u8(4), o.grf, o.u, o.iters, o.status, s);
    if (st != A1MPC_OK) return st;
    A1_HIP(hipMemcpyAsync(h->h_pin + h->h_pin_in_bytes, h->d_out, o.bytes, hipMemcpyDeviceToHost, s));
    return A1MPC_OK;
}

a1mpc_status a1mpc_solve_batch(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                               const double* foot_abs, const uint8_t* contact, double* grf_body_out, double* u_full_out,
                               int32_t* iters_out, int32_t* status_out) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || !x0 || !x_ref || !R_world || !foot_abs || !contact || !grf_body_out)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    size_t armed = 0;
    if (a1mpc_status st = host_submit(h, n, x0, x_ref, R_world, foot_abs, contact, u_full_out != nullptr, &armed); st != A1MPC_OK) return st;
    if (a1mpc_status st = wait_outputs(h, n, armed, "a1mpc_solve_batch"); st != A1MPC_OK) return st;
    host_collect(h, n, 12 * h->cfg.horizon, grf_body_out, u_full_out, iters_out, status_out);
    return A1MPC_OK;
}

// ---- the dense QP the reference's ConvexMpc members hold (debug / verification; see a1mpc_form_kernel)
a1mpc_status a1mpc_form_qp_batch(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world, const double* foot_abs,
                                 int32_t foot_stride, const uint8_t* contact, int32_t contact_stride, const double* yaw_A, double* P_out, double* g_out,
                                 double* l_out, double* u_out) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || !x0 || !x_ref || !R_world || !foot_abs || !contact || !P_out || !g_out || !l_out || !u_out)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (!((foot_stride == 0 || foot_stride == 12) && (contact_stride == 0 || contact_stride == 4)))
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    const size_t N = n, H = h->cfg.horizon, nv = 12 * H, nc = 20 * H, nfoot = foot_stride ? 12 * H : 12, ncont = contact_stride ? 4 * H : 4;
    hipStream_t s = h->stream;
    A1_ORDER(h, s);
    // own, call-scoped device buffers: this is a verification path, not a tick
    double *d_in = nullptr, *d_out = nullptr;
    uint8_t* d_c = nullptr;
    const size_t in_d = N * (13 + 13 * H + 9 + nfoot + 1), out_d = N * (nv * nv + nv + 2 * nc);
    A1_HIP(hipMalloc(&d_in, in_d * sizeof(double)));
    hipError_t e1 = hipMalloc(&d_out, out_d * sizeof(double)), e2 = hipMalloc(&d_c, N * ncont);
    if (e1 != hipSuccess || e2 != hipSuccess) { (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_c); return fail(A1MPC_ERR_HIP, "hipMalloc (a1mpc_form_qp_batch)"); }
    double *dx0 = d_in, *dxr = dx0 + N * 13, *dR = dxr + N * 13 * H, *df = dR + N * 9, *dyaw = df + N * nfoot;
    double *dP = d_out, *dg = dP + N * nv * nv, *dl = dg + N * nv, *du = dl + N * nc;
    hipError_t e = hipMemcpyAsync(dx0, x0, N * 13 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dxr, x_ref, N * 13 * H * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dR, R_world, N * 9 * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(df, foot_abs, N * nfoot * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_c, contact, N * ncont, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && yaw_A) e = hipMemcpyAsync(dyaw, yaw_A, N * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        FormArgs a;
        a.P = h->dp; a.n = n; a.H = static_cast<int32_t>(H); a.foot_stride = foot_stride; a.contact_stride = contact_stride;
        a.x0 = dx0; a.xref = dxr; a.R = dR; a.foot = df; a.contact = d_c; a.yaw_A = yaw_A ? dyaw : nullptr; a.Pout = dP; a.gout = dg; a.lout = dl; a.uout = du;
        hipLaunchKernelGGL(a1mpc_form_kernel, dim3(static_cast<unsigned>(N)), dim3(256), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(P_out, dP, N * nv * nv * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g_out, dg, N * nv * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(l_out, dl, N * nc * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(u_out, du, N * nc * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_c);
    if (e != hipSuccess) return fail(A1MPC_ERR_HIP, std::string("a1mpc_form_qp_batch: ") + hipGetErrorString(e));
    return A1MPC_OK;
}

a1mpc_status a1mpc_solve_batch_strided_device(a1mpc_handle h, int32_t n, const double* d_x0, const double* d_x_ref, const double* d_R_world,
                                              const double* d_foot_abs, int32_t foot_stride, const uint8_t* d_contact, int32_t contact_stride,
                                              const double* d_yaw_A, double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out,
                                              int32_t* d_status_out, void* hip_stream) {
    if (!d_x0 || !d_x_ref) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (!strides_ok(foot_stride, contact_stride)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    return solve_device_impl(h, n, nullptr, d_x0, d_x_ref, d_R_world, d_foot_abs, d_contact, d_grf_body_out, d_u_full_out, d_iters_out,
                             d_status_out, hip_stream, foot_stride, contact_stride, d_yaw_A);
}
// The host-pointer strided entry in two halves, like host_submit / host_collect (a pipeline slot leaves the batch in flight: a1mpc_pipeline_submit_strided).
// strided_host_submit: the caller's arrays are snapshotted by pageable H2D copies on the handle's stream (synchronous w.r.t. the host buffers), the launches and ONE
// D2H copy into the handle's pinned mirror are queued; host_collect hands the mirror to the caller's arrays once the stream has drained.
static a1mpc_status strided_host_submit(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world, const double* foot_abs, int32_t foot_stride,
                                        const uint8_t* contact, int32_t contact_stride, const double* yaw_A, bool want_u) {
    A1_HIP(hipSetDevice(h->device));
    const size_t N = n, H = h->cfg.horizon, nfoot = foot_stride ? 12 * H : 12, ncont = contact_stride ? 4 * H : 4;
    hipStream_t s = h->stream;
    A1_ORDER(h, s);
    if (!h->d_foot_steps) {
        A1_HIP(hipMalloc(&h->d_foot_steps, static_cast<size_t>(h->max_batch) * 12 * H * sizeof(double)));
        A1_HIP(hipMalloc(&h->d_contact_steps, static_cast<size_t>(h->max_batch) * 4 * H));
    }
    A1_HIP(hipMemcpyAsync(h->d_x0, x0, N * 13 * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_xref, x_ref, N * 13 * H * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_R, R_world, N * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_foot_steps, foot_abs, N * nfoot * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_contact_steps, contact, N * ncont, hipMemcpyHostToDevice, s));
    if (yaw_A) A1_HIP(hipMemcpyAsync(h->d_aux, yaw_A, N * sizeof(double), hipMemcpyHostToDevice, s));  // d_aux: n x 6 doubles of balance-QP staging, free here
    const HostOut o = host_out_layout(h->d_out, N, want_u ? 12 * H : 0);
    a1mpc_status st = solve_device_impl(h, n, nullptr, h->d_x0, h->d_xref, h->d_R, h->d_foot_steps, h->d_contact_steps, o.grf, o.u, o.iters, o.status, s,
                                        foot_stride, contact_stride, yaw_A ? h->d_aux : nullptr);
    if (st != A1MPC_OK) return st;
    A1_HIP(hipMemcpyAsync(h->h_pin + h->h_pin_in_bytes, h->d_out, o.bytes, hipMemcpyDeviceToHost, s));
    return A1MPC_OK;
}
a1mpc_status a1mpc_solve_batch_strided(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                                       const double* foot_abs, int32_t foot_stride, const uint8_t* contact, int32_t contact_stride,
                                       const double* yaw_A, double* grf_body_out, double* u_full_out, int32_t* iters_out, int32_t* status_out) {
    if (!strides_ok(foot_stride, contact_stride)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    if (foot_stride == 0 && contact_stride == 0 && !yaw_A)  // the reference controller's case: the fast path, bit for bit
        return a1mpc_solve_batch(h, n, x0, x_ref, R_world, foot_abs, contact, grf_body_out, u_full_out, iters_out, status_out);
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || !x0 || !x_ref || !R_world || !foot_abs || !contact || !grf_body_out)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    const size_t N = n, H = h->cfg.horizon;
    if (N <= small_general_max() && h->d_pin != nullptr) {   // a handful of QPs on the general path (the drop-in's ConvexMpc-level call is n = 1)
        A1_HIP(hipSetDevice(h->device));
        const size_t nfoot = foot_stride ? 12 * H : 12, ncont = contact_stride ? 4 * H : 4;
        const PinnedIn in = pin_inputs(h, {{x0, N * 13 * sizeof(double)}, {x_ref, N * 13 * H * sizeof(double)}, {R_world, N * 9 * sizeof(double)},
                                           {foot_abs, N * nfoot * sizeof(double)}, {yaw_A, N * sizeof(double)}, {contact, N * ncont}});
        const HostOut o = arm_outputs(h, N, u_full_out ? 12 * H : 0);
        if (a1mpc_status st = solve_device_impl(h, n, nullptr, in.f64(0), in.f64(1), in.f64(2), in.f64(3), in.u8(5), o.grf, o.u, o.iters,
                                                o.status, h->stream, foot_stride, contact_stride, in.f64(4)); st != A1MPC_OK) return st;
        if (a1mpc_status st = wait_outputs(h, N, o.bytes, "a1mpc_solve_batch_strided (general path)"); st != A1MPC_OK) return st;
        host_collect(h, N, 12 * H, grf_body_out, u_full_out, iters_out, status_out);
        return A1MPC_OK;
    }
    if (a1mpc_status st = strided_host_submit(h, n, x0, x_ref, R_world, foot_abs, foot_stride, contact, contact_stride, yaw_A, u_full_out != nullptr); st != A1MPC_OK) return st;
    A1_HIP(hipStreamSynchronize(h->stream));
    host_collect(h, N, 12 * H, grf_body_out, u_full_out, iters_out, status_out);
    return A1MPC_OK;
}
// Tick records + strides, host pointers: staged through device memory at every n (the tick record rides in the x_ref staging buffer like a1mpc_solve_batch_ticks',
// feet and contacts in the per-step staging of a1mpc_solve_batch_strided), one D2H copy of the packed outputs into the pinned mirror
a1mpc_status a1mpc_solve_batch_ticks_strided(a1mpc_handle h, int32_t n, const double* tick, const double* R_world, const double* foot_abs, int32_t foot_stride,
                                             const uint8_t* contact, int32_t contact_stride, const double* yaw_A, double* grf_body_out, double* u_full_out,
                                             int32_t* iters_out, int32_t* status_out) {
    if (!strides_ok(foot_stride, contact_stride)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    if (foot_stride == 0 && contact_stride == 0 && !yaw_A)   // a1mpc_solve_batch_ticks itself: same transport, same kernels, same bits
        return a1mpc_solve_batch_ticks(h, n, tick, R_world, foot_abs, contact, grf_body_out, u_full_out, iters_out, status_out);
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || !tick || !R_world || !foot_abs || !contact || !grf_body_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (h->cfg.horizon < 2) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "tick records need horizon >= 2");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    if (a1mpc_status st = ensure_step_staging(h); st != A1MPC_OK) return st;
    const size_t N = n, H = h->cfg.horizon, nfoot = foot_stride ? 12 * H : 12, ncont = contact_stride ? 4 * H : 4;
    hipStream_t s = h->stream;
    A1_ORDER(h, s);
    A1_HIP(hipMemcpyAsync(h->d_xref, tick, N * 22 * sizeof(double), hipMemcpyHostToDevice, s));   // (13H >= 22 doubles per QP for H >= 2)
    A1_HIP(hipMemcpyAsync(h->d_R, R_world, N * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_foot_steps, foot_abs, N * nfoot * sizeof(double), hipMemcpyHostToDevice, s));
    A1_HIP(hipMemcpyAsync(h->d_contact_steps, contact, N * ncont, hipMemcpyHostToDevice, s));
    if (yaw_A) A1_HIP(hipMemcpyAsync(h->d_aux, yaw_A, N * sizeof(double), hipMemcpyHostToDevice, s));  // d_aux: n x 6 doubles of balance-QP staging, free here
    const HostOut o = host_out_layout(h->d_out, N, u_full_out ? 12 * H : 0);
    if (a1mpc_status st = solve_device_impl(h, n, h->d_xref, nullptr, nullptr, h->d_R, h->d_foot_steps, h->d_contact_steps, o.grf, o.u, o.iters, o.status, s, foot_stride,
                                            contact_stride, yaw_A ? h->d_aux : nullptr); st != A1MPC_OK) return st;
    A1_HIP(hipMemcpyAsync(h->h_pin + h->h_pin_in_bytes, h->d_out, o.bytes, hipMemcpyDeviceToHost, s));
    A1_HIP(hipStreamSynchronize(s));
    host_collect(h, N, 12 * H, grf_body_out, u_full_out, iters_out, status_out);
    return A1MPC_OK;
}
// the balance QP as the H = 1 member of the kernel family: dt = 0, wrench weights (torque first) in q2[6:12], R on the diagonal, the handle's OSQP settings with the
// warm start off.  The caller sets the input / output pointers
static KernelArgs balance_kernel_args(a1mpc_handle h, const a1mpc_balance_config& qp, int32_t n) {
    KernelArgs a;
    std::memset(&a, 0, sizeof a);
    a.P = h->dp;
    a.P.dt = 0.0; a.P.mu = qp.mu; a.P.fz_min = qp.F_min; a.P.fz_max = qp.F_max; a.P.warm_start = 0;
    for (int i = 0; i < 12; ++i) { a.P.q2[i] = 0.0; a.P.r2[i] = qp.R; }
    for (int k = 0; k < 3; ++k) { a.P.q2[6 + k] = qp.Q[3 + k]; a.P.q2[9 + k] = qp.Q[k]; }
    a.tab = h->d_tab1; a.n = n; a.nfact = h->d_nfact;
    return a;
}
// the balance launch on device pointers between the handle's timing events (a1mpc_last_kernel_ms, a1mpc_last_nfact); the caller has ordered the stream and marks it
static a1mpc_status launch_balance_device(a1mpc_handle h, const a1mpc_balance_config& qp, int32_t n, const double* root_acc, const double* R_world, const double* R_z,
                                          const double* foot_abs, const uint8_t* contact, double* grf_body_out, double* f_world_out, int32_t* iters_out,
                                          int32_t* status_out, hipStream_t s) {
    KernelArgs a = balance_kernel_args(h, qp, n);
    a.root_acc = root_acc; a.R = R_world; a.Rz = R_z; a.foot = foot_abs; a.contact = contact;
    a.grf = grf_body_out; a.u_full = f_world_out; a.iters = iters_out; a.status = status_out;
    if (h->timing) A1_HIP(hipEventRecord(h->ev0, s));
    h->staged = false;
    if (a1mpc_status st = launch<1, kModeBalance>(a, s); st != A1MPC_OK) return st;
    if (h->timing) A1_HIP(hipEventRecord(h->ev1, s));
    h->timed = h->timing;
    return A1MPC_OK;
}
a1mpc_status a1mpc_balance_solve_batch(a1mpc_handle h, const a1mpc_balance_config* qp, int32_t n, const double* root_acc,
                                       const double* R_world, const double* R_z, const double* foot_abs, const uint8_t* contact,
                                       double* grf_body_out, double* f_world_out, int32_t* iters_out, int32_t* status_out) {
    if (!h || !qp) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/config");
    if (const char* why = invalid_balance_config(*qp)) return fail(A1MPC_ERR_INVALID_ARGUMENT, why);
    if (n < 0 || !root_acc || !R_world || !R_z || !foot_abs || !contact || !grf_body_out)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    const size_t N = n;
    hipStream_t s = h->stream;
    A1_ORDER(h, s);
    KernelArgs a = balance_kernel_args(h, *qp, n);
    size_t armed = 0;
    if (small_batch(h, n)) {   // a handful of QPs (the drop-in's compute_grf with stance_leg_control_type = 0 is n = 1)
        const PinnedIn in = pin_inputs(h, {{root_acc, N * 6 * sizeof(double)}, {R_world, N * 9 * sizeof(double)}, {R_z, N * 9 * sizeof(double)},
                                           {foot_abs, N * 12 * sizeof(double)}, {contact, N * 4}});
        const HostOut o = arm_outputs(h, N, f_world_out ? 12 : 0);
        a.root_acc = in.f64(0); a.R = in.f64(1); a.Rz = in.f64(2); a.foot = in.f64(3); a.contact = in.u8(4);
        a.grf = o.grf; a.u_full = o.u; a.iters = o.iters; a.status = o.status;
        armed = o.bytes;
    } else {   // larger batches: the transfers are small (344 B per QP); pageable copies on the stream are synchronous w.r.t. the host buffer
        A1_HIP(hipMemcpyAsync(h->d_aux, root_acc, N * 6 * sizeof(double), hipMemcpyHostToDevice, s));
        A1_HIP(hipMemcpyAsync(h->d_R, R_world, N * 9 * sizeof(double), hipMemcpyHostToDevice, s));
        A1_HIP(hipMemcpyAsync(h->d_Rz, R_z, N * 9 * sizeof(double), hipMemcpyHostToDevice, s));
        A1_HIP(hipMemcpyAsync(h->d_foot, foot_abs, N * 12 * sizeof(double), hipMemcpyHostToDevice, s));
        A1_HIP(hipMemcpyAsync(h->d_contact, contact, N * 4, hipMemcpyHostToDevice, s));
        a.root_acc = h->d_aux; a.Rz = h->d_Rz; a.R = h->d_R; a.foot = h->d_foot; a.contact = h->d_contact;
        a.grf = h->d_grf; a.u_full = h->d_u; a.iters = h->d_iters; a.status = h->d_status;
    }
    if (h->timing) A1_HIP(hipEventRecord(h->ev0, s));
    h->staged = false;
    a1mpc_status st = launch<1, kModeBalance>(a, s);
    if (st != A1MPC_OK) return st;
    if (h->timing) A1_HIP(hipEventRecord(h->ev1, s));
    h->timed = h->timing;
    A1_MARK(h, s);
    if (armed) {
        if (a1mpc_status sw = wait_outputs(h, N, armed, "a1mpc_balance_solve_batch"); sw != A1MPC_OK) return sw;
        host_collect(h, N, 12, grf_body_out, f_world_out, iters_out, status_out);
        return A1MPC_OK;
    }
    A1_HIP(hipMemcpyAsync(grf_body_out, h->d_grf, N * 12 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (f_world_out) A1_HIP(hipMemcpyAsync(f_world_out, h->d_u, N * 12 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (iters_out) A1_HIP(hipMemcpyAsync(iters_out, h->d_iters, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (status_out) A1_HIP(hipMemcpyAsync(status_out, h->d_status, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    A1_HIP(hipStreamSynchronize(s));
    return A1MPC_OK;
}
// a1mpc_balance_solve_batch on device pointers: asynchronous on hip_stream (NULL = the handle's), no host synchronisation, no pinned small-batch block -- the same
// argument fill and the same launch, the same bits
a1mpc_status a1mpc_balance_solve_batch_device(a1mpc_handle h, const a1mpc_balance_config* qp, int32_t n, const double* d_root_acc, const double* d_R_world,
                                              const double* d_R_z, const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out, double* d_f_world_out,
                                              int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream) {
    if (!h || !qp) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/config");
    if (const char* why = invalid_balance_config(*qp)) return fail(A1MPC_ERR_INVALID_ARGUMENT, why);
    if (n < 0 || !d_root_acc || !d_R_world || !d_R_z || !d_foot_abs || !d_contact || !d_grf_body_out)
        return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream;
    A1_ORDER(h, s);
    if (a1mpc_status st = launch_balance_device(h, *qp, n, d_root_acc, d_R_world, d_R_z, d_foot_abs, d_contact, d_grf_body_out, d_f_world_out, d_iters_out, d_status_out, s);
        st != A1MPC_OK) return st;
    A1_MARK(h, s);
    return A1MPC_OK;
}

// One control tick of n robots on the balance-QP stance controller (stance_leg_control_type 0) in ONE call: stages 1-4 of control_tick_impl (leg state, EKF, plan, swing
// legs), the contact block WITHOUT the terrain fit (S/A1RobotControl.cpp:335) and without a tick record, then compute_grf's other branch -- the PD wrench (:379-391), the
// 12-variable QP (:393-444) -- and compute_joint_torques (:289-319) as a launch of its own, back to back on one stream, no host round trip.  Bit-identical to chaining
// a1mpc_leg_state_batch_device, a1mpc_ekf_update_batch_device, a1mpc_update_plan_batch_device, a1mpc_swing_legs_batch_device, a1mpc_contacts_batch_device,
// a1mpc_balance_wrench_batch_device, a1mpc_balance_solve_batch_device, a1mpc_joint_torques_batch_device.  buffers->root_pos_d_z and ->terrain_angle are not used (either
// may be null), ->root_euler_d is read only; any horizon of the handle will do
a1mpc_status a1mpc_control_tick_balance_device(a1mpc_handle h, const a1mpc_tick_params* p, const a1mpc_balance_tick* bt, const a1mpc_tick_buffers* bf, int32_t n,
                                               void* hip_stream) {
    if (!h || !p || !bt || !bf) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle / params / balance tick / buffers");
    if (const char* bad = invalid_balance_gains(&bt->gains)) return fail(A1MPC_ERR_INVALID_ARGUMENT, bad);
    if (const char* why = invalid_balance_config(bt->qp)) return fail(A1MPC_ERR_INVALID_ARGUMENT, why);
    if (n < 0) return fail(A1MPC_ERR_INVALID_ARGUMENT, "negative n");
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_create");
    if (!bt->root_pos_d) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null a1mpc_balance_tick.root_pos_d");
    const void* need[] = {bf->joint_pos, bf->joint_vel, bf->R_world, bf->R_z, bf->root_euler, bf->root_ang_vel, bf->imu_acc, bf->imu_ang_vel, bf->foot_force, bf->movement_mode,
                          bf->mpc_active, bf->root_lin_vel_d, bf->root_ang_vel_d, bf->gait_counter_speed, bf->torques_gravity, bf->gait_counter, bf->foot_pos_start,
                          bf->foot_pos_rel_last_time, bf->foot_pos_target_last_time, bf->root_euler_d, bf->joint_torques, bf->root_pos, bf->root_lin_vel, bf->estimated_contacts,
                          bf->plan_contacts, bf->contacts, bf->foot_pos_rel, bf->j_foot_blocks, bf->foot_vel_rel, bf->foot_pos_abs, bf->foot_pos_target_rel, bf->foot_pos_cur,
                          bf->foot_forces_kin, bf->foot_pos_recent_contact, bf->grf};
    for (const void* q : need) if (!q) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null device pointer in a1mpc_tick_buffers (only the optional outputs, root_pos_d_z and terrain_angle may be null)");
    if (!(p->control_dt > 0)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "control_dt <= 0");
    if (n == 0) return A1MPC_OK;
    A1_HIP(hipSetDevice(h->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream;
    A1_ORDER(h, s);
    double* root_acc = bt->root_acc;
    if (!root_acc) {   // the handle's own, allocated once
        if (!h->d_bal_acc) A1_HIP(hipMalloc(&h->d_bal_acc, static_cast<size_t>(h->max_batch) * 6 * sizeof(double)));
        root_acc = h->d_bal_acc;
    }
    if (a1mpc_status st = ensure_ekf_state(h, s); st != A1MPC_OK) return st;
    if (a1mpc_status st = ensure_contact_state(h, s); st != A1MPC_OK) return st;
    if (h->timing) A1_HIP(hipEventRecord(h->ev_tick0, s));   // (ev_tick0 .. ev_tick1 = the whole tick; ev0 .. ev1 = the balance launch)
    // 1. leg state, 2. EKF, 3. update_plan + 4. swing legs: the launches of control_tick_impl
    launch_leg(n, p->rho_fix, p->rho_opt, bf->joint_pos, bf->joint_vel, bf->R_world, bf->root_pos, bf->root_lin_vel, bf->foot_pos_rel, bf->j_foot_blocks, bf->foot_vel_rel,
               bf->foot_pos_abs, bf->foot_vel_abs, bf->foot_pos_world, bf->foot_vel_world, s);
    if (a1mpc_status st = launch_ekf(h, n, p->control_dt, p->assume_flat_ground, bf->movement_mode, bf->foot_force, bf->R_world, bf->imu_acc, bf->imu_ang_vel, bf->foot_pos_rel,
                                     bf->foot_vel_rel, bf->root_pos, bf->root_lin_vel, bf->estimated_contacts, s); st != A1MPC_OK) return st;
    hipLaunchKernelGGL(a1mpc_plan_swing_kernel, leg_lane_grid(n), dim3(256), 0, s,
                       make_plan_args(p->gait, n, bf->movement_mode, bf->gait_counter, bf->gait_counter_speed, bf->root_lin_vel, bf->R_z, bf->R_world, bf->root_pos, bf->root_lin_vel_d,
                                      bf->plan_contacts, bf->foot_pos_target_rel, bf->foot_pos_target_abs, bf->foot_pos_target_world),
                       make_swing_args(n, p->gait.counter_per_swing, p->control_dt, p->kp_foot, p->kd_foot, bf->R_z, bf->foot_pos_abs, bf->gait_counter, bf->foot_pos_target_rel,
                                       bf->foot_pos_start, bf->foot_pos_rel_last_time, bf->foot_pos_target_last_time, bf->foot_pos_cur, bf->foot_forces_kin));
    // 5. the contact block alone, 6. the PD wrench from this tick's estimate
    launch_contacts(h, p->contact, n, bf->gait_counter, bf->plan_contacts, bf->foot_force, bf->foot_pos_abs, bf->contacts, bf->foot_pos_recent_contact, s);
    launch_wrench(h, bt->gains, n, bt->root_pos_d, bf->root_pos, bf->root_lin_vel_d, bf->root_lin_vel, bf->root_euler_d, bf->root_euler, bf->root_ang_vel_d, bf->root_ang_vel,
                  bf->R_world, root_acc, s);
    A1_HIP(hipGetLastError());
    // 7. the balance QP, 8. joint torques
    if (a1mpc_status st = launch_balance_device(h, bt->qp, n, root_acc, bf->R_world, bf->R_z, bf->foot_pos_abs, bf->contacts, bf->grf, bt->f_world, bf->iters, bf->status, s);
        st != A1MPC_OK) return st;
    launch_torque(n, bf->mpc_active, bf->contacts, bf->j_foot_blocks, bf->grf, bf->foot_forces_kin, p->km_foot, bf->torques_gravity, bf->joint_torques, s);
    A1_HIP(hipGetLastError());
    h->tick_fused = false;
    if (h->timing) A1_HIP(hipEventRecord(h->ev_tick1, s));
    h->tick_timed = h->timing;
    A1_MARK(h, s);
    return A1MPC_OK;
}

a1mpc_status a1mpc_last_kernel_ms(a1mpc_handle h, float* ms_out) {
    if (!h || !ms_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/out");
    if (!h->timed) return fail(A1MPC_ERR_INVALID_ARGUMENT, "no kernel has been launched through this handle");
    A1_HIP(hipSetDevice(h->device));
    A1_HIP(hipEventSynchronize(h->ev1));
    A1_HIP(hipEventElapsedTime(ms_out, h->ev0, h->ev1));
    return A1MPC_OK;
}

a1mpc_status a1mpc_last_stage_ms(a1mpc_handle h, float* form_ms_out, float* solve_ms_out) {
    if (!h || !form_ms_out || !solve_ms_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/out");
    if (!h->timed) return fail(A1MPC_ERR_INVALID_ARGUMENT, "no kernel has been launched through this handle");
    A1_HIP(hipSetDevice(h->device));
    A1_HIP(hipEventSynchronize(h->ev1));
    if (h->staged) {
        A1_HIP(hipEventElapsedTime(form_ms_out, h->ev0, h->ev_mid));
        A1_HIP(hipEventElapsedTime(solve_ms_out, h->ev_mid, h->ev1));
    } else {  // fused / latency kernel: one launch from inputs to outputs, the stages are not separable from outside
        *form_ms_out = 0.0f;
        A1_HIP(hipEventElapsedTime(solve_ms_out, h->ev0, h->ev1));
    }
    return A1MPC_OK;
}

a1mpc_status a1mpc_last_nfact(a1mpc_handle h, int32_t n, int32_t* nfact_out) {
    if (!h || !nfact_out || n < 0 || n > h->max_batch) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/out or bad n");
    if (!h->timed) return fail(A1MPC_ERR_INVALID_ARGUMENT, "no kernel has been launched through this handle");
    A1_HIP(hipSetDevice(h->device));
    A1_HIP(hipStreamSynchronize(h->last_stream));
    A1_HIP(hipMemcpy(nfact_out, h->d_nfact, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return A1MPC_OK;
}

a1mpc_status a1mpc_kernel_info(a1mpc_handle h, int32_t* lds_bytes_per_workgroup, int32_t* qps_per_workgroup,
                               int32_t* threads_per_workgroup) {
    if (!h) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    // the geometry of the persistent ADMM kernel large batches run, from where its launch takes it (the fused / latency kernels of small batches: one wavefront of
    // default_rows_per_wg QPs)
    const Geometry g = ops_of(h->cfg.horizon)->admm_geometry();
    if (lds_bytes_per_workgroup) *lds_bytes_per_workgroup = static_cast<int32_t>(g.lds);
    if (qps_per_workgroup) *qps_per_workgroup = g.qps;
    if (threads_per_workgroup) *threads_per_workgroup = g.threads;
    return A1MPC_OK;
}

// ======================================================================================================================
// Batch sharding across the GPUs of one node inside the C ABI (SURVEY 8b "device = -1 = all", 8e): one host thread, one handle and one
// stream per device, the batch cut into contiguous shards (sizes differ by at most one, remainder to the low shards -- the QPs are
// independent, there is no data-path collective).  Two transports for scatter-inputs / gather-GRFs:
//   0  pinned host memory, one hipMemcpyAsync fan-out per device each way (no root hop; every GPU is fed over its own PCIe link)
//   1  RCCL over xGMI: the whole batch goes to shard 0's GPU in one copy, grouped ncclSend / ncclRecv move the other shards' inputs
//      out and their results back (the north_star's named path); librccl.so is dlopen()ed on first use
// The same device may be listed twice (two shards on one GPU: how the single-GPU test box exercises transport 0).
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load() {
        if (lib) return true;
        lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) return false;
#define A1_SYM(n) n = reinterpret_cast<decltype(n)>(dlsym(lib, "nccl" #n))
        A1_SYM(CommInitAll); A1_SYM(CommDestroy); A1_SYM(CommAbort); A1_SYM(GroupStart); A1_SYM(GroupEnd); A1_SYM(Send); A1_SYM(Recv); A1_SYM(GetErrorString);
#undef A1_SYM
        return CommInitAll && CommDestroy && CommAbort && GroupStart && GroupEnd && Send && Recv && GetErrorString;
    }
};
static RcclApi g_rccl;

struct a1mpc_sharded_s {
    int ndev = 0, transport = 0, max_batch = 0, horizon = 0;
    std::vector<int> dev;
    std::vector<a1mpc_handle> h;            // one engine handle per shard (its own stream, staging, warm start)
    char* pin = nullptr;                    // pinned mirror of inputs + outputs (transport 0; transport 1 uses it for the two big copies)
    size_t pin_bytes = 0;
    // transport 1: the whole batch on shard 0's device + communicators
    double *r_x0 = nullptr, *r_xref = nullptr, *r_R = nullptr, *r_foot = nullptr, *r_grf = nullptr;
    uint8_t* r_contact = nullptr;
    int32_t *r_iters = nullptr, *r_status = nullptr;
    std::vector<ncclComm_t> comm;
    std::vector<hipEvent_t> ev;             // per shard: "my part of this call is finished"
    bool broken = false;                    // an error inside an open RCCL group: the communicators were aborted, the handle only accepts a1mpc_sharded_destroy
    long long last_scatter_bytes = 0, last_gather_bytes = 0;   // what the last solve moved from the root to the other shards and back (a1mpc_sharded_last_transfer)
};
static void shard_range(int n, int g, int G, int* start, int* count) {
    const int base = n / G, rem = n % G;
    *count = base + (g < rem ? 1 : 0);
    *start = g * base + (g < rem ? g : rem);
}

void a1mpc_sharded_destroy(a1mpc_sharded S) {
    if (!S) return;
    for (size_t g = 0; g < S->comm.size(); ++g) if (S->comm[g] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(S->comm[g]);
    if (!S->dev.empty()) (void)hipSetDevice(S->dev[0]);
    void* ptrs[] = {S->r_x0, S->r_xref, S->r_R, S->r_foot, S->r_grf, S->r_contact, S->r_iters, S->r_status};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (size_t g = 0; g < S->ev.size(); ++g) if (S->ev[g]) { (void)hipSetDevice(S->dev[g]); (void)hipEventDestroy(S->ev[g]); }
    for (a1mpc_handle h : S->h) a1mpc_destroy(h);
    if (S->pin) (void)hipHostFree(S->pin);
    delete S;
}

a1mpc_status a1mpc_sharded_create(const a1mpc_config* cfg, int32_t max_batch, const int32_t* devices, int32_t n_devices, int32_t transport,
                                  a1mpc_sharded* out) {
    if (!cfg || !out || max_batch <= 0 || (transport != 0 && transport != 1)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null config/out, bad batch or transport");
    *out = nullptr;
    if (ops_of(cfg->horizon) == nullptr) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "horizon must be " A1MPC_HORIZON_LIST);
    if (const char* why = invalid_config(*cfg)) return fail(A1MPC_ERR_INVALID_ARGUMENT, why);
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) return fail(A1MPC_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    a1mpc_sharded S = new (std::nothrow) a1mpc_sharded_s();
    if (!S) return fail(A1MPC_ERR_HIP, "out of host memory");
    if (n_devices <= 0 || !devices) { for (int d = 0; d < visible; ++d) S->dev.push_back(d); }   // -1 = all visible devices
    else for (int g = 0; g < n_devices; ++g) {
        if (devices[g] < 0 || devices[g] >= visible) { delete S; return fail(A1MPC_ERR_NO_DEVICE, "device ordinal out of range"); }
        S->dev.push_back(devices[g]);
    }
    S->ndev = static_cast<int>(S->dev.size()); S->transport = transport; S->max_batch = max_batch; S->horizon = cfg->horizon;
    const int per = (max_batch + S->ndev - 1) / S->ndev;
    const size_t N = max_batch, H = cfg->horizon;
    for (int g = 0; g < S->ndev; ++g) {
        a1mpc_handle hg = nullptr;
        const a1mpc_status st = a1mpc_create(cfg, per, S->dev[g], &hg);
        if (st != A1MPC_OK) { a1mpc_sharded_destroy(S); return st; }
        S->h.push_back(hg);
        hipEvent_t e = nullptr;
        if (hipSetDevice(S->dev[g]) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { a1mpc_sharded_destroy(S); return fail(A1MPC_ERR_HIP, "hipEventCreate"); }
        S->ev.push_back(e);
    }
    S->pin_bytes = N * ((13 + 13 * H + 9 + 12 + 12) * sizeof(double) + 4 + 2 * sizeof(int32_t));
    if (hipHostMalloc(reinterpret_cast<void**>(&S->pin), S->pin_bytes, hipHostMallocPortable) != hipSuccess) { a1mpc_sharded_destroy(S); return fail(A1MPC_ERR_HIP, "hipHostMalloc"); }
    if (transport == 1) {
        for (int a = 0; a < S->ndev; ++a) for (int b = a + 1; b < S->ndev; ++b)
            if (S->dev[a] == S->dev[b]) { a1mpc_sharded_destroy(S); return fail(A1MPC_ERR_INVALID_ARGUMENT, "RCCL transport needs distinct devices"); }
        if (!g_rccl.load()) { a1mpc_sharded_destroy(S); return fail(A1MPC_ERR_HIP, std::string("cannot load librccl.so: ") + (dlerror() ? dlerror() : "missing symbols")); }
        S->comm.assign(S->ndev, nullptr);
        const ncclResult_t rc = g_rccl.CommInitAll(S->comm.data(), S->ndev, S->dev.data());
        if (rc != ncclSuccess) { S->comm.clear(); a1mpc_sharded_destroy(S); return fail(A1MPC_ERR_HIP, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(rc)); }
        bool ok = hipSetDevice(S->dev[0]) == hipSuccess;
        ok = ok && hipMalloc(&S->r_x0, N * 13 * sizeof(double)) == hipSuccess && hipMalloc(&S->r_xref, N * 13 * H * sizeof(double)) == hipSuccess;
        ok = ok && hipMalloc(&S->r_R, N * 9 * sizeof(double)) == hipSuccess && hipMalloc(&S->r_foot, N * 12 * sizeof(double)) == hipSuccess;
        ok = ok && hipMalloc(&S->r_contact, N * 4) == hipSuccess && hipMalloc(&S->r_grf, N * 12 * sizeof(double)) == hipSuccess;
        ok = ok && hipMalloc(&S->r_iters, N * sizeof(int32_t)) == hipSuccess && hipMalloc(&S->r_status, N * sizeof(int32_t)) == hipSuccess;
        if (!ok) { a1mpc_sharded_destroy(S); return fail(A1MPC_ERR_HIP, "hipMalloc (root staging of the RCCL transport)"); }
    }
    *out = S;
    return A1MPC_OK;
}

a1mpc_status a1mpc_sharded_info(a1mpc_sharded S, int32_t* n_shards, int32_t* devices_out, int32_t* transport) {
    if (!S) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n_shards) *n_shards = S->ndev;
    if (devices_out) for (int g = 0; g < S->ndev; ++g) devices_out[g] = S->dev[g];
    if (transport) *transport = S->transport;
    return A1MPC_OK;
}

// One implementation behind the four entry points (round 6): inputs as (x0, x_ref) or as the compact tick records (S/A1RobotControl.cpp:452-488), in HOST
// arrays (snapshotted into the pinned mirror first) or in DEVICE arrays resident on shard 0's GPU (the root: the fleet's state lives there, shards are fed over xGMI --
// peer copies with transport 0, grouped ncclSend / ncclRecv with transport 1 -- and their results come back into the caller's arrays on the root).  Every shard's engine
// handle carries its own warm start / update-path workspace: with cfg.warm_start = 1 | 2 and a constant n the closed loop of a1mpc_solve_batch* runs unchanged, shard by shard.
struct ShardedIo {
    bool device = false;                      // the arrays below live on shard 0's device (else: host)
    const double *x0 = nullptr, *xref = nullptr, *tick = nullptr, *R = nullptr, *foot = nullptr;
    const uint8_t* contact = nullptr;
    double* grf = nullptr; int32_t *iters = nullptr, *status = nullptr;
    void* stream = nullptr;                   // device form: the root-device stream the inputs were produced on (NULL: they are ready)
};
static a1mpc_status sharded_solve_impl(a1mpc_sharded S, int32_t n, const ShardedIo& io) {
    if (!S) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    const bool ticks = io.tick != nullptr;
    if (n < 0 || (!ticks && (!io.x0 || !io.xref)) || !io.R || !io.foot || !io.contact || !io.grf) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (n > S->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_sharded_create");
    if (S->broken) return fail(A1MPC_ERR_HIP, "an earlier call failed inside an RCCL group and the communicators were aborted: destroy this handle and create a new one");
    if (ticks && S->horizon < 2) return fail(A1MPC_ERR_UNSUPPORTED_HORIZON, "tick records need horizon >= 2");
    if (n == 0) return A1MPC_OK;
    const size_t N = n, H = S->horizon, G = S->ndev;
    // the input fields of a QP: bytes per QP, where the whole batch lies (host forms: the pinned snapshot `pin` and, transport 1, the root staging `root`; device forms: the
    // caller's array on the root device) and which staging buffer of a shard's engine handle receives a slice (tick records ride in the x_ref buffer: 13 H >= 22)
    struct Field { size_t bytes; const char* pin; const char* root; int which; };
    Field in[5]; int nin = 0;
    char* p = S->pin;
    auto take = [&](size_t bytes) { char* q = p; p += N * bytes; return q; };
    char* p_a = take(ticks ? 22 * sizeof(double) : 13 * sizeof(double));
    char* p_b = ticks ? nullptr : take(13 * H * sizeof(double));
    char* p_R = take(9 * sizeof(double)); char* p_f = take(12 * sizeof(double));
    double* p_grf = reinterpret_cast<double*>(take(12 * sizeof(double)));
    int32_t* p_it = reinterpret_cast<int32_t*>(take(sizeof(int32_t))); int32_t* p_st = reinterpret_cast<int32_t*>(take(sizeof(int32_t)));
    char* p_c = take(4);
    if (io.device) {
        if (ticks) in[nin++] = {22 * sizeof(double), nullptr, reinterpret_cast<const char*>(io.tick), 1};
        else { in[nin++] = {13 * sizeof(double), nullptr, reinterpret_cast<const char*>(io.x0), 0}; in[nin++] = {13 * H * sizeof(double), nullptr, reinterpret_cast<const char*>(io.xref), 1}; }
        in[nin++] = {9 * sizeof(double), nullptr, reinterpret_cast<const char*>(io.R), 2}; in[nin++] = {12 * sizeof(double), nullptr, reinterpret_cast<const char*>(io.foot), 3};
        in[nin++] = {4, nullptr, reinterpret_cast<const char*>(io.contact), 4};
    } else {
        // pinned snapshot (the caller's program mutates its arrays concurrently, see a1mpc.h), field after field like the device layout
        if (ticks) { std::memcpy(p_a, io.tick, N * 22 * sizeof(double)); in[nin++] = {22 * sizeof(double), p_a, reinterpret_cast<const char*>(S->r_xref), 1}; }
        else {
            std::memcpy(p_a, io.x0, N * 13 * sizeof(double)); std::memcpy(p_b, io.xref, N * 13 * H * sizeof(double));
            in[nin++] = {13 * sizeof(double), p_a, reinterpret_cast<const char*>(S->r_x0), 0}; in[nin++] = {13 * H * sizeof(double), p_b, reinterpret_cast<const char*>(S->r_xref), 1};
        }
        std::memcpy(p_R, io.R, N * 9 * sizeof(double)); std::memcpy(p_f, io.foot, N * 12 * sizeof(double)); std::memcpy(p_c, io.contact, N * 4);
        in[nin++] = {9 * sizeof(double), p_R, reinterpret_cast<const char*>(S->r_R), 2}; in[nin++] = {12 * sizeof(double), p_f, reinterpret_cast<const char*>(S->r_foot), 3};
        in[nin++] = {4, p_c, reinterpret_cast<const char*>(S->r_contact), 4};
    }
    auto shard_buf = [](a1mpc_handle h, int which) -> char* {
        switch (which) {
            case 0: return reinterpret_cast<char*>(h->d_x0);
            case 1: return reinterpret_cast<char*>(h->d_xref);
            case 2: return reinterpret_cast<char*>(h->d_R);
            case 3: return reinterpret_cast<char*>(h->d_foot);
        }
        return reinterpret_cast<char*>(h->d_contact);
    };
    // where the results of the whole batch are collected on the root device (device forms: the caller's arrays; host forms with transport 1: the root staging)
    double* root_grf = io.device ? io.grf : S->r_grf;
    int32_t* root_it = io.device ? io.iters : S->r_iters;
    int32_t* root_st = io.device ? io.status : S->r_status;
    // Error handling of a multi-device call: nothing may be left behind -- an open RCCL group is closed and every shard's stream is drained (their async copies
    // target the shared pinned mirror, which the next call overwrites) before the status goes back to the caller.
    bool group_open = false;
    auto drain = [&]() {
        if (group_open && g_rccl.GroupEnd) {
            // A failure between paired ncclSend / ncclRecv calls leaves point-to-point operations without their partner: GroupEnd submits them and a stream
            // synchronise would then wait for ever.  Close the group, ABORT every communicator -- that terminates the operations in flight -- and only
            // then drain the streams; the handle is unusable afterwards (the solve entries refuse, a1mpc_sharded_destroy frees it).
            (void)g_rccl.GroupEnd(); group_open = false;
            for (size_t g = 0; g < S->comm.size(); ++g)
                if (S->comm[g]) { if (hipSetDevice(S->dev[g]) == hipSuccess) (void)g_rccl.CommAbort(S->comm[g]); S->comm[g] = nullptr; }
            S->broken = true;
        }
        for (size_t g = 0; g < G; ++g) { if (hipSetDevice(S->h[g]->device) == hipSuccess) (void)hipStreamSynchronize(S->h[g]->stream); }
    };
#define A1_SH_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { drain(); return fail(A1MPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } } while (0)
#define A1_SH_ST(call) do { a1mpc_status s_ = (call); if (s_ != A1MPC_OK) { drain(); return s_; } } while (0)
    a1mpc_handle h0 = S->h[0];
    const int dev0 = h0->device;
    S->last_scatter_bytes = S->last_gather_bytes = 0;
    // device forms: every shard's stream starts behind what the caller has queued on `stream` (an event of the root device; cross-device waits are stream-ordered)
    if (io.device && io.stream != nullptr) {
        A1_SH_HIP(hipSetDevice(dev0));
        A1_SH_HIP(hipEventRecord(S->ev[0], static_cast<hipStream_t>(io.stream)));
        for (size_t g = 0; g < G; ++g) { A1_SH_HIP(hipSetDevice(S->h[g]->device)); A1_SH_HIP(hipStreamWaitEvent(S->h[g]->stream, S->ev[0], 0)); }
    }
    // the solve of shard g: on its handle's staging buffers, or -- shard 0 of the device forms and of transport 1 -- in place on the root arrays
    auto solve_shard = [&](size_t g, int c, bool in_place, size_t o) -> a1mpc_status {
        a1mpc_handle h = S->h[g];
        if (in_place) {
            const char* base[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            for (int f = 0; f < nin; ++f) base[in[f].which] = in[f].root + o * in[f].bytes;
            return solve_device_impl(h, c, ticks ? reinterpret_cast<const double*>(base[1]) : nullptr, ticks ? nullptr : reinterpret_cast<const double*>(base[0]),
                                     ticks ? nullptr : reinterpret_cast<const double*>(base[1]), reinterpret_cast<const double*>(base[2]), reinterpret_cast<const double*>(base[3]),
                                     reinterpret_cast<const uint8_t*>(base[4]), root_grf + o * 12, nullptr, root_it ? root_it + o : h->d_iters, root_st ? root_st + o : h->d_status, h->stream);
        }
        return solve_device_impl(h, c, ticks ? h->d_xref : nullptr, ticks ? nullptr : h->d_x0, ticks ? nullptr : h->d_xref, h->d_R, h->d_foot, h->d_contact, h->d_grf, nullptr,
                                 h->d_iters, h->d_status, h->stream);
    };
    if (S->transport == 0) {
        for (size_t g = 0; g < G; ++g) {   // everything asynchronous: the G devices copy and solve concurrently
            int s0 = 0, c = 0;
            shard_range(n, static_cast<int>(g), static_cast<int>(G), &s0, &c);
            if (c == 0) continue;
            a1mpc_handle h = S->h[g];
            A1_SH_HIP(hipSetDevice(h->device));
            hipStream_t st = h->stream;
            A1_SH_ST(order_streams(h, st));
            const size_t o = s0, C = c;
            const bool in_place = io.device && g == 0;   // shard 0 of a device-resident batch reads and writes the caller's arrays
            if (!in_place) {
                for (int f = 0; f < nin; ++f) {
                    if (io.device && h->device != dev0) A1_SH_HIP(hipMemcpyPeerAsync(shard_buf(h, in[f].which), h->device, in[f].root + o * in[f].bytes, dev0, C * in[f].bytes, st));   // over xGMI
                    else if (io.device) A1_SH_HIP(hipMemcpyAsync(shard_buf(h, in[f].which), in[f].root + o * in[f].bytes, C * in[f].bytes, hipMemcpyDeviceToDevice, st));   // (a second shard on the root's own GPU)
                    else A1_SH_HIP(hipMemcpyAsync(shard_buf(h, in[f].which), in[f].pin + o * in[f].bytes, C * in[f].bytes, hipMemcpyHostToDevice, st));
                    S->last_scatter_bytes += static_cast<long long>(C * in[f].bytes);
                }
            }
            A1_SH_ST(solve_shard(g, c, in_place, o));
            if (in_place) continue;
            if (io.device && h->device != dev0) {
                A1_SH_HIP(hipMemcpyPeerAsync(root_grf + o * 12, dev0, h->d_grf, h->device, C * 12 * sizeof(double), st));
                if (root_it) A1_SH_HIP(hipMemcpyPeerAsync(root_it + o, dev0, h->d_iters, h->device, C * sizeof(int32_t), st));
                if (root_st) A1_SH_HIP(hipMemcpyPeerAsync(root_st + o, dev0, h->d_status, h->device, C * sizeof(int32_t), st));
            } else if (io.device) {
                A1_SH_HIP(hipMemcpyAsync(root_grf + o * 12, h->d_grf, C * 12 * sizeof(double), hipMemcpyDeviceToDevice, st));
                if (root_it) A1_SH_HIP(hipMemcpyAsync(root_it + o, h->d_iters, C * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                if (root_st) A1_SH_HIP(hipMemcpyAsync(root_st + o, h->d_status, C * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            } else {
                A1_SH_HIP(hipMemcpyAsync(p_grf + o * 12, h->d_grf, C * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
                A1_SH_HIP(hipMemcpyAsync(p_it + o, h->d_iters, C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                A1_SH_HIP(hipMemcpyAsync(p_st + o, h->d_status, C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            }
            S->last_gather_bytes += static_cast<long long>(C * (12 * sizeof(double) + 2 * sizeof(int32_t)));
        }
        for (size_t g = 0; g < G; ++g) { A1_SH_HIP(hipSetDevice(S->h[g]->device)); A1_SH_HIP(hipStreamSynchronize(S->h[g]->stream)); }
    } else {
        // every RCCL call is issued with the device of ITS communicator current (one thread drives all the communicators of ncclCommInitAll: the stream
        // handed to a call belongs to that device)
#define A1_NCCL(dev, call) do { A1_SH_HIP(hipSetDevice(dev)); ncclResult_t r_ = (call); if (r_ != ncclSuccess) { drain(); return fail(A1MPC_ERR_HIP, std::string(#call) + ": " + g_rccl.GetErrorString(r_)); } } while (0)
        A1_SH_HIP(hipSetDevice(dev0));
        hipStream_t s0 = h0->stream;
        A1_SH_ST(order_streams(h0, s0));
        if (!io.device)   // host form: the whole batch to the root staging in one copy per field
            for (int f = 0; f < nin; ++f) A1_SH_HIP(hipMemcpyAsync(const_cast<char*>(in[f].root), in[f].pin, N * in[f].bytes, hipMemcpyHostToDevice, s0));
        for (size_t g = 1; g < G; ++g) { A1_SH_HIP(hipSetDevice(S->h[g]->device)); A1_SH_ST(order_streams(S->h[g], S->h[g]->stream)); }
        // scatter: shard g > 0 receives its slice of every field from shard 0's device (root drives all its xGMI links concurrently)
        A1_NCCL(dev0, g_rccl.GroupStart()); group_open = true;
        for (size_t g = 1; g < G; ++g) {
            int st0 = 0, c = 0;
            shard_range(n, static_cast<int>(g), static_cast<int>(G), &st0, &c);
            if (c == 0) continue;
            a1mpc_handle h = S->h[g];
            const size_t o = st0, C = c;
            const int gi = static_cast<int>(g);
            for (int f = 0; f < nin; ++f) {
                A1_NCCL(dev0, g_rccl.Send(in[f].root + o * in[f].bytes, C * in[f].bytes, ncclUint8, gi, S->comm[0], s0));
                A1_NCCL(h->device, g_rccl.Recv(shard_buf(h, in[f].which), C * in[f].bytes, ncclUint8, 0, S->comm[g], h->stream));
                S->last_scatter_bytes += static_cast<long long>(C * in[f].bytes);
            }
        }
        group_open = false;
        A1_NCCL(dev0, g_rccl.GroupEnd());
        // every shard solves on its own stream (stream order: after its receives); shard 0 works in place on the root buffers
        for (size_t g = 0; g < G; ++g) {
            int st0 = 0, c = 0;
            shard_range(n, static_cast<int>(g), static_cast<int>(G), &st0, &c);
            if (c == 0) continue;
            A1_SH_HIP(hipSetDevice(S->h[g]->device));
            A1_SH_ST(solve_shard(g, c, g == 0, static_cast<size_t>(st0)));
        }
        // gather: results of shard g > 0 back to their slice of the root buffers
        A1_NCCL(dev0, g_rccl.GroupStart()); group_open = true;
        for (size_t g = 1; g < G; ++g) {
            int st0 = 0, c = 0;
            shard_range(n, static_cast<int>(g), static_cast<int>(G), &st0, &c);
            if (c == 0) continue;
            a1mpc_handle h = S->h[g];
            const size_t o = st0, C = c;
            const int gi = static_cast<int>(g);
            A1_NCCL(h->device, g_rccl.Send(h->d_grf, C * 12, ncclFloat64, 0, S->comm[g], h->stream));
            A1_NCCL(dev0, g_rccl.Recv(root_grf + o * 12, C * 12, ncclFloat64, gi, S->comm[0], s0));
            if (root_it) { A1_NCCL(h->device, g_rccl.Send(h->d_iters, C, ncclInt32, 0, S->comm[g], h->stream)); A1_NCCL(dev0, g_rccl.Recv(root_it + o, C, ncclInt32, gi, S->comm[0], s0)); }
            if (root_st) { A1_NCCL(h->device, g_rccl.Send(h->d_status, C, ncclInt32, 0, S->comm[g], h->stream)); A1_NCCL(dev0, g_rccl.Recv(root_st + o, C, ncclInt32, gi, S->comm[0], s0)); }
            S->last_gather_bytes += static_cast<long long>(C * (12 * sizeof(double) + 2 * sizeof(int32_t)));
        }
        group_open = false;
        A1_NCCL(dev0, g_rccl.GroupEnd());
        // the RCCL operations ran on the handles' streams behind their solves: the handles' "last launch" events move with them
        for (size_t g = 0; g < G; ++g) { A1_SH_HIP(hipSetDevice(S->h[g]->device)); A1_SH_ST(mark_launched(S->h[g], S->h[g]->stream)); }
        A1_SH_HIP(hipSetDevice(dev0));
        if (!io.device) {
            A1_SH_HIP(hipMemcpyAsync(p_grf, S->r_grf, N * 12 * sizeof(double), hipMemcpyDeviceToHost, s0));
            A1_SH_HIP(hipMemcpyAsync(p_it, S->r_iters, N * sizeof(int32_t), hipMemcpyDeviceToHost, s0));
            A1_SH_HIP(hipMemcpyAsync(p_st, S->r_status, N * sizeof(int32_t), hipMemcpyDeviceToHost, s0));
        }
        for (size_t g = 0; g < G; ++g) { A1_SH_HIP(hipSetDevice(S->h[g]->device)); A1_SH_HIP(hipStreamSynchronize(S->h[g]->stream)); }
#undef A1_NCCL
    }
#undef A1_SH_HIP
#undef A1_SH_ST
    if (!io.device) {
        std::memcpy(io.grf, p_grf, N * 12 * sizeof(double));
        if (io.iters) std::memcpy(io.iters, p_it, N * sizeof(int32_t));
        if (io.status) std::memcpy(io.status, p_st, N * sizeof(int32_t));
    }
    return A1MPC_OK;
}

a1mpc_status a1mpc_sharded_solve_batch(a1mpc_sharded S, int32_t n, const double* x0, const double* x_ref, const double* R_world, const double* foot_abs,
                                       const uint8_t* contact, double* grf_body_out, int32_t* iters_out, int32_t* status_out) {
    ShardedIo io; io.x0 = x0; io.xref = x_ref; io.R = R_world; io.foot = foot_abs; io.contact = contact; io.grf = grf_body_out; io.iters = iters_out; io.status = status_out;
    if (!x0 || !x_ref) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return sharded_solve_impl(S, n, io);
}
a1mpc_status a1mpc_sharded_solve_batch_ticks(a1mpc_sharded S, int32_t n, const double* tick, const double* R_world, const double* foot_abs, const uint8_t* contact,
                                             double* grf_body_out, int32_t* iters_out, int32_t* status_out) {
    ShardedIo io; io.tick = tick; io.R = R_world; io.foot = foot_abs; io.contact = contact; io.grf = grf_body_out; io.iters = iters_out; io.status = status_out;
    if (!tick) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return sharded_solve_impl(S, n, io);
}
a1mpc_status a1mpc_sharded_solve_batch_device(a1mpc_sharded S, int32_t n, const double* d_x0, const double* d_x_ref, const double* d_R_world, const double* d_foot_abs,
                                              const uint8_t* d_contact, double* d_grf_body_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream) {
    ShardedIo io; io.device = true; io.x0 = d_x0; io.xref = d_x_ref; io.R = d_R_world; io.foot = d_foot_abs; io.contact = d_contact; io.grf = d_grf_body_out;
    io.iters = d_iters_out; io.status = d_status_out; io.stream = hip_stream;
    if (!d_x0 || !d_x_ref) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return sharded_solve_impl(S, n, io);
}
a1mpc_status a1mpc_sharded_solve_batch_ticks_device(a1mpc_sharded S, int32_t n, const double* d_tick, const double* d_R_world, const double* d_foot_abs,
                                                    const uint8_t* d_contact, double* d_grf_body_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream) {
    ShardedIo io; io.device = true; io.tick = d_tick; io.R = d_R_world; io.foot = d_foot_abs; io.contact = d_contact; io.grf = d_grf_body_out;
    io.iters = d_iters_out; io.status = d_status_out; io.stream = hip_stream;
    if (!d_tick) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return sharded_solve_impl(S, n, io);
}
// shard g's engine handle (warm-start I/O, a1mpc_reset_warm_start, the instrumentation calls) and the bytes the last solve moved between the root and the other shards
a1mpc_status a1mpc_sharded_handle(a1mpc_sharded S, int32_t shard, a1mpc_handle* out) {
    if (!S || !out || shard < 0 || shard >= S->ndev) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle/out or shard out of range");
    *out = S->h[shard];
    return A1MPC_OK;
}
a1mpc_status a1mpc_sharded_last_transfer(a1mpc_sharded S, int64_t* scatter_bytes, int64_t* gather_bytes) {
    if (!S) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null handle");
    if (scatter_bytes) *scatter_bytes = S->last_scatter_bytes;
    if (gather_bytes) *gather_bytes = S->last_gather_bytes;
    return A1MPC_OK;
}


// ======================================================================================================================
// Batch pipeline: `depth` engine handles on `depth` HIP streams of ONE device, batches submitted round-robin.  A launch of a few thousand QPs
// ends in a tail (its few 150-225-iteration QPs keep a handful of wavefronts busy, the rest of the chip idles); with a second batch in flight
// on another stream the hardware dispatches that batch's set-up kernel and persistent rows onto the SIMDs the tail has left.  Every slot is a
// complete handle (its own prepared-state records, queue, warm start), so batches in flight share nothing and results are bit-identical to a
// lone handle's.  One host thread per pipeline (like a handle).
struct a1mpc_pipeline_s {
    int device = 0, depth = 0, next = 0;
    std::vector<a1mpc_handle> h;
    std::vector<hipEvent_t> ready, done;   // per slot: "the caller's inputs are ready" (recorded on the caller's stream), "this slot's last submit has finished"
    std::vector<char> used;
    struct HostPending { int32_t n = 0; double *grf = nullptr, *u = nullptr; int32_t *iters = nullptr, *status = nullptr; };
    std::vector<HostPending> pending;      // per slot: a host-pointer submit whose outputs are still in the slot's pinned mirror (n = 0: none)
};
// a slot's host-pointer batch has to be handed to its caller before the slot's pinned mirror is reused
static a1mpc_status pipeline_deliver(a1mpc_pipeline p, int k) {
    a1mpc_pipeline_s::HostPending& q = p->pending[k];
    if (q.n == 0) return A1MPC_OK;
    A1_HIP(hipStreamSynchronize(p->h[k]->stream));   // (the slot's stream carries nothing but this batch; the wait a1mpc_solve_batch uses)
    host_collect(p->h[k], q.n, 12 * p->h[k]->cfg.horizon, q.grf, q.u, q.iters, q.status);
    q = a1mpc_pipeline_s::HostPending();
    return A1MPC_OK;
}

void a1mpc_pipeline_destroy(a1mpc_pipeline p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    for (int k = 0; k < static_cast<int>(p->pending.size()); ++k) (void)pipeline_deliver(p, k);   // batches still in flight reach their callers' arrays before the slots go
    for (hipEvent_t e : p->ready) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->done) if (e) (void)hipEventDestroy(e);
    for (a1mpc_handle h : p->h) a1mpc_destroy(h);
    delete p;
}

a1mpc_status a1mpc_pipeline_create(const a1mpc_config* cfg, int32_t max_batch, int32_t device, int32_t depth, a1mpc_pipeline* out) {
    if (!cfg || !out || max_batch <= 0 || device < 0 || depth < 0 || depth > 8) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null config/out, bad batch/device or depth > 8");
    *out = nullptr;
    a1mpc_pipeline p = new (std::nothrow) a1mpc_pipeline_s();
    if (!p) return fail(A1MPC_ERR_HIP, "out of host memory");
    p->device = device; p->depth = depth;
    if (depth == 0) p->depth = 2;   // default: two batches in flight.  (Round 2 took three for batches small enough for the fused kernel; with this round's kernels two win at every
                                    // size measured -- 512 / 1024 / 2048 / 4096 x h10: 0.28 / 0.30 / 0.35 / 0.61 ms per batch at depth 2, 0.35 / 0.40 / 0.43 / 0.69 at depth 3.)
    for (int k = 0; k < p->depth; ++k) {
        a1mpc_handle hk = nullptr;
        const a1mpc_status st = a1mpc_create(cfg, max_batch, device, &hk);
        if (st != A1MPC_OK) { a1mpc_pipeline_destroy(p); return st; }
        hk->pipeline_depth = p->depth;
        p->h.push_back(hk);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess) {
            if (e0) (void)hipEventDestroy(e0);
            a1mpc_pipeline_destroy(p);
            return fail(A1MPC_ERR_HIP, "hipEventCreate (pipeline)");
        }
        p->ready.push_back(e0); p->done.push_back(e1); p->used.push_back(0); p->pending.emplace_back();
    }
    *out = p;
    return A1MPC_OK;
}

a1mpc_status a1mpc_pipeline_depth(a1mpc_pipeline p, int32_t* depth_out) {
    if (!p || !depth_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline/out");
    *depth_out = p->depth;
    return A1MPC_OK;
}

a1mpc_status a1mpc_pipeline_handle(a1mpc_pipeline p, int32_t slot, a1mpc_handle* out) {
    if (!p || !out || slot < 0 || slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline/out or slot out of range");
    // A host-pointer batch still in flight on this slot keeps its results in the handle's ONE pinned mirror: any host-pointer call the caller makes on the handle
    // would overwrite them.  Hand the batch to its caller's arrays first -- the handle that leaves here carries nothing pending.
    A1_HIP(hipSetDevice(p->device));
    if (a1mpc_status sd = pipeline_deliver(p, slot); sd != A1MPC_OK) return sd;
    *out = p->h[slot];
    return A1MPC_OK;
}

a1mpc_status a1mpc_pipeline_submit_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_x0, const double* d_x_ref,
                                          const double* d_R_world, const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out,
                                          double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* inputs_ready_stream, int32_t* slot_out) {
    if (!p) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline");
    if (slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "slot out of range");
    if (!d_x0 || !d_x_ref) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    const int k = slot >= 0 ? slot : p->next;
    a1mpc_handle h = p->h[k];
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_pipeline_create");
    A1_HIP(hipSetDevice(p->device));
    if (a1mpc_status sd = pipeline_deliver(p, k); sd != A1MPC_OK) return sd;
    if (inputs_ready_stream) {   // the slot's stream starts after everything the caller has queued on that stream so far
        A1_HIP(hipEventRecord(p->ready[k], static_cast<hipStream_t>(inputs_ready_stream)));
        A1_HIP(hipStreamWaitEvent(h->stream, p->ready[k], 0));
    }
    if (fresh_batch) h->hint_n = 0;   // QPs this slot has not seen before: queue ordered by the set-up kernel's cost guess, not by the costs of the slot's previous
                                      // batch (what a1mpc_set_schedule does, without touching the handle's index-order / history setting)
    if (a1mpc_status st = solve_device_impl(h, n, nullptr, d_x0, d_x_ref, d_R_world, d_foot_abs, d_contact, d_grf_body_out, d_u_full_out, d_iters_out,
                                            d_status_out, h->stream); st != A1MPC_OK) return st;
    A1_HIP(hipEventRecord(p->done[k], h->stream));
    p->used[k] = 1;
    if (slot < 0) p->next = (p->next + 1) % p->depth;
    if (slot_out) *slot_out = k;
    return A1MPC_OK;
}

// Round 6: the general path -- per-step feet / contact schedules / its own A_c yaw (S/ConvexMpc.h:74, S/test/test_mpc.cpp:106-122) -- and the compact tick
// records (S/A1RobotControl.cpp:452-488) with two batches in flight.  A first solve of the general path is PURELY tail-bound (its queue order is unpredictable:
// profiles/r05_general_path_order.txt), which is exactly the loss a second batch in flight hides.  Same slots, same events; the solve is the lone handle's, bit for bit.
static a1mpc_status pipeline_submit_device_impl(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_tick, const double* d_x0, const double* d_x_ref,
                                                const double* d_R_world, const double* d_foot_abs, int32_t foot_stride, const uint8_t* d_contact, int32_t contact_stride,
                                                const double* d_yaw_A, double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out,
                                                void* inputs_ready_stream, int32_t* slot_out) {
    if (!p) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline");
    if (slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "slot out of range");
    if (!d_tick && (!d_x0 || !d_x_ref)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    if (!strides_ok(foot_stride, contact_stride)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    const int k = slot >= 0 ? slot : p->next;
    a1mpc_handle h = p->h[k];
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_pipeline_create");
    A1_HIP(hipSetDevice(p->device));
    if (a1mpc_status sd = pipeline_deliver(p, k); sd != A1MPC_OK) return sd;
    if (inputs_ready_stream) {   // the slot's stream starts after everything the caller has queued on that stream so far
        A1_HIP(hipEventRecord(p->ready[k], static_cast<hipStream_t>(inputs_ready_stream)));
        A1_HIP(hipStreamWaitEvent(h->stream, p->ready[k], 0));
    }
    if (fresh_batch) h->hint_n = 0;
    if (a1mpc_status st = solve_device_impl(h, n, d_tick, d_x0, d_x_ref, d_R_world, d_foot_abs, d_contact, d_grf_body_out, d_u_full_out, d_iters_out,
                                            d_status_out, h->stream, foot_stride, contact_stride, d_yaw_A); st != A1MPC_OK) return st;
    A1_HIP(hipEventRecord(p->done[k], h->stream));
    p->used[k] = 1;
    if (slot < 0) p->next = (p->next + 1) % p->depth;
    if (slot_out) *slot_out = k;
    return A1MPC_OK;
}
a1mpc_status a1mpc_pipeline_submit_strided_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_x0, const double* d_x_ref,
                                                  const double* d_R_world, const double* d_foot_abs, int32_t foot_stride, const uint8_t* d_contact,
                                                  int32_t contact_stride, const double* d_yaw_A, double* d_grf_body_out, double* d_u_full_out,
                                                  int32_t* d_iters_out, int32_t* d_status_out, void* inputs_ready_stream, int32_t* slot_out) {
    return pipeline_submit_device_impl(p, slot, fresh_batch, n, nullptr, d_x0, d_x_ref, d_R_world, d_foot_abs, foot_stride, d_contact, contact_stride, d_yaw_A, d_grf_body_out,
                                       d_u_full_out, d_iters_out, d_status_out, inputs_ready_stream, slot_out);
}
a1mpc_status a1mpc_pipeline_submit_ticks_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_tick, const double* d_R_world,
                                                const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out, double* d_u_full_out,
                                                int32_t* d_iters_out, int32_t* d_status_out, void* inputs_ready_stream, int32_t* slot_out) {
    if (!d_tick) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return pipeline_submit_device_impl(p, slot, fresh_batch, n, d_tick, nullptr, nullptr, d_R_world, d_foot_abs, 0, d_contact, 0, nullptr, d_grf_body_out,
                                       d_u_full_out, d_iters_out, d_status_out, inputs_ready_stream, slot_out);
}
// the tick-record submit with the strides let through, as a1mpc_solve_batch_ticks_strided_device is on a lone handle: (0, 0, NULL) IS a1mpc_pipeline_submit_ticks_device
a1mpc_status a1mpc_pipeline_submit_ticks_strided_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_tick, const double* d_R_world,
                                                        const double* d_foot_abs, int32_t foot_stride, const uint8_t* d_contact, int32_t contact_stride,
                                                        const double* d_yaw_A, double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out,
                                                        void* inputs_ready_stream, int32_t* slot_out) {
    if (!d_tick) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    return pipeline_submit_device_impl(p, slot, fresh_batch, n, d_tick, nullptr, nullptr, d_R_world, d_foot_abs, foot_stride, d_contact, contact_stride, d_yaw_A,
                                       d_grf_body_out, d_u_full_out, d_iters_out, d_status_out, inputs_ready_stream, slot_out);
}
// ... and host arrays in / out (what a caller on the reference's side of the boundary holds): snapshot + launches queued on the slot's stream, outputs handed over by
// a1mpc_pipeline_wait / the next submit to the slot
a1mpc_status a1mpc_pipeline_submit_strided(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                                           const double* foot_abs, int32_t foot_stride, const uint8_t* contact, int32_t contact_stride, const double* yaw_A,
                                           double* grf_body_out, double* u_full_out, int32_t* iters_out, int32_t* status_out, int32_t* slot_out) {
    if (!strides_ok(foot_stride, contact_stride)) return fail(A1MPC_ERR_INVALID_ARGUMENT, "foot_stride must be 0 or 12, contact_stride 0 or 4");
    if (foot_stride == 0 && contact_stride == 0 && !yaw_A)   // (0, 0, NULL) IS a1mpc_pipeline_submit
        return a1mpc_pipeline_submit(p, slot, fresh_batch, n, x0, x_ref, R_world, foot_abs, contact, grf_body_out, u_full_out, iters_out, status_out, slot_out);
    if (!p) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline");
    if (slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "slot out of range");
    if (n < 0 || !x0 || !x_ref || !R_world || !foot_abs || !contact || !grf_body_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    const int k = slot >= 0 ? slot : p->next;
    a1mpc_handle h = p->h[k];
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_pipeline_create");
    A1_HIP(hipSetDevice(p->device));
    if (a1mpc_status sd = pipeline_deliver(p, k); sd != A1MPC_OK) return sd;   // the slot's previous batch leaves its pinned mirror first
    if (slot_out) *slot_out = k;
    if (slot < 0) p->next = (p->next + 1) % p->depth;
    if (n == 0) return A1MPC_OK;
    if (fresh_batch) h->hint_n = 0;
    if (a1mpc_status st = strided_host_submit(h, n, x0, x_ref, R_world, foot_abs, foot_stride, contact, contact_stride, yaw_A, u_full_out != nullptr); st != A1MPC_OK) return st;
    A1_HIP(hipEventRecord(p->done[k], h->stream));
    p->used[k] = 1;
    a1mpc_pipeline_s::HostPending& q = p->pending[k];
    q.n = n; q.grf = grf_body_out; q.u = u_full_out; q.iters = iters_out; q.status = status_out;
    return A1MPC_OK;
}

// Host pointers in, host pointers out, and still more than one batch in flight (the reference's boundary is host-side: A1CtrlStates in, a 3x4 matrix
// out, S/A1RobotControl.h:44): the call snapshots the inputs into the slot's pinned block, queues H2D copy + launches + D2H copy on the slot's stream
// and returns; a1mpc_pipeline_wait() hands the results to the output arrays given here.  While the GPU solves batch k the caller's thread snapshots
// batch k + 1 and the copy engines move it.
a1mpc_status a1mpc_pipeline_submit(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* x0, const double* x_ref,
                                   const double* R_world, const double* foot_abs, const uint8_t* contact, double* grf_body_out, double* u_full_out,
                                   int32_t* iters_out, int32_t* status_out, int32_t* slot_out) {
    if (!p) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline");
    if (slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "slot out of range");
    if (n < 0 || !x0 || !x_ref || !R_world || !foot_abs || !contact || !grf_body_out) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null input/output pointer");
    const int k = slot >= 0 ? slot : p->next;
    a1mpc_handle h = p->h[k];
    if (n > h->max_batch) return fail(A1MPC_ERR_BATCH_TOO_LARGE, "n > max_batch given to a1mpc_pipeline_create");
    A1_HIP(hipSetDevice(p->device));
    if (a1mpc_status sd = pipeline_deliver(p, k); sd != A1MPC_OK) return sd;   // the slot's previous batch leaves its pinned mirror first
    if (slot_out) *slot_out = k;
    if (slot < 0) p->next = (p->next + 1) % p->depth;
    if (n == 0) return A1MPC_OK;
    if (fresh_batch) h->hint_n = 0;
    size_t armed;   // (unused: pipeline_deliver synchronises the slot's stream)
    if (a1mpc_status st = host_submit(h, n, x0, x_ref, R_world, foot_abs, contact, u_full_out != nullptr, &armed); st != A1MPC_OK) return st;
    A1_HIP(hipEventRecord(p->done[k], h->stream));
    p->used[k] = 1;
    a1mpc_pipeline_s::HostPending& q = p->pending[k];
    q.n = n; q.grf = grf_body_out; q.u = u_full_out; q.iters = iters_out; q.status = status_out;
    return A1MPC_OK;
}

a1mpc_status a1mpc_pipeline_wait(a1mpc_pipeline p, int32_t slot) {
    if (!p || slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline or slot out of range");
    A1_HIP(hipSetDevice(p->device));
    for (int k = 0; k < p->depth; ++k)
        if ((slot < 0 || slot == k) && p->used[k]) {
            A1_HIP(hipEventSynchronize(p->done[k]));
            if (a1mpc_status sd = pipeline_deliver(p, k); sd != A1MPC_OK) return sd;
        }
    return A1MPC_OK;
}

a1mpc_status a1mpc_pipeline_join(a1mpc_pipeline p, int32_t slot, void* hip_stream) {
    if (!p || slot >= p->depth) return fail(A1MPC_ERR_INVALID_ARGUMENT, "null pipeline or slot out of range");
    A1_HIP(hipSetDevice(p->device));
    for (int k = 0; k < p->depth; ++k)
        if ((slot < 0 || slot == k) && p->used[k]) A1_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), p->done[k], 0));
    return A1MPC_OK;
}

}  // extern "C"
