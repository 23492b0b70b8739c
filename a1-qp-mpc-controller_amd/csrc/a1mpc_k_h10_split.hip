// a1mpc_k_h10_split.hip -- one translation unit of liba1mpc.so: the fast path's split pipeline at horizon 10 (set-up kernel + persistent ADMM rows)
// (kernels and launch functions: a1mpc_kernels.hpp; the entry points below are declared in a1mpc_common.hpp and called from a1mpc_hip.hip)
#include "a1mpc_kernels.hpp"

namespace a1mpc {

template a1mpc_status launch_split<10>(const KernelArgs&, double*, int*, hipStream_t, hipEvent_t);
template a1mpc_status resident_rows<10>(int*);


// the round-5 trial kernel (see a1mpc_solve_queue_kernel): h = 10, cold or warm_start = 1 batches beyond the resident rows, contacts broadcast
a1mpc_status launch_fused_queue(const KernelArgs& a, int* counter, hipStream_t stream) {
    constexpr int H = 10, ROWS = 2;
    const Kernel<KernelArgs, int*> k{&a1mpc_solve_queue_kernel<H, kModeMpc, ROWS>, {64, ROWS, lds_bytes<H>(ROWS)}};
    int dev = 0, res = 0;
    A1_HIP(hipGetDevice(&dev));
    if (a1mpc_status st = resident_workgroups(dev, select_admm_rows<H>(false, false, false), &res); st != A1MPC_OK) return st;   // (as many wavefronts as the split pipeline's rows)
    A1_HIP(hipMemsetAsync(counter, 0, sizeof(int), stream));
    if (a.cost != nullptr && a.order != nullptr) {
        if (a.predict) launch_predict_kernel(a, H, stream);
        launch_order_kernel(static_cast<int>(a.n), static_cast<const int32_t*>(a.cost), const_cast<int32_t*>(a.order), stream);
    }
    const int64_t want = workgroups_for(a.n, k.g);
    return launch_kernel(dev, k, want < res ? want : res, stream, a, counter);
}

}  // namespace a1mpc
