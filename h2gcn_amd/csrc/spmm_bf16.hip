// spmm_bf16.hip -- the bf16-source instantiations of h2gcn::spmm_hops_kernel (TS = bf16, TD = float or bf16; see
// spmm_kernels.hip.h) and their launcher.  A translation unit of its own, like spmm_short.hip: kernels compiled in the same
// unit change the register allocation of their neighbours, and the fp32 instantiations must compile exactly as before
// (tools/kernel_resources.py).  Only the combinations the C ABI accepts exist: bf16 -> fp32 and bf16 -> bf16, forward and
// adjoint; every segment walk of the fp32 dispatch, with the same arithmetic (the canonical summation tree on the exactly
// widened elements).
#include <hip/hip_runtime.h>

#include "spmm_kernels.hip.h"

namespace h2gcn {

namespace {
template <bool SUM, typename TD>
void launch_one(const LaunchParams& p, const KernelChoice& k, dim3 grid, hipStream_t stream) {
    if (k.shortrow && k.slice == 128) launch_in_tile_short_kernels<SUM, 32, bf16, TD>(p, k.off32, k.fb4, grid, stream);
    else if (k.shortrow && k.slice == 64) launch_in_tile_short_kernels<SUM, 16, bf16, TD>(p, k.off32, k.fb4, grid, stream);
    else launch_spmm_kernels<SUM, bf16, TD>(p, k, grid, stream);
}
}  // namespace

// the caller checks hipGetLastError
void launch_bf16(bool sum, bool out_bf16, const LaunchParams& p, const KernelChoice& k, dim3 grid, hipStream_t stream) {
    if (sum) {
        if (out_bf16) launch_one<true, bf16>(p, k, grid, stream);
        else launch_one<true, float>(p, k, grid, stream);
    } else {
        if (out_bf16) launch_one<false, bf16>(p, k, grid, stream);
        else launch_one<false, float>(p, k, grid, stream);
    }
}

}  // namespace h2gcn
