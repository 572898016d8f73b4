// spmm_bf16.hip -- the bf16-source instantiations of h2gcn::spmm_hops_kernel (TS = bf16, TD = float or bf16; see
// spmm_kernels.hip.h): explicit instantiations of launch_spmm, which h2gcn_capi.hip declares `extern template`.  A translation
// unit of its own, like spmm_short.hip: kernels compiled in the same unit change the register allocation of their neighbours,
// and the fp32 instantiations must compile exactly as before (tools/kernel_resources.py).  Only the combinations the C ABI
// accepts exist: bf16 -> fp32 and bf16 -> bf16, forward and adjoint; every segment walk of the fp32 dispatch, with the same
// arithmetic (the canonical summation tree on the exactly widened elements).
#include <hip/hip_runtime.h>

#include "spmm_kernels.hip.h"

namespace h2gcn {

template void launch_spmm<false, bf16, float>(const LaunchParams&, const Schedule&, dim3, hipStream_t);
template void launch_spmm<false, bf16, bf16>(const LaunchParams&, const Schedule&, dim3, hipStream_t);
template void launch_spmm<true, bf16, float>(const LaunchParams&, const Schedule&, dim3, hipStream_t);
template void launch_spmm<true, bf16, bf16>(const LaunchParams&, const Schedule&, dim3, hipStream_t);

}  // namespace h2gcn
