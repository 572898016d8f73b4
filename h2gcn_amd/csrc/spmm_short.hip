// spmm_short.hip -- the in-tile short-row instantiations of h2gcn::spmm_hops_kernel (SHORT = true; see spmm_kernels.hip.h) for
// fp32 operands: explicit instantiations of launch_in_tile_short_rows, which h2gcn_capi.hip declares `extern template`.  A
// translation unit of its own on purpose: compiled in the same unit as the tile-walk kernels, their presence makes the compiler
// allocate 2-6 more VGPRs to THOSE kernels and pushes several of them into scratch (tools/kernel_resources.py; round 3 shipped
// that way).  Nothing else lives here.
#include <hip/hip_runtime.h>

#include "spmm_kernels.hip.h"

namespace h2gcn {

template void launch_in_tile_short_rows<32, false, float, float>(const LaunchParams&, const Schedule&, dim3, hipStream_t);
template void launch_in_tile_short_rows<16, false, float, float>(const LaunchParams&, const Schedule&, dim3, hipStream_t);
template void launch_in_tile_short_rows<32, true, float, float>(const LaunchParams&, const Schedule&, dim3, hipStream_t);
template void launch_in_tile_short_rows<16, true, float, float>(const LaunchParams&, const Schedule&, dim3, hipStream_t);

}  // namespace h2gcn
