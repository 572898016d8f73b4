// spmm_short.hip -- the in-tile short-row instantiations of h2gcn::spmm_hops_kernel (SHORT = true; see spmm_kernels.hip.h)
// (fp32 operands) and their launcher.  A translation unit of its own on purpose: compiled in the same unit as the tile-walk kernels, their
// presence makes the compiler allocate 2-6 more VGPRs to THOSE kernels and pushes several of them into scratch
// (tools/kernel_resources.py; round 3 shipped that way).  Nothing else lives here.
#include <hip/hip_runtime.h>

#include "spmm_kernels.hip.h"

namespace h2gcn {

// slice: 64 (4 lane groups per wave) or 128 (2) feature columns; the caller checks hipGetLastError
void launch_in_tile_short(bool sum, const LaunchParams& p, int slice, bool off32, bool fb4, dim3 grid, hipStream_t stream) {
    if (sum) {
        if (slice == 128) launch_in_tile_short_kernels<true, 32, float, float>(p, off32, fb4, grid, stream);
        else launch_in_tile_short_kernels<true, 16, float, float>(p, off32, fb4, grid, stream);
    } else {
        if (slice == 128) launch_in_tile_short_kernels<false, 32, float, float>(p, off32, fb4, grid, stream);
        else launch_in_tile_short_kernels<false, 16, float, float>(p, off32, fb4, grid, stream);
    }
}

}  // namespace h2gcn
