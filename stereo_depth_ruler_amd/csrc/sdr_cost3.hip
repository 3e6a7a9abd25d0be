// sdr_cost3.hip -- the cost-volume kernel for 3-channel input (calcPixelCostBT's cn == 3 branch:
// each channel's Sobel and raw BT costs are summed into the pixel cost).  The kernel template is
// sdr_cost_kernel.hpp; this file holds its CN = 3 instantiations for D <= 128 (K = 1) and the
// dispatch; sdr_cost3k2.hip the D > 128 ones (two translation units that compile in parallel).
#include "sdr_cost_kernel.hpp"

namespace sdr {

CostBands launch_cost_cn3_k2(const Geometry& g, const CostArgs& a, const CostChoice& c, int F, hipStream_t st);

// No blockSize 11: check_channels refuses it for three channels at every preFilterCap and P2 (the
// block term alone, 3 * 93 * 121, passes the int16 cost range), so the plan never names it.
CostBands launch_cost_cn3(const Geometry& g, const CostArgs& a, const CostChoice& c, int F, hipStream_t st) {
    if (c.k == 2) return launch_cost_cn3_k2(g, a, c, F, st);
    switch (c.nr) {
        case 1: return launch_cost_t<1, 1, 3>(g, a, F, st);
        case 3: return launch_cost_t<3, 1, 3>(g, a, F, st);
        case 5: return launch_cost_t<5, 1, 3>(g, a, F, st);
        case 7: return launch_cost_t<7, 1, 3>(g, a, F, st);
        case 9: return launch_cost_t<9, 1, 3>(g, a, F, st);
        default: return kNoCostKernel;
    }
}

}  // namespace sdr
