// sdr_cost3k2.hip -- CN = 3 cost-volume instantiations for D > 128 (two disparity pairs per lane);
// see sdr_cost3.hip.
#include "sdr_cost_kernel.hpp"

namespace sdr {

CostBands launch_cost_cn3_k2(const Geometry& g, const CostArgs& a, const CostChoice& c, int F, hipStream_t st) {
    switch (c.nr) {
        case 1: return launch_cost_t<1, 2, 3>(g, a, F, st);
        case 3: return launch_cost_t<3, 2, 3>(g, a, F, st);
        case 5: return launch_cost_t<5, 2, 3>(g, a, F, st);
        case 7: return launch_cost_t<7, 2, 3>(g, a, F, st);
        case 9: return launch_cost_t<9, 2, 3>(g, a, F, st);
        default: return kNoCostKernel;  // blockSize 11: refused by the plan (sdr_cost3.hip)
    }
}

}  // namespace sdr
