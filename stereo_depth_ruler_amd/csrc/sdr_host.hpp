// sdr_host.hpp -- what the host side of every unit shares: the one hipError_t check and the
// size checks of the C entries.
#pragma once
#include "sdr_internal.hpp"

#include <string>

// Returns SDR_ERR_DEVICE from the enclosing function, with the call's own text and HIP's message
// as sdr_last_error(), when a HIP call fails.
#define SDR_HIP(call)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return sdr::set_error(SDR_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace sdr {

inline int check_dims(int W, int H, size_t stride, int F) {
    if (W <= 0 || H <= 0 || F <= 0) return set_error(SDR_ERR_ARG, "non-positive size");
    if (stride < (size_t)W) return set_error(SDR_ERR_ARG, "stride < width");
    return SDR_OK;
}

}  // namespace sdr
