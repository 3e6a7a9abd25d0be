// sdr_layout.hpp -- the one rule by which a call lays several arrays out in one block of device
// memory: typed slices in take order, every slice 256-byte aligned.  The owner of the block
// resolves a slice to a pointer (sdr_host.hpp Scratch, sdr_ruler_shared.hpp HostCall, the voxel
// grid's arena).  Plain host arithmetic: no HIP include, so a host program can include it
// (tests/cpp/layout_check.hip).
#pragma once
#include <stddef.h>

namespace sdr {

constexpr size_t kSliceAlign = 256;  // what the block's base must be aligned to as well

// `count` elements of T at byte `off` of the block; count 0 is legal (an aligned offset, no bytes)
template <typename T>
struct Slice {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    size_t end() const { return off + bytes(); }
};

struct ScratchLayout {
    size_t total = 0;  // the block's size: the end of the last slice taken
    template <typename T>
    Slice<T> take(size_t count) {
        const Slice<T> s{(total + kSliceAlign - 1) & ~(kSliceAlign - 1), count};
        total = s.end();
        return s;
    }
};

}  // namespace sdr
