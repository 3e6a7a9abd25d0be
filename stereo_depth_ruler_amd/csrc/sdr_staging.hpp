// sdr_staging.hpp -- page-locked staging of the host-pointer entry points (sdr_staging.hip).
#pragma once
#include "sdr_internal.hpp"

#include <vector>

namespace sdr {

// Page-locked staging for the host-pointer entry points, kept by its owner across calls (no
// allocation per call).  Copies go through it in row chunks of about kXferChunk bytes: on the way
// in, the CPU copy of chunk i+1 overlaps the DMA of chunk i; on the way out, every chunk's DMA is
// queued behind the compute with an event, and the CPU copies chunk i out while chunk i+1 is
// still on the link.  Rows inside a block from sdr_host_alloc are copied by DMA directly.
struct HostXfer {
    char* pin = nullptr;
    size_t cap = 0, used = 0;
    std::vector<hipEvent_t> ev;
    size_t nev = 0;
    struct Out {
        char* dst;
        size_t dpitch, rowbytes;
        const char* src;  // in pin
        int rows;
        size_t ev;        // event index
    };
    std::vector<Out> outs;

    // start a call needing `bytes` of staging (the sum of stage_bytes() of its copies)
    int begin(size_t bytes);
    // host rows (src, spitch) -> device rows (dst, dpitch), enqueued on st
    int upload(void* dst, size_t dpitch, const void* src, size_t spitch, size_t rowbytes, int rows,
               hipStream_t st);
    // device rows (src, spitch) -> host rows (dst, dpitch): DMA chunks queued on st now, the
    // host copies done by drain()
    int download(void* dst, size_t dpitch, const void* src, size_t spitch, size_t rowbytes, int rows,
                 hipStream_t st);
    int drain();
    void release();

private:
    char* take(size_t bytes);
    int event(size_t* idx);
};

// staging one copy of n bytes takes
inline size_t stage_bytes(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace sdr
