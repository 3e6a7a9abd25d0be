// sdr_host.hpp -- what the host side of every unit shares: the one hipError_t check, the size
// checks of the C entries, the release of device buffers, the device and stream binding of the
// auxiliary handles (Bound), the per-thread state of the host-pointer entries (ThreadState) and the
// owner of a device call's stream-ordered scratch (Scratch).
#pragma once
#include "sdr_internal.hpp"
#include "sdr_layout.hpp"

#include <initializer_list>
#include <string>
#include <vector>

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

// frees the buffers' device memory (on the current device) and leaves them empty
inline void free_bufs(std::initializer_list<Buf*> bufs) {
    for (Buf* b : bufs) {
        if (b->p) (void)hipFree(b->p);
        *b = Buf();
    }
}

// The device and stream binding of a handle that owns device buffers (sdr_rectifier, sdr_display,
// sdr_wls embed it; the matcher's persistent / transient binding is sdr_handle.hpp's).  The handle
// names its Bufs once, where it is declared; close() frees exactly those.
struct Bound {
    int device = 0;
    hipStream_t stream = nullptr;      // the bound stream: own_stream, or the caller's
    hipStream_t own_stream = nullptr;  // non-blocking, created by open()
    std::vector<Buf*> bufs;
    Bound(std::initializer_list<Buf*> owned) : bufs(owned) {}
    Bound(const Bound&) = delete;
    Bound& operator=(const Bound&) = delete;

    // makes `device` current and binds a new stream of it; a failed open() needs no close()
    int open(int dev) {
        int ndev = 0;
        SDR_HIP(hipGetDeviceCount(&ndev));
        if (dev < 0 || dev >= ndev) return set_error(SDR_ERR_DEVICE, "invalid device index");
        SDR_HIP(hipSetDevice(dev));
        if (hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking) != hipSuccess)
            return set_error(SDR_ERR_DEVICE, "hipStreamCreate failed");
        device = dev;
        stream = own_stream;
        return SDR_OK;
    }
    // waits for the bound stream's work, then frees the buffers and the own stream
    void close() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (Buf* b : bufs) free_bufs({b});
        if (own_stream) (void)hipStreamDestroy(own_stream);
        stream = own_stream = nullptr;
    }
    void bind(void* s) { stream = (hipStream_t)s; }  // NULL = the HIP null (legacy default) stream
    void unbind() { stream = own_stream; }
};

// The per-thread state of the host-pointer entries that take no handle: one stream and one set of
// grow-only device resources a thread, of the thread's current device; released and rebuilt when
// the current device has changed since the last call, released at thread exit.  Res names the
// resources and frees them in Res::release() (the stream is still alive and idle then).
template <typename Res>
struct ThreadState : Res {
    int device = -1;  // -1: nothing is held
    hipStream_t st = nullptr;
    ~ThreadState() { release(); }

    void release() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        Res::release();
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
        device = -1;
    }
    // the state of the current device (which stays current)
    int acquire() {
        int dev = 0;
        SDR_HIP(hipGetDevice(&dev));
        if (device == dev) return SDR_OK;
        release();
        SDR_HIP(hipSetDevice(dev));
        SDR_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        device = dev;
        return SDR_OK;
    }
};

// The stream-ordered scratch of one call on one stream: one block of the library's pool
// (scratch_alloc), laid out by a ScratchLayout.  An entry opens it, resolves its slices, launches and
// returns finish(); a return before that frees the block in the destructor.
struct Scratch {
    hipStream_t st;
    char* base = nullptr;  // non-null: a block is open
    explicit Scratch(hipStream_t s) : st(s) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (base) (void)scratch_free(base, st);
    }

    int open(const ScratchLayout& layout) {
        SDR_HIP(scratch_alloc((void**)&base, layout.total, st));
        // the layout aligns offsets; the slices are aligned only on a base that is
        if ((uintptr_t)base % kSliceAlign) return set_error(SDR_ERR_DEVICE, "scratch block is not 256-byte aligned");
        return SDR_OK;
    }
    template <typename T>
    T* at(const Slice<T>& s) const {
        return (T*)(base + s.off);
    }
    // after the call's last launch: frees the block (if one is open) on the stream and reports the
    // first failure of the free, of `e` (an earlier HIP call of the entry) and of the launches
    int finish(hipError_t e = hipSuccess) {
        const hipError_t le = hipGetLastError();
        char* block = base;
        base = nullptr;
        if (block) SDR_HIP(scratch_free(block, st));
        SDR_HIP(e);
        SDR_HIP(le);
        return SDR_OK;
    }
};

}  // namespace sdr
