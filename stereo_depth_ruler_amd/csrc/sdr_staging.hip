// sdr_staging.hip -- the memory the host side hands out: grow-only device buffers, the
// stream-ordered scratch pool, page-locked blocks (sdr_host_alloc) and the staging of the
// host-pointer entry points (sdr_staging.hpp).
#include "sdr_staging.hpp"
#include "sdr_host.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

int sdr::ensure(Buf& b, size_t bytes) {
    if (b.n >= bytes && b.p) return SDR_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
    if (bytes == 0) return SDR_OK;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        const bool cap = e == hipErrorStreamCaptureUnsupported || e == hipErrorStreamCaptureInvalidated;
        return set_error(SDR_ERR_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e) +
                                            (cap ? " (scratch grows inside a graph capture: make one call of "
                                                   "this shape before capturing)" : ""));
    }
    b.n = bytes;
    return SDR_OK;
}

hipError_t sdr::scratch_alloc(void** p, size_t bytes, hipStream_t st) {
    static std::mutex mu;
    static std::map<int, hipMemPool_t> pools;
    int dev = 0;
    hipError_t e = st ? hipStreamGetDevice(st, &dev) : hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemPool_t pool = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = pools.find(dev);
        if (it == pools.end()) {
            hipMemPoolProps props = {};
            props.allocType = hipMemAllocationTypePinned;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = dev;
            e = hipMemPoolCreate(&pool, &props);
            if (e != hipSuccess) return e;
            uint64_t keep = UINT64_MAX;
            e = hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
            if (e != hipSuccess) {
                (void)hipMemPoolDestroy(pool);
                return e;
            }
            pools[dev] = pool;  // lives as long as the process
        } else {
            pool = it->second;
        }
    }
    return hipMallocFromPoolAsync(p, bytes, pool, st);
}

hipError_t sdr::scratch_free(void* p, hipStream_t st) { return hipFreeAsync(p, st); }

namespace {
constexpr size_t kXferChunk = (size_t)1 << 20;  // (256 KB and 4-16 MB chunks measured slower)
// page-locked blocks handed out by sdr_host_alloc: base -> size
std::mutex g_pin_mu;
std::map<uintptr_t, size_t> g_pinned;
// [p, p + bytes) lies inside one sdr_host_alloc block
bool is_pinned(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pinned.upper_bound((uintptr_t)p);
    if (it == g_pinned.begin()) return false;
    --it;
    return (uintptr_t)p + bytes <= it->first + it->second;
}
// 2-D copy, as one linear copy when both sides are dense
hipError_t copy2d(void* dst, size_t dp, const void* src, size_t sp, size_t rb, int rows,
                  hipMemcpyKind kind, hipStream_t st) {
    if (dp == rb && sp == rb) return hipMemcpyAsync(dst, src, rb * rows, kind, st);
    return hipMemcpy2DAsync(dst, dp, src, sp, rb, rows, kind, st);
}
}  // namespace

namespace sdr {

int HostXfer::begin(size_t bytes) {
    used = 0;
    nev = 0;
    outs.clear();
    if (bytes <= cap) return SDR_OK;
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    cap = 0;
    if (hipHostMalloc((void**)&pin, bytes, hipHostMallocDefault) != hipSuccess) {
        pin = nullptr;
        return set_error(SDR_ERR_NOMEM, "hipHostMalloc failed");
    }
    cap = bytes;
    return SDR_OK;
}

char* HostXfer::take(size_t bytes) {
    char* p = pin + used;
    used += stage_bytes(bytes);
    return p;
}

int HostXfer::event(size_t* idx) {
    if (nev == ev.size()) {
        hipEvent_t e = nullptr;
        SDR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.push_back(e);
    }
    *idx = nev++;
    return SDR_OK;
}

int HostXfer::upload(void* dst, size_t dpitch, const void* src, size_t spitch, size_t rowbytes, int rows,
                     hipStream_t st) {
    if (is_pinned(src, spitch * (rows - 1) + rowbytes)) {
        SDR_HIP(copy2d(dst, dpitch, src, spitch, rowbytes, rows, hipMemcpyHostToDevice, st));
        return SDR_OK;
    }
    char* stage = take(rowbytes * rows);
    const int step = (int)std::max<size_t>(1, kXferChunk / rowbytes);
    for (int r0 = 0; r0 < rows; r0 += step) {
        const int n = std::min(step, rows - r0);
        char* sp = stage + (size_t)r0 * rowbytes;
        const char* hp = (const char*)src + (size_t)r0 * spitch;
        if (spitch == rowbytes) std::memcpy(sp, hp, rowbytes * n);
        else
            for (int r = 0; r < n; r++) std::memcpy(sp + r * rowbytes, hp + r * spitch, rowbytes);
        SDR_HIP(copy2d((char*)dst + (size_t)r0 * dpitch, dpitch, sp, rowbytes, rowbytes, n,
                       hipMemcpyHostToDevice, st));
    }
    return SDR_OK;
}

int HostXfer::download(void* dst, size_t dpitch, const void* src, size_t spitch, size_t rowbytes, int rows,
                       hipStream_t st) {
    if (is_pinned(dst, dpitch * (rows - 1) + rowbytes)) {
        SDR_HIP(copy2d(dst, dpitch, src, spitch, rowbytes, rows, hipMemcpyDeviceToHost, st));
        size_t e = 0;
        int rc = event(&e);
        if (rc) return rc;
        SDR_HIP(hipEventRecord(ev[e], st));
        outs.push_back({nullptr, 0, 0, nullptr, 0, e});  // nothing to copy: wait only
        return SDR_OK;
    }
    char* stage = take(rowbytes * rows);
    const int step = (int)std::max<size_t>(1, kXferChunk / rowbytes);
    for (int r0 = 0; r0 < rows; r0 += step) {
        const int n = std::min(step, rows - r0);
        char* sp = stage + (size_t)r0 * rowbytes;
        SDR_HIP(copy2d(sp, rowbytes, (const char*)src + (size_t)r0 * spitch, spitch, rowbytes, n,
                       hipMemcpyDeviceToHost, st));
        size_t e = 0;
        int rc = event(&e);
        if (rc) return rc;
        SDR_HIP(hipEventRecord(ev[e], st));
        outs.push_back({(char*)dst + (size_t)r0 * dpitch, dpitch, rowbytes, sp, n, e});
    }
    return SDR_OK;
}

int HostXfer::drain() {
    for (const Out& o : outs) {
        SDR_HIP(hipEventSynchronize(ev[o.ev]));
        if (!o.dst) continue;
        if (o.dpitch == o.rowbytes) std::memcpy(o.dst, o.src, o.rowbytes * o.rows);
        else
            for (int r = 0; r < o.rows; r++) std::memcpy(o.dst + r * o.dpitch, o.src + r * o.rowbytes, o.rowbytes);
    }
    outs.clear();
    return SDR_OK;
}

void HostXfer::release() {
    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    cap = 0;
}

}  // namespace sdr

extern "C" {

int sdr_host_alloc(size_t bytes, void** out) {
    if (!out) return sdr::set_error(SDR_ERR_ARG, "null argument");
    *out = nullptr;
    if (!bytes) return sdr::set_error(SDR_ERR_ARG, "zero size");
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess)
        return sdr::set_error(SDR_ERR_NOMEM, "hipHostMalloc failed");
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pinned[(uintptr_t)p] = bytes;
    *out = p;
    return SDR_OK;
}

int sdr_host_free(void* p) {
    if (!p) return SDR_OK;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pinned.find((uintptr_t)p);
        if (it == g_pinned.end()) return sdr::set_error(SDR_ERR_ARG, "not a block from sdr_host_alloc");
        g_pinned.erase(it);
    }
    SDR_HIP(hipHostFree(p));
    return SDR_OK;
}

}  // extern "C"
