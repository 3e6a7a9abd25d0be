// sdr_region.hpp -- the region rule, once: which queries run, which pixels of a rectangle count and
// how high each lies above the query's plane (steps 1 to 5 of "the relief of a region" in
// include/sdr/sdr.h, which the footprint takes over), and the frame of a sweep that gives a
// workgroup a slice of a rectangle's row-major order.  The relief, the footprint, the objects, the
// clearance, the plane fit and the plane search are written on it.
#pragma once
#include "sdr_ruler_shared.hpp"

namespace sdr {

// A region is cut into slices of kRegionSlice pixels of its row-major order, a workgroup a slice.
// The sweeps sum integers, count and take extremes only: neither the slice size nor the order the
// workgroups finish in shows in a result.
constexpr int kRegionThreads = 256;
constexpr int kRegionWaves = kRegionThreads / 64;
constexpr int kRegionPix = 8;  // pixels a thread
constexpr int kRegionSlice = kRegionThreads * kRegionPix;

inline unsigned region_slices(int W, int H) {
    return (unsigned)(((size_t)W * H + kRegionSlice - 1) / kRegionSlice);
}

__device__ __forceinline__ sdr_segment region_segment(const sdr_relief_query& q) {
    return sdr_segment{q.frame, q.x0, q.y0, q.x1, q.y1};
}

struct RegionPlane {
    double n[3], off;
};

// the plane a query names: false when the index is out of range or the record is not a plane
__device__ __forceinline__ bool query_plane(const sdr_plane* __restrict__ planes, int NP, int index, RegionPlane* pl) {
    if (index < 0 || index >= NP) return false;
    const sdr_plane* p = planes + index;
    if (!(p->flags & SDR_PLANE_OK)) return false;
    pl->n[0] = p->normal[0];
    pl->n[1] = p->normal[1];
    pl->n[2] = p->normal[2];
    pl->off = p->offset;
    return true;
}

// one refusal for the five record types
static_assert(SDR_RELIEF_OUT_OF_RANGE == 2 && SDR_FOOTPRINT_OUT_OF_RANGE == 2 && SDR_PDIST_OUT_OF_RANGE == 2 &&
                  SDR_OBJECTS_OUT_OF_RANGE == 2 && SDR_CLEARANCE_OUT_OF_RANGE == 2,
              "the OUT_OF_RANGE flags share a value");
static_assert(SDR_RELIEF_NO_PLANE == 4 && SDR_FOOTPRINT_NO_PLANE == 4 && SDR_PDIST_NO_PLANE == 4 &&
                  SDR_OBJECTS_NO_PLANE == 4 && SDR_CLEARANCE_NO_PLANE == 4,
              "the NO_PLANE flags share a value");
constexpr uint32_t kRegionOutOfRange = 2, kRegionNoPlane = 4;

// 0, or the flag that refuses the query without a read of the maps; the plane of one that runs
__device__ __forceinline__ uint32_t region_refusal(const sdr_relief_query& q, int W, int H, int F, bool has_labels,
                                                   const sdr_plane* __restrict__ planes, int NP, RegionPlane* pl) {
    if (!segment_in_range(region_segment(q), W, H, F) || q.label < -1 || q.label > 255 ||
        (q.label >= 0 && !has_labels))
        return kRegionOutOfRange;
    return query_plane(planes, NP, q.plane, pl) ? 0 : kRegionNoPlane;
}

struct RegionPix {
    bool masked, valid, member;
    float hf;      // the height (a member's, or of a valid pixel that is not one)
    float xyz[3];  // the point (valid pixels)
};

// Pixel (u, v) of the region whose origin (xs, ys) fd, fc and fl point at: the definition's steps
// 1 to 5.  Every sweep of every unit repeats it: the same bits in every pass.
template <typename T>
__device__ __forceinline__ RegionPix region_pixel(const T* __restrict__ fd, size_t stride,
                                                  const float* __restrict__ fc, const uint8_t* __restrict__ fl,
                                                  int W, const Q16& Q, const RegionPlane& pl, float min_disp,
                                                  float conf_min, int label, int xs, int ys, unsigned u, unsigned v) {
#pragma clang fp contract(off)
    RegionPix r = {false, false, false, 0.f, {0.f, 0.f, 0.f}};
    r.masked = label < 0 || fl[(size_t)v * W + u] == (uint8_t)label;
    if (!r.masked) return r;
    const float d = load_disp(fd + (size_t)v * stride + u);
    const float c = fc ? fc[(size_t)v * W + u] : 0.f;
    r.valid = isfinite(d) && d > min_disp && (!fc || c >= conf_min);  // a NaN confidence fails
    if (!r.valid) return r;
    reproject_px(Q, xs + (int)u, ys + (int)v, (double)d, 0.0, 0, r.xyz);
    const double h = ((pl.n[0] * (double)r.xyz[0] + pl.n[1] * (double)r.xyz[1]) + pl.n[2] * (double)r.xyz[2]) + pl.off;
    r.hf = (float)h + 0.0f;
    r.member = finite3(r.xyz) && fabsf(r.hf) < 1048576.0f;
    return r;
}

// A workgroup's slice of a rectangle: the rectangle, its area, the slice's first pixel, and the
// disparity, confidence and label maps at the rectangle's origin (L: const uint8_t, or uint8_t for
// the sweep that writes labels).
template <typename T, typename L>
struct RegionSlice {
    PlaneRect R;
    unsigned area, base;
    const T* fd;
    const float* fc;
    L* fl;

    // body(u, v) for each of the slice's pixels the calling thread takes
    template <typename Body>
    __device__ __forceinline__ void each(Body&& body) const {
#pragma unroll
        for (int j = 0; j < kRegionPix; j++) {
            const unsigned p = base + (unsigned)(j * kRegionThreads + (int)threadIdx.x);
            if (p >= area) continue;
            const unsigned v = p / (unsigned)R.rw, u = p - v * (unsigned)R.rw;
            body(u, v);
        }
    }
};

// The slice blockIdx.x of the rectangle sg (in range) of frame sg.frame; conf: all frames' maps or
// null; labels: the frame's map or null.  False for a slice past the area (block-uniform).
template <typename T, typename L>
__device__ __forceinline__ bool region_slice(const sdr_segment& sg, const T* __restrict__ disp, size_t stride,
                                             size_t fstride, int W, int H, const float* __restrict__ conf, L* labels,
                                             RegionSlice<T, L>* s) {
    s->R = plane_rect(sg);
    s->area = (unsigned)s->R.rw * (unsigned)s->R.rh;  // <= W * H <= 2^24
    s->base = blockIdx.x * (unsigned)kRegionSlice;
    if (s->base >= s->area) return false;
    const size_t org = (size_t)s->R.ys * W + (size_t)s->R.xs;
    s->fd = disp + (size_t)sg.frame * fstride + (size_t)s->R.ys * stride + (size_t)s->R.xs;
    s->fc = conf ? conf + (size_t)sg.frame * H * W + org : nullptr;
    s->fl = labels ? labels + org : nullptr;
    return true;
}

}  // namespace sdr
