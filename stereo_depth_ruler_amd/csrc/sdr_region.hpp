// sdr_region.hpp -- the region rule, once: which queries run, which pixels of a rectangle count and
// how high each lies above the query's plane (steps 1 to 5 of "the relief of a region" in
// include/sdr/sdr.h, which the footprint takes over), and the frame of a sweep that gives a
// workgroup a slice of a rectangle's row-major order.  A kernel takes the call's maps as one
// RegionMaps (sdr_ruler_shared.hpp) and opens its query with one call: query_refusal (no map read),
// query_view (the rectangle and the maps at its origin) or query_slice (the workgroup's slice of
// it); region_pixel is the rule on a view.  The relief, the footprint, the objects, the clearance,
// the plane fit and the plane search are written on it.
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

// the rectangle of a query (sdr_relief_query, sdr_clearance_query)
template <typename Query>
__device__ __forceinline__ sdr_segment region_segment(const Query& q) {
    return sdr_segment{q.frame, q.x0, q.y0, q.x1, q.y1};
}
// a query's labels are in range and, where it needs a label map, the call has one
__device__ __forceinline__ bool labels_in_range(const sdr_relief_query& q, bool has_labels) {
    return q.label >= -1 && q.label <= 255 && (q.label < 0 || has_labels);
}
__device__ __forceinline__ bool labels_in_range(const sdr_clearance_query& q, bool has_labels) {
    return q.label_a >= 0 && q.label_a <= 255 && q.label_b >= 0 && q.label_b <= 255 && q.label_a != q.label_b &&
           has_labels;
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
template <typename Query>
__device__ __forceinline__ uint32_t query_refusal(const RegionDims& d, const sdr_plane* __restrict__ planes, int NP,
                                                  const Query& q, RegionPlane* pl) {
    if (!d.holds(region_segment(q)) || !labels_in_range(q, d.has_labels != 0)) return kRegionOutOfRange;
    return query_plane(planes, NP, q.plane, pl) ? 0 : kRegionNoPlane;
}

struct RegionPix {
    bool masked, valid, member;
    float hf;      // the height (a member's, or of a valid pixel that is not one)
    float xyz[3];  // the point (valid pixels)
};

// Pixel (u, v) of the view's rectangle: the definition's steps 1 to 5.  Every sweep of every unit
// repeats it: the same bits in every pass.
template <typename T, typename L>
__device__ __forceinline__ RegionPix region_pixel(const RegionView<T, L>& vw, const Q16& Q, const RegionPlane& pl,
                                                  float min_disp, float conf_min, int label, unsigned u, unsigned v) {
#pragma clang fp contract(off)
    const T* __restrict__ fd = vw.fd;
    const float* __restrict__ fc = vw.fc;
    const uint8_t* __restrict__ fl = vw.fl;
    const size_t stride = vw.stride;
    const int W = vw.W, xs = vw.R.xs, ys = vw.R.ys;
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

// A workgroup's slice of a view's rectangle: its area and the slice's first pixel.
template <typename T, typename L = const uint8_t>
struct RegionSlice : RegionView<T, L> {
    unsigned area, base;

    // body(u, v) for each of the slice's pixels the calling thread takes
    template <typename Body>
    __device__ __forceinline__ void each(Body&& body) const {
#pragma unroll
        for (int j = 0; j < kRegionPix; j++) {
            const unsigned p = base + (unsigned)(j * kRegionThreads + (int)threadIdx.x);
            if (p >= area) continue;
            const unsigned v = p / (unsigned)this->R.rw, u = p - v * (unsigned)this->R.rw;
            body(u, v);
        }
    }
};

// The slice blockIdx.x of a view.  False for a slice past the area (block-uniform).
template <typename T, typename L>
__device__ __forceinline__ bool region_cut(const RegionView<T, L>& vw, RegionSlice<T, L>* s) {
    static_cast<RegionView<T, L>&>(*s) = vw;
    s->area = (unsigned)vw.R.rw * (unsigned)vw.R.rh;  // <= W * H <= 2^24
    s->base = blockIdx.x * (unsigned)kRegionSlice;
    return s->base < s->area;
}

// The prologue of a kernel that applies the rule to a query's rectangle.  query_view: the
// rectangle with its frame's maps, of a query that is in range.  The other two: the refusal flag
// first (0: the query runs, *pl its plane), then the view, or the workgroup's slice of it (false: the
// query is refused or the slice is past the area; block-uniform).
template <typename T, typename Query>
__device__ __forceinline__ RegionView<T> query_view(const RegionMaps<T>& m, const Query& q) {
    return m.view(region_segment(q), m.frame_labels(q.frame));
}
template <typename T, typename Query>
__device__ __forceinline__ uint32_t query_view(const RegionMaps<T>& m, const sdr_plane* __restrict__ planes, int NP,
                                               const Query& q, RegionPlane* pl, RegionView<T>* vw) {
    const uint32_t refused = query_refusal(m.dims(), planes, NP, q, pl);
    if (!refused) *vw = query_view(m, q);
    return refused;
}
template <typename T, typename Query>
__device__ __forceinline__ bool query_slice(const RegionMaps<T>& m, const sdr_plane* __restrict__ planes, int NP,
                                            const Query& q, RegionPlane* pl, RegionSlice<T>* s) {
    return !query_refusal(m.dims(), planes, NP, q, pl) && region_cut(query_view(m, q), s);
}

}  // namespace sdr
