// sdr_unionfind.hpp -- the lock-free min-root union-find (Playne & Hawick 2018) the speckle filter
// (sdr_post.hip) and the object labelling (sdr_objects.hip) share: a union links the larger root
// under the smaller, so parents only ever decrease, every loop ends, and no thread waits on another.
#pragma once
#include <hip/hip_runtime.h>

namespace sdr {

__device__ __forceinline__ int uf_load(const int* P, int i) {
    return __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// find with path halving; parents only ever decrease (union links the larger root under the
// smaller), so a no-return atomicMin keeps concurrent unions intact
__device__ __forceinline__ int uf_find(int* P, int x) {
    int p = uf_load(P, x);
    while (p != x) {
        const int gp = uf_load(P, p);
        if (gp != p) atomicMin(&P[x], gp);
        x = p;
        p = gp;
    }
    return x;
}
__device__ __forceinline__ void uf_unite(int* P, int a, int b) {
    for (;;) {
        a = uf_find(P, a);
        b = uf_find(P, b);
        if (a == b) return;
        if (a < b) {
            int old = atomicMin(&P[b], a);
            if (old == b) return;
            b = old;
        } else {
            int old = atomicMin(&P[a], b);
            if (old == a) return;
            a = old;
        }
    }
}

// the same on a tile's labels in LDS (no path halving: the chains of a tile are short)
__device__ __forceinline__ int lds_find(int* lab, int x) {
    int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return x;
}
__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) {
            int old = atomicMin(&lab[b], a);
            if (old == b) return;
            b = old;
        } else {
            int old = atomicMin(&lab[a], b);
            if (old == a) return;
            a = old;
        }
    }
}

}  // namespace sdr
