// Lock-free union-find over int indices in global memory, shared by the DBSCAN clusters (preprocess.hip) and the connected-component
// labelling (metrics.hip).  parent[x] <= x always and a parent only ever DECREASES: hooking is a compare-and-swap on a root (the
// larger root goes under the smaller), paths are shortened with atomicMin.  So there are no cycles whatever the schedule, every
// walk ends, no thread waits for another one's progress, and once all unions of a launch are done the root of a tree is its
// SMALLEST index.
#pragma once
#include "common.h"

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; parents only ever decrease, so every value read is an ancestor of x and the walk ends at a (then) root
__device__ __forceinline__ int uf_find(int* parent, int x)
{
    int p = uf_load(parent + x);
    while (p != x) {
        const int gp = uf_load(parent + p);
        if (gp != p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

// joins the trees of a and b, the larger root under the smaller; returns the common root
__device__ __forceinline__ int uf_union(int* parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(parent + a, a, b) == a) return b;
    }
}
