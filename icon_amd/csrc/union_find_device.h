// union_find_device.h - the lock-free union-find of clean_mesh.hip (over the faces) and mesh_cc.hip (over the vertices):
// parent[i] = i at the start; uf_unite hooks the larger root under the smaller by atomicCAS, so a root is the smallest index
// of its tree; uf_root reads the labels out once every union of the pass is done (a later kernel).
#pragma once

#include "common.h"

namespace icon {

// FRESH: agent-scope loads (the eight XCDs have an L2 each, and a CU's L1 is not refreshed by another CU's stores).  The first
// walk uses ordinary loads - a stale parent is still an ancestor-or-self of what it was, the walk ends at a node that WAS a
// root, and the CAS in uf_unite is the judge; after a lost CAS the walk is repeated on fresh values.
template <bool FRESH>
__device__ __forceinline__ int uf_find(int *parent, int x)
{
    while (true) {
        const int p = FRESH ? __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : parent[x];
        if (p == x) return x;
        const int gp = FRESH ? __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : parent[p];
        if (gp != p) parent[x] = gp;       // path halving: benign race, always an ancestor
        x = p;
    }
}

__device__ __forceinline__ void uf_unite(int *parent, int u, int v)
{
    u = uf_find<false>(parent, u); v = uf_find<false>(parent, v);
    while (u != v) {
        const int hi = max(u, v), lo = min(u, v);
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
        u = uf_find<true>(parent, u); v = uf_find<true>(parent, v);
    }
}

// read-only walk to the root, for a result stored out of place: a flatten that compresses in place can have its final store
// parent[i] = root overtaken by another thread's path-halving store parent[i] = grandparent
__device__ __forceinline__ int uf_root(const int *parent, int x)
{
    while (true) { const int p = parent[x]; if (p == x) return x; x = p; }
}

}  // namespace icon
