// The lock-free union-find the labellings share: mesh_components.hip (a lane per index triple, over the vertices) and voxel_set.hpp (a
// lane per listed voxel, over the list: the frontier clusters of explore.hip and the class objects of objects.hip).  Hooks go towards
// the smaller index; DESIGN.md 20 argues the three invariants:
//   1. parent[v] <= v always; a word changes only from v to something smaller in the same component (the CAS of unite) or from one
//      ancestor to a smaller one (the atomicMin of find).  So every chain strictly decreases: find terminates, there are no cycles,
//      and the final root is the component's minimum.
//   2. A stale read sees v itself or a former ancestor -- still in the component, still <= v.  Nothing rests on a read being fresh,
//      only on the CAS, which executes at device scope and returns the true word.
//   3. No lane ever waits for another lane, wave or workgroup: no spin loops, locks or flags.  A failed CAS means another lane made
//      the word smaller, and the loop goes on from the value it returned; every loop is bounded by a strictly decreasing index.
#pragma once

#include "common.hpp"

namespace tsdf {

__device__ inline uint32_t parent_load(const uint32_t *parent, uint32_t v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root the chain from x ends in.  SHORTEN: every node passed whose parent has a parent is pointed at that grandparent, with
// atomicMin (the word can only get smaller, and a grandparent -- fresh or stale -- is a smaller member of the same tree).
// Bounded: x strictly decreases.
template <bool SHORTEN>
__device__ inline uint32_t components_find(uint32_t *parent, uint32_t x) {
    uint32_t p = parent_load(parent, x);
    while (p != x) {
        const uint32_t g = parent_load(parent, p);
        if (SHORTEN && g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// Bounded: a + b strictly decreases with every trip (find never goes up, and a failed CAS returns a word below hi).
__device__ inline void components_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = components_find<true>(parent, a);
        b = components_find<true>(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;   // someone else hooked hi, below itself: go on from there
        b = lo;
    }
}

}  // namespace tsdf
