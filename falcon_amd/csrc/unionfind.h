// The lock-free union-find of the connected-components steps: DBSCAN's core graph (graph.hip; per tile in LDS, tail.hip), the
// linkage components (linkage.hip) and the molecular families (families.hip).  One parent[] of int32 ids, every node its own
// parent at the start; any number of threads call uf_union concurrently; after the last union (a launch boundary or a barrier)
// every node's root is the SMALLEST id of its component, whatever the order of arrival.  Integer atomics at relaxed order only.
//
// Links only ever point to smaller ids.  A hook stores b into parent[a] only for a > b, and only by a compare-and-swap that
// expects parent[a] == a: a node is hooked once, while it is a root, so the links form a forest and every walk upwards strictly
// decreases and ends.  A halving store writes parent[parent[x]], read a moment ago, into parent[x]: a smaller node that x's
// walk passed through, and nodes never leave a component.  So whatever order the stores of different threads land in,
// parent[x] names x itself (x was never hooked) or a smaller node of x's component, and a find from x ends at the component's
// current root.
//
// The find of the FINAL pass (every node -> its root, after all unions) must not halve.  With halving, a thread that has loaded
// parent[i] and parent[parent[i]] may store that grandparent into parent[i] AFTER the row's own thread has stored the root there
// (dbscan_roots_kernel, lk_roots_kernel and tile_dbscan_kernel write roots into parent[] in the pass that finds them) --
// parent[i] then names an ancestor that is not the root and the row gets the label slot of a non-root (found by a 3,000-row chain
// in tests/test_gpu_linkage.py; shallow trees make it rare, not impossible).  Read-only finds race with nothing: whatever a
// concurrent reader sees in parent[i] (the old link or the root) is an ancestor.  Hence uf_find_final.
//
// The retry loop of uf_union ends.  Its compare-and-swap fails only when another thread has hooked the same root a in between;
// every such failure is paid for by a hook that succeeded, at most n - 1 of them can ever succeed, and the retry starts from a
// (no longer a root) and follows its new link to a smaller id.  It is the one loop here bounded by other threads' progress.
//
// Compiles two ways (netfamily.h's idiom): under hipcc for the kernels, and under a plain host compiler, where real threads
// race the same function bodies under ThreadSanitizer (tests/hostbuild_unionfind.py).  Only the three primitives differ.
#pragma once
#ifdef __HIPCC__
#include "common.h"
#else                        // plain host compiler: the qualifiers mean nothing there
#include <stdint.h>
#ifndef __host__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#endif

namespace fal {

// the scope of the relaxed atomic loads and stores: where parent[] lives and who shares it
#ifdef __HIPCC__
constexpr int kUfAgent = __HIP_MEMORY_SCOPE_AGENT;               // global memory, every workgroup of the launch
constexpr int kUfWorkgroup = __HIP_MEMORY_SCOPE_WORKGROUP;       // a tile's parent[] in LDS
#else
constexpr int kUfAgent = 1, kUfWorkgroup = 2;                    // (one kind of atomic on the host)
#endif
constexpr int kUfPlainLoads = -1;      // uf_find_final only: plain loads, for a launch in which nothing writes parent[]

template <int Scope>
__device__ __forceinline__ int32_t uf_load(const int32_t* p) {
    if constexpr (Scope == kUfPlainLoads) return *p;
#ifdef __HIPCC__
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, Scope);
#else
    else return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

template <int Scope>
__device__ __forceinline__ void uf_store(int32_t* p, int32_t v) {
#ifdef __HIPCC__
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, Scope);
#else
    __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}

// -> the value found in *p (== expect: the swap took place)
__device__ __forceinline__ int32_t uf_cas(int32_t* p, int32_t expect, int32_t want) {
#ifdef __HIPCC__
    return atomicCAS(p, expect, want);
#else
    __atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;
#endif
}

// path halving: every node passed is pointed at its grandparent
template <int Scope>
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t p = uf_load<Scope>(&parent[x]);
    while (p != x) {
        const int32_t g = uf_load<Scope>(&parent[p]);
        if (g != p) uf_store<Scope>(&parent[x], g);
        x = p;
        p = g;
    }
    return x;
}

// the read-only walk to the root, for the pass behind the last union.  Loads = kUfAgent / kUfWorkgroup where that pass stores
// its roots into parent[] as it goes, kUfPlainLoads where nothing writes parent[] while it runs
template <int Loads>
__device__ __forceinline__ int32_t uf_find_final(const int32_t* parent, int32_t x) {
    int32_t p = uf_load<Loads>(&parent[x]);
    while (p != x) {
        x = p;
        p = uf_load<Loads>(&parent[x]);
    }
    return x;
}

// hook the larger root under the smaller one
template <int Scope>
__device__ __forceinline__ void uf_union(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = uf_find<Scope>(parent, a);
        b = uf_find<Scope>(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }     // a > b
        if (uf_cas(&parent[a], a, b) == a) return;
    }
}

}  // namespace fal
