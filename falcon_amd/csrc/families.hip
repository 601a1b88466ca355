// Molecular families of the representative network (fal_network_families; DESIGN.md "Molecular families"; netfamily.h holds the
// pure core and the rule).
//
// A pass computes the components of the alive edges from scratch: every node its own parent; one thread per alive edge hooks the
// larger root under the smaller with a compare-and-swap (a component's root is its smallest node); a read-only find gives every
// node its root and counts the root's nodes; one thread per alive edge of a component above the cap lowers lo[root] to the
// edge's key with an unsigned atomicMin and raises the pass's `over` word; one thread per such edge then compares its sim with
// lo[root] and marks the round.  The lo and cut kernels are enqueued before the host knows whether a component is above the cap:
// without one they touch nothing.  Integer atomics only (compare-and-swap, add, min): minima and counts do not depend on the
// order of arrival, and which of two roots a hook finds first changes the tree, not the root.
//
// Synchronisations: one per pass for the `over` word (the first also brings the error word of the edge check) -- a call of R
// cutting rounds makes R + 1 passes -- plus one for the family and cut counts.  Nothing is written to the caller's arrays
// before the last pass: the rounds live in scratch.
#include "common.h"
#include "ivf.h"
#include "netfamily.h"
#include "unionfind.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kFamBlock = 256;
enum { FAM_ERR = 0, FAM_OVER = 1 };          // int32 words of the misc block; the cut count is the unsigned long long at byte 8

// every edge alive (0), or never alive (-1) and the error word raised: no kernel behind this one follows an invalid endpoint
__global__ void fam_check_kernel(const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, const float* __restrict__ es, int64_t m,
                                 int64_t n, int32_t* __restrict__ round, int32_t* __restrict__ misc) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const bool ok = fam_valid_edge(eu[e], ev[e], es[e], n);
        if (!ok) misc[FAM_ERR] = 1;                                          // (every writer stores the same 1)
        round[e] = ok ? 0 : -1;
    }
}

__global__ void fam_init_kernel(int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ size, uint32_t* __restrict__ lo) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        parent[i] = (int32_t)i;
        size[i] = 0;
        lo[i] = kFamNoKey;
    }
}

// unionfind.h's union-find: path halving while the hooks run ...  (The loop is uf_union's, left written out: called as
// uf_union<kUfAgent>(parent, eu[e], ev[e]) the kernel compiles to the same 139 instructions and registers in another block order,
// and a kernel whose listing moves is not kept without a measurement -- profiles/NOTES.md, "One union-find header".)
__global__ void fam_hook_kernel(const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, const int32_t* __restrict__ round,
                                int64_t m, int32_t* __restrict__ parent) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        if (round[e] != 0) continue;
        int32_t a = eu[e], b = ev[e];
        while (true) {                                                        // uf_union's loop, written out (see above)
            a = uf_find<kUfAgent>(parent, a);
            b = uf_find<kUfAgent>(parent, b);
            if (a == b) break;
            if (a < b) { const int32_t t = a; a = b; b = t; }
            if (uf_cas(&parent[a], a, b) == a) break;
        }
    }
}

// ... and none in the find behind the last hook (unionfind.h, uf_find_final).  That find runs in a launch of its own behind the
// hook kernel's: nothing writes `parent` while it runs, so plain loads do (the root passes of graph.hip and linkage.hip share
// their launch with stores and load atomically -- another instruction form).
// root[i] = the smallest node of i's component; size[root] = its nodes.  parent is read only: the roots go to their own array
__global__ void fam_find_kernel(const int32_t* __restrict__ parent, int64_t n, int32_t* __restrict__ root, int32_t* __restrict__ size) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = uf_find_final<kUfPlainLoads>(parent, (int32_t)i);
        root[i] = r;
        atomicAdd(&size[r], 1);
    }
}

__global__ void fam_lo_kernel(const int32_t* __restrict__ eu, const float* __restrict__ es, const int32_t* __restrict__ round, int64_t m,
                              const int32_t* __restrict__ root, const int32_t* __restrict__ size, int32_t max_size,
                              uint32_t* __restrict__ lo, int32_t* __restrict__ misc) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        if (round[e] != 0) continue;
        const int32_t r = root[eu[e]];
        if (!fam_oversized(size[r], max_size)) continue;
        atomicMin(&lo[r], fam_key(es[e]));
        misc[FAM_OVER] = 1;                                                  // (every writer stores the same 1)
    }
}

__global__ void fam_cut_kernel(const int32_t* __restrict__ eu, const float* __restrict__ es, int32_t* __restrict__ round, int64_t m,
                               const int32_t* __restrict__ root, const int32_t* __restrict__ size, int32_t max_size,
                               const uint32_t* __restrict__ lo, double delta, int32_t r_next) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        if (round[e] != 0) continue;
        const int32_t r = root[eu[e]];
        if (fam_oversized(size[r], max_size) && fam_is_cut(es[e], lo[r], delta)) round[e] = r_next;
    }
}

__global__ void fam_flag_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, int64_t n, int32_t* __restrict__ flag) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        flag[i] = root[i] == (int32_t)i && fam_is_family(size[i]);
}

// rank[r] = the families with a root below r
__global__ void fam_number_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ size, const int64_t* __restrict__ rank,
                                  int64_t n, int32_t* __restrict__ node_family, int32_t* __restrict__ node_size) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = root[i], s = size[r];
        node_family[i] = fam_is_family(s) ? (int32_t)rank[r] : -1;
        node_size[i] = s;
    }
}

// the rounds into the caller's array, and the edges cut (one atomic per wave; whole waves: every lane reaches the ballot)
__global__ __launch_bounds__(kFamBlock) void fam_rounds_kernel(const int32_t* __restrict__ round, int64_t m, int32_t* __restrict__ edge_round,
                                                               unsigned long long* __restrict__ n_cut) {
    for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < m; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = base + threadIdx.x;
        const int32_t r = e < m ? round[e] : 0;
        if (e < m) edge_round[e] = r;
        const unsigned long long mask = __ballot(r > 0);
        if (mask != 0 && (threadIdx.x & 63) == 0) atomicAdd(n_cut, (unsigned long long)__popcll(mask));
    }
}

}  // namespace
}  // namespace fal
FAL_WARM_KERNEL(fal::fam_hook_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_network_families(fal_ctx* ctx, const int32_t* edge_u, const int32_t* edge_v, const float* edge_sim, int64_t m, int64_t n,
                                    int max_size, double delta, int32_t* node_family, int32_t* node_size, int32_t* edge_round,
                                    int64_t* n_families, int64_t* n_rounds) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_families && n_rounds && n >= 0 && n < (int64_t)INT32_MAX && m >= 0, FAL_EINVAL,
                "fal_network_families: bad argument");
    FAL_REQUIRE(max_size >= 0, FAL_EINVAL, "fal_network_families: max_size %d is negative", max_size);
    FAL_REQUIRE(delta >= 0.0, FAL_EINVAL, "fal_network_families: delta %g is negative or not a number", delta);
    FAL_REQUIRE(n > 0 || m == 0, FAL_EINVAL, "fal_network_families: %lld edges between no nodes", (long long)m);
    FAL_REQUIRE(m == 0 || (edge_u && edge_v && edge_sim && edge_round), FAL_EINVAL, "fal_network_families: NULL edge array");
    FAL_REQUIRE(n == 0 || (node_family && node_size), FAL_EINVAL, "fal_network_families: NULL node array");
    ctx->counters[13] = 0;
    if (n == 0) {
        *n_families = *n_rounds = 0;
        return FAL_OK;
    }
    hipStream_t st = ctx->stream;
    fal::ScratchLayout L;
    const auto misc = L.array<int32_t>(16);             // 64 B of meta words; the 64-bit cut lives in words 2 and 3
    const auto rank = L.array<int64_t>(n + 1);
    const auto parent = L.array<int32_t>(n), root = L.array<int32_t>(n), size = L.array<int32_t>(n), flag = L.array<int32_t>(n);
    const auto lo = L.array<uint32_t>(n);
    const auto round = L.array<int32_t>(m);
    FAL_TRY(L.reserve(ctx, SLOT_FAM));
    unsigned long long* d_cut = reinterpret_cast<unsigned long long*>(misc + 2);
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    int32_t* h_misc = reinterpret_cast<int32_t*>(pin);
    unsigned long long* h_cut = reinterpret_cast<unsigned long long*>(pin + 8);
    int64_t* h_fam = reinterpret_cast<int64_t*>(pin + 16);
    const unsigned ngrid = capped_grid(ctx, n, kFamBlock), egrid = capped_grid(ctx, m, kFamBlock);
    FAL_CHECK_HIP(hipMemsetAsync(misc, 0, 64, st));
    if (m > 0) hipLaunchKernelGGL(fam_check_kernel, dim3(egrid), dim3(kFamBlock), 0, st, edge_u, edge_v, edge_sim, m, n, round, misc);
    int64_t rounds = 0;
    for (;;) {
        hipLaunchKernelGGL(fam_init_kernel, dim3(ngrid), dim3(kFamBlock), 0, st, n, parent, size, lo);
        if (m > 0) hipLaunchKernelGGL(fam_hook_kernel, dim3(egrid), dim3(kFamBlock), 0, st, edge_u, edge_v, round, m, parent);
        hipLaunchKernelGGL(fam_find_kernel, dim3(ngrid), dim3(kFamBlock), 0, st, parent, n, root, size);
        if (m > 0 && max_size > 0) {
            hipLaunchKernelGGL(fam_lo_kernel, dim3(egrid), dim3(kFamBlock), 0, st, edge_u, edge_sim, round, m, root, size,
                               (int32_t)max_size, lo, misc);
            hipLaunchKernelGGL(fam_cut_kernel, dim3(egrid), dim3(kFamBlock), 0, st, edge_u, edge_sim, round, m, root, size,
                               (int32_t)max_size, lo, delta, (int32_t)(rounds + 1));
        }
        FAL_CHECK_HIP(hipGetLastError());
        // the pass's wait: is a component above the cap (then the cut kernel has marked round rounds + 1); the first pass's also
        // brings the error word
        FAL_CHECK_HIP(hipMemcpyAsync(h_misc, misc, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FAL_CHECK_HIP(hipStreamSynchronize(st));
        FAL_REQUIRE(h_misc[FAM_ERR] == 0, FAL_EINVAL,
                    "fal_network_families: an edge with an end outside the %lld nodes, with both ends the same, or with a sim that is "
                    "negative or not finite", (long long)n);
        if (h_misc[FAM_OVER] == 0) break;
        rounds += 1;
        FAL_REQUIRE(rounds < (int64_t)INT32_MAX, FAL_EINTERNAL, "fal_network_families: the rounds did not end");
        FAL_CHECK_HIP(hipMemsetAsync(misc + FAM_OVER, 0, sizeof(int32_t), st));
    }
    // root / size hold the components of the surviving edges (the last pass cut nothing)
    hipLaunchKernelGGL(fam_flag_kernel, dim3(ngrid), dim3(kFamBlock), 0, st, root, size, n, flag);
    FAL_CHECK_HIP(hipGetLastError());
    FAL_TRY(device_scan_i32(ctx, flag, n, rank, SLOT_FAM2));
    hipLaunchKernelGGL(fam_number_kernel, dim3(ngrid), dim3(kFamBlock), 0, st, root, size, rank, n, node_family, node_size);
    if (m > 0) hipLaunchKernelGGL(fam_rounds_kernel, dim3(egrid), dim3(kFamBlock), 0, st, round, m, edge_round, d_cut);
    FAL_CHECK_HIP(hipGetLastError());
    // the last wait: the families and the edges cut
    FAL_CHECK_HIP(hipMemcpyAsync(h_fam, rank + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipMemcpyAsync(h_cut, d_cut, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipStreamSynchronize(st));
    *n_families = *h_fam;
    *n_rounds = rounds;
    ctx->counters[13] = (int64_t)*h_cut;
    return FAL_OK;
}
