// Annotation propagation through the molecular families (fal_network_propagate; DESIGN.md "Annotation propagation";
// netpropagate.h holds the pure core and the rule).
//
// A level-synchronous walk from the annotated nodes.  The state (hops, source, parent, score, and one 64-bit key per node) lives
// in scratch.  Level d is two launches: the relax kernel, one thread per link, offers the unreached end of a link whose other
// end has hops d - 1 the candidate's key with an unsigned atomicMax; the commit kernel, one thread per node, turns a node with a
// key into a node of level d.  They are two launches because they must be: in one, a node committed at level d would be read as
// a parent by a link's thread that runs later, and the result would depend on the order of the threads.  The maximum of the keys
// does not depend on the order of arrival, and nothing else is contended.
//
// All max_hops levels are enqueued without the host looking.  Two device words let a level without work return at once: the
// relax kernel of level d runs only when `levels` == d - 1 (the commit of the level before reached a node; level 0 always
// counts) and raises `pending` = d with its first candidate; the commit kernel of level d runs only when `pending` == d and
// sets `levels` = d.  Each word is written by the launches of one kind and read by those of the other, so no launch reads a
// word that it writes.  A link or seed the check refuses raises the error word, and every later kernel returns on it: no kernel
// follows an invalid endpoint, and the emit kernel, the only one that writes the caller's arrays, writes nothing.
//
// Synchronisations: one, for the error word and the two counts.
#include "common.h"
#include "ivf.h"
#include "netpropagate.h"
#include "util.h"

namespace fal {
namespace {

constexpr int kPropBlock = 256;
enum { PROP_ERR = 0, PROP_LEVELS = 1, PROP_PENDING = 2 };   // int32 words of the misc block; the reached count is the unsigned long long at byte 16

__global__ void prop_check_kernel(const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, const float* __restrict__ es, int64_t m,
                                  int64_t n, int32_t* __restrict__ misc) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x)
        if (!prop_valid_edge(eu[e], ev[e], es[e], n)) misc[PROP_ERR] = 1;     // (every writer stores the same 1)
}

// level 0, and the seed check
__global__ void prop_init_kernel(const int32_t* __restrict__ seed, int64_t n, int32_t* __restrict__ hops, int32_t* __restrict__ source,
                                 int32_t* __restrict__ parent, float* __restrict__ score, unsigned long long* __restrict__ key,
                                 int32_t* __restrict__ misc) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = seed[i];
        if (!prop_valid_seed(s)) misc[PROP_ERR] = 1;
        const bool annotated = s >= 0;
        hops[i] = annotated ? 0 : -1;
        source[i] = annotated ? (int32_t)i : -1;
        parent[i] = -1;
        score[i] = annotated ? 1.0f : 0.0f;
        key[i] = 0ull;
    }
}

// hops and score are read only here: the commit kernel of this level, a later launch, writes them
__global__ void prop_relax_kernel(const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, const float* __restrict__ es, int64_t m,
                                  const int32_t* __restrict__ hops, const float* __restrict__ score, unsigned long long* __restrict__ key,
                                  double min_score, int32_t d, int32_t* __restrict__ misc) {
    if (misc[PROP_ERR] != 0 || misc[PROP_LEVELS] != d - 1) return;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = eu[e], v = ev[e];
        const int32_t hu = hops[u], hv = hops[v];
        int32_t a, b;
        if (hu == d - 1 && hv == -1) a = u, b = v;
        else if (hv == d - 1 && hu == -1) a = v, b = u;
        else continue;
        const float c = prop_candidate(score[a], es[e]);
        if (!prop_counts(c, min_score)) continue;
        atomicMax(&key[b], prop_key(c, a));
        misc[PROP_PENDING] = d;                                             // (every writer stores the same d)
    }
}

// whole waves: every lane reaches the ballot (one atomic per wave for the count).  source[a] is a node of level d - 1: nobody
// writes it in this launch
__global__ __launch_bounds__(kPropBlock) void prop_commit_kernel(int64_t n, const unsigned long long* __restrict__ key, int32_t* __restrict__ hops,
                                                                int32_t* source, int32_t* __restrict__ parent, float* __restrict__ score,
                                                                int32_t d, int32_t* __restrict__ misc, unsigned long long* __restrict__ n_reached) {
    if (misc[PROP_ERR] != 0 || misc[PROP_PENDING] != d) return;
    for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        bool reached = false;
        if (i < n && hops[i] == -1) {
            const unsigned long long k = key[i];
            if (k != 0ull) {
                const int32_t a = prop_key_parent(k);
                hops[i] = d;
                parent[i] = a;
                source[i] = source[a];
                score[i] = prop_key_score(k);
                misc[PROP_LEVELS] = d;                                      // (every writer stores the same d)
                reached = true;
            }
        }
        const unsigned long long mask = __ballot(reached);
        if (mask != 0 && (threadIdx.x & 63) == 0) atomicAdd(n_reached, (unsigned long long)__popcll(mask));
    }
}

// the state into the caller's arrays, unless the check refused the input
__global__ void prop_emit_kernel(int64_t n, const int32_t* __restrict__ hops, const int32_t* __restrict__ source,
                                 const int32_t* __restrict__ parent, const float* __restrict__ score, const int32_t* __restrict__ misc,
                                 int32_t* __restrict__ node_source, int32_t* __restrict__ node_hops, int32_t* __restrict__ node_parent,
                                 float* __restrict__ node_score) {
    if (misc[PROP_ERR] != 0) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        node_source[i] = source[i];
        node_hops[i] = hops[i];
        node_parent[i] = parent[i];
        node_score[i] = score[i];
    }
}

}  // namespace
}  // namespace fal
FAL_WARM_KERNEL(fal::prop_relax_kernel);      // (fal_ctx_plan: this unit's code object is loaded up front)

using namespace fal;

extern "C" int fal_network_propagate(fal_ctx* ctx, const int32_t* edge_u, const int32_t* edge_v, const float* edge_sim, int64_t m, int64_t n,
                                     const int32_t* node_seed, int max_hops, double min_score, int32_t* node_source, int32_t* node_hops,
                                     int32_t* node_parent, float* node_score, int64_t* n_reached, int64_t* n_levels) {
    fal::CallScope _call(ctx);
    FAL_REQUIRE(ctx && n_reached && n_levels && n >= 0 && n < (int64_t)INT32_MAX && m >= 0, FAL_EINVAL,
                "fal_network_propagate: bad argument");
    FAL_REQUIRE(prop_valid_hops(max_hops), FAL_EINVAL, "fal_network_propagate: max_hops %d is outside [1, %d]", max_hops, kPropMaxHops);
    FAL_REQUIRE(prop_valid_min_score(min_score), FAL_EINVAL, "fal_network_propagate: min_score %g is outside [0, 1] or not a number",
                min_score);
    FAL_REQUIRE(n > 0 || m == 0, FAL_EINVAL, "fal_network_propagate: %lld links between no nodes", (long long)m);
    FAL_REQUIRE(m == 0 || (edge_u && edge_v && edge_sim), FAL_EINVAL, "fal_network_propagate: NULL link array");
    FAL_REQUIRE(n == 0 || (node_seed && node_source && node_hops && node_parent && node_score), FAL_EINVAL,
                "fal_network_propagate: NULL node array");
    ctx->counters[15] = 0;
    if (n == 0) {
        *n_reached = *n_levels = 0;
        return FAL_OK;
    }
    hipStream_t st = ctx->stream;
    ScratchLayout L;
    const auto misc = L.array<int32_t>(16);                // 64 B of meta words; the 64-bit count of reached nodes lives in words 4 and 5
    const auto key = L.array<unsigned long long>(n);
    const auto hops = L.array<int32_t>(n), source = L.array<int32_t>(n), parent = L.array<int32_t>(n);
    const auto score = L.array<float>(n);
    FAL_TRY(L.reserve(ctx, SLOT_PROP));
    unsigned long long* d_reached = reinterpret_cast<unsigned long long*>(misc + 4);
    unsigned char* pin = nullptr;
    FAL_TRY(ctx->pinned_reserve(64, (void**)&pin));
    const int32_t* h_misc = reinterpret_cast<const int32_t*>(pin);
    const unsigned long long* h_reached = reinterpret_cast<const unsigned long long*>(pin + 16);
    const unsigned ngrid = capped_grid(ctx, n, kPropBlock), egrid = capped_grid(ctx, m, kPropBlock);
    FAL_CHECK_HIP(hipMemsetAsync(misc, 0, 64, st));
    if (m > 0) hipLaunchKernelGGL(prop_check_kernel, dim3(egrid), dim3(kPropBlock), 0, st, edge_u, edge_v, edge_sim, m, n, misc);
    hipLaunchKernelGGL(prop_init_kernel, dim3(ngrid), dim3(kPropBlock), 0, st, node_seed, n, hops, source, parent, score, key, misc);
    for (int32_t d = 1; m > 0 && d <= (int32_t)max_hops; ++d) {
        hipLaunchKernelGGL(prop_relax_kernel, dim3(egrid), dim3(kPropBlock), 0, st, edge_u, edge_v, edge_sim, m, hops, score, key, min_score,
                           d, misc);
        hipLaunchKernelGGL(prop_commit_kernel, dim3(ngrid), dim3(kPropBlock), 0, st, n, key, hops, source, parent, score, d, misc, d_reached);
    }
    hipLaunchKernelGGL(prop_emit_kernel, dim3(ngrid), dim3(kPropBlock), 0, st, n, hops, source, parent, score, misc, node_source, node_hops,
                       node_parent, node_score);
    FAL_CHECK_HIP(hipGetLastError());
    // the call's one wait: the error word, the last level that reached a node and the nodes reached
    FAL_CHECK_HIP(hipMemcpyAsync(pin, misc, 64, hipMemcpyDeviceToHost, st));
    FAL_CHECK_HIP(hipStreamSynchronize(st));
    FAL_REQUIRE(h_misc[PROP_ERR] == 0, FAL_EINVAL,
                "fal_network_propagate: a link with an end outside the %lld nodes, with both ends the same, or with a sim that is negative "
                "or not finite, or a seed below -1", (long long)n);
    *n_reached = (int64_t)*h_reached;
    *n_levels = h_misc[PROP_LEVELS];
    ctx->counters[15] = (int64_t)*h_reached;
    return FAL_OK;
}
