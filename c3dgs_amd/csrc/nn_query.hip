// nn_query.hip -- exact nearest neighbour of EXTERNAL queries in the box tree knn.hip builds (knn_tree.hpp): the search behind the
// geometry metrics (accuracy / completeness / Chamfer / F-score), where the two point sets differ. Compiled without contraction.
//
//   d(q, j) = dx*dx + dy*dy + dz*dz, left to right in fp32, dx = x[j] - q.x        (knn_d2)
//   result(q) = the lexicographically smallest pair (d, j) over all j: among equal distances the lowest original index wins,
//               at d == 0 too. d may be +inf (the subtraction overflowed): then every d is +inf and j = 0.
//   P == 0 or a query with a non-finite coordinate: idx = -1, d2 = FLT_MAX, nothing is walked.
//
// The index IS the knn workspace after knn_sort + knn_bounds; a query only reads it, so one index serves any number of calls.
//
// nn_query_kernel, one lane per query:
//   seed   the query, clamped into the reference's bounding box, gets the Morton code knn_codes would give it; a binary search in
//          codes_sorted finds its place s, and the leaf of s plus the KNN_WINDOW sorted points each side of s are scanned. The seed
//          only lowers the first bound: the result is the minimum over everything the walk visits, and the walk alone is exact.
//   walk   the stackless depth-first step of knn_query's sibling subtrees with the ROOT as the subtree: left child first, a node is
//          entered iff knn_box_d2 <= the best distance so far (non-strict: a box whose bound equals it can hold a point at that
//          distance with a lower index), leaves are scanned, and `while (k & 1)` climbs to the next node. Every loop is bounded by
//          the tree (at most 2 npow - 1 node visits, KNN_LEAF points per leaf); there is no waiting loop.
// knn_box_d2 is a lower bound of knn_d2 over the box AFTER rounding for any finite q, inside the bounding box or far outside it:
// per axis the clamp of q into [lo, hi] is exact and |c - q| <= |p - q| for every p of the box, fl(a - q) is monotone in a, so is
// the square, and fl(u + v) is monotone in u and v. An overflow gives +inf on both sides and keeps the order.
//
// Two query orders, identical results (the contract fixes them): the caller's, and Morton order -- nn_query_codes_kernel +
// a rocPRIM pair sort in `workspace`, the kernel then takes query order[t] and scatters its result. A wave of Morton neighbours
// walks the same nodes, so its lanes stay converged and its loads coalesce; the sort costs what it costs.
#include "knn_tree.hpp"
#include <cfloat>
#include <climits>
#include <rocprim/device/device_radix_sort.hpp>

namespace c3dgs {

namespace {

struct NnSortLayout { size_t codes, codes_sorted, ids, ids_sorted, temp, temp_bytes, total; };

size_t nn_sort_temp_bytes(size_t q)
{
    size_t temp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, temp, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                    (uint32_t*)nullptr, q, 0u, 64u);
    return temp < 256 ? 256 : temp;
}

NnSortLayout nn_sort_layout(int Q)
{
    NnSortLayout L{};
    const size_t q = (size_t)(Q > 0 ? Q : 1);
    size_t o = 0;
    L.codes = o;        o = align_up(o + q * 8);
    L.codes_sorted = o; o = align_up(o + q * 8);
    L.ids = o;          o = align_up(o + q * 4);
    L.ids_sorted = o;   o = align_up(o + q * 4);
    L.temp = o;         L.temp_bytes = nn_sort_temp_bytes(q);
    o = align_up(o + L.temp_bytes);
    L.total = o;
    return L;
}

__device__ __forceinline__ bool nn_finite(const float x, const float y, const float z)
{
    return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;
}

// the code knn_codes gives the query clamped into the reference's bounding box (an empty box, P == 0, gives 0)
__device__ __forceinline__ uint64_t nn_code(const float4 q, const uint32_t* __restrict__ box)
{
    const float v[3] = { q.x, q.y, q.z };
    uint64_t code = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float mn = ord2f(box[a]), mx = ord2f(box[3 + a]);
        code |= knn_split_by_3(knn_axis_cell(fminf(fmaxf(v[a], mn), mx), mn, mx)) << a;
    }
    return code;
}

// Sort keys of the queries: the code above; a query with a non-finite coordinate sorts behind every other (it walks nothing).
__global__ void __launch_bounds__(256)
nn_query_codes_kernel(const int Q, const float* __restrict__ queries, const uint32_t* __restrict__ box,
                      uint64_t* __restrict__ codes, uint32_t* __restrict__ ids)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const float4 q = make_float4(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2], 0.f);
    codes[i] = nn_finite(q.x, q.y, q.z) ? nn_code(q, box) : ~0ull;
    ids[i] = (uint32_t)i;
}

struct NnBest {
    float d; int id;
    __device__ __forceinline__ void consider(const float c, const uint32_t* __restrict__ ids_sorted, const int j)
    {
        if (!(c <= d)) return;
        const int cid = (int)ids_sorted[j];
        if (c < d || cid < id) { d = c; id = cid; }
    }
};

__device__ __forceinline__ void nn_scan(const int j0, const int j1, const float4* __restrict__ pts,
                                        const uint32_t* __restrict__ ids_sorted, const float4 q, NnBest& b)
{
    for (int j = j0; j < j1; j++) b.consider(knn_d2(pts[j], q), ids_sorted, j);
}

template <bool SORTED, bool COUNT>
__global__ void __launch_bounds__(256)
nn_query_kernel(const int P, const int npow, const int levels, const uint32_t* __restrict__ box,
                const uint64_t* __restrict__ codes_sorted, const float4* __restrict__ pts, const float4* __restrict__ nodes,
                const uint32_t* __restrict__ ids_sorted, const int Q, const float* __restrict__ queries,
                const uint32_t* __restrict__ order, int32_t* __restrict__ idx, float* __restrict__ d2,
                uint32_t* __restrict__ leaves)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Q) return;
    size_t qi = (size_t)t;
    if (SORTED) { qi = order[t]; if (qi >= (size_t)Q) return; }          // (a workspace that is not this call's sort)
    const float4 q = make_float4(queries[3 * qi], queries[3 * qi + 1], queries[3 * qi + 2], 0.f);
    if (P <= 0 || !nn_finite(q.x, q.y, q.z)) {
        idx[qi] = -1; d2[qi] = FLT_MAX;
        if (COUNT) leaves[qi] = 0u;
        return;
    }
    // seed: lower bound of the query's code among the sorted codes
    const uint64_t code = nn_code(q, box);
    int lo = 0, hi = P;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (codes_sorted[mid] < code) lo = mid + 1; else hi = mid;
    }
    const int s = min(lo, P - 1), seed_leaf = s / KNN_LEAF;
    NnBest b{ INFINITY, INT_MAX };
    nn_scan(max(0, min(seed_leaf * KNN_LEAF, s - KNN_WINDOW)), min(P, max((seed_leaf + 1) * KNN_LEAF, s + KNN_WINDOW + 1)), pts,
            ids_sorted, q, b);
    uint32_t nleaves = 1u;
    // walk: the whole tree as one subtree; depth first, left child first
    const int two_npow = 2 * npow, top = levels - 1;
    int l = top, k = 0;
    for (;;) {
        const float4* nd = nodes + 2 * ((size_t)knn_level_offset(two_npow, l) + k);
        if (knn_box_d2(nd[0], nd[1], q) <= b.d) {
            if (l > 0) { l--; k <<= 1; continue; }
            if (k != seed_leaf) {                                         // the seed has scanned its leaf
                nn_scan(k * KNN_LEAF, min(P, (k + 1) * KNN_LEAF), pts, ids_sorted, q, b);
                if (COUNT) nleaves++;
            }
        }
        while (l != top && (k & 1)) { k >>= 1; l++; }                     // next node in depth-first order
        if (l == top) break;
        k++;
    }
    idx[qi] = b.id; d2[qi] = b.d;
    if (COUNT) leaves[qi] = nleaves;
}

int nn_grid(const size_t n) { return (int)((n + 255) / 256); }

} // namespace

size_t nn_query_workspace_bytes(int Q) { return nn_sort_layout(Q).total; }

// keys and ids of the Q queries, sorted by key, in `workspace`
int run_nn_query_sort(int P, const void* index, int Q, const float* queries, void* workspace, hipStream_t s)
{
    const KnnLayout K = knn_layout(P);
    const NnSortLayout L = nn_sort_layout(Q);
    char* w = (char*)workspace;
    nn_query_codes_kernel<<<nn_grid((size_t)Q), 256, 0, s>>>(Q, queries, (const uint32_t*)((const char*)index + K.box),
                                                             (uint64_t*)(w + L.codes), (uint32_t*)(w + L.ids));
    size_t temp_bytes = L.temp_bytes;
    return rocprim::radix_sort_pairs((void*)(w + L.temp), temp_bytes, (const uint64_t*)(w + L.codes), (uint64_t*)(w + L.codes_sorted),
                                     (const uint32_t*)(w + L.ids), (uint32_t*)(w + L.ids_sorted), (size_t)Q, 0u, 64u, s) != hipSuccess;
}

// sorted: the queries in the order run_nn_query_sort left in `workspace`; leaves: optional [Q] count of the leaves each query scanned
void launch_nn_query(int P, const void* index, int Q, const float* queries, bool sorted, const void* workspace, int32_t* idx, float* d2,
                     uint32_t* leaves, hipStream_t s)
{
    const KnnLayout K = knn_layout(P);
    const char* x = (const char*)index;
    const uint32_t* order = sorted ? (const uint32_t*)((const char*)workspace + nn_sort_layout(Q).ids_sorted) : nullptr;
    const uint32_t* box = (const uint32_t*)(x + K.box);
    const uint64_t* codes = (const uint64_t*)(x + K.codes_sorted);
    const float4* pts = (const float4*)(x + K.pts);
    const float4* nodes = (const float4*)(x + K.nodes);
    const uint32_t* ids = (const uint32_t*)(x + K.ids_sorted);
    const int grid = nn_grid((size_t)Q);
#define C3DGS_NN_LAUNCH(S, C) nn_query_kernel<S, C><<<grid, 256, 0, s>>>(P, K.npow, K.levels, box, codes, pts, nodes, ids, Q, queries, \
                                                                         order, idx, d2, leaves)
    if (sorted) { if (leaves) C3DGS_NN_LAUNCH(true, true); else C3DGS_NN_LAUNCH(true, false); }
    else { if (leaves) C3DGS_NN_LAUNCH(false, true); else C3DGS_NN_LAUNCH(false, false); }
#undef C3DGS_NN_LAUNCH
}

} // namespace c3dgs
