// knn.hip -- mean squared distance of every point to its 3 nearest neighbours: the contract of simple_knn's distCUDA2,
// which the reference's GaussianModel.load_ply calls (scene/gaussian_model.py:39,459) to give a point cloud without
// scale_* properties its initial scales. Exact: every result equals the brute force bit for bit (DESIGN.md "3-NN").
//
//   d(i,j) = dx*dx + dy*dy + dz*dz, left to right in fp32, dx = x[j] - x[i]     (built with -ffp-contract=off)
//   out[i] = ((d0 + d1) + d2) / 3,  d0 <= d1 <= d2 the three smallest d(i,j) over j != i (by index, so a duplicate is a 0);
//   fewer than 3 neighbours (P <= 3): the missing slots hold FLT_MAX.
//
// Three stages (stage names knn_sort / knn_bounds / knn_query in the profile):
//   sort    bounding box -> 63-bit Morton code per point -> rocPRIM radix sort of (code, id) -> coordinates gathered
//           into sorted order (one float4 per point)
//   bounds  boxes of KNN_LEAF consecutive sorted points, then an implicit complete binary tree over the leaves
//           (padded to a power of two; absent nodes hold the empty box, whose bound is +inf)
//   query   one lane per sorted point (a wave holds 64 Morton neighbours): seed the best 3 from the +-3 sorted window,
//           scan the own leaf, then climb: at every level visit the sibling subtree depth first, pruning every node
//           whose lower bound is >= the current third-best. Stops as soon as the third-best is 0.
//
// The lower bound of a box uses the same fp32 operations in the same order as d(i,j), on the box point nearest to the
// query (per axis a clamp, which is exact). |fl(a - q)| is monotone in |a - q| and fl(u + v) in u and v, so the bound is
// <= d(i,j) for every point of the box after rounding too: pruning never drops a neighbour that would change the result.
//
// knn_query has two compile-time variants of one body. KnnBest (above) keeps the three distances only. KnnBestIdx keeps
// (distance, original index) pairs for c3dgs_knn_neighbours, whose contract is the three smallest PAIRS in lexicographic
// order: among equal distances the lowest original index wins, whatever order the tree is walked in. That tie rule changes
// two things and only in that variant. A candidate is compared as (d, id), the id read from ids_sorted only when d <= the
// third-best distance. And a node is pruned only when its bound is STRICTLY greater than the third-best: a box whose bound
// equals it can hold a point at exactly that distance with a lower index, so it is visited (while the third-best is
// non-zero; at zero the search stops as before, and the three coincident points found are reported in ascending index
// order). The bound's exactness argument is untouched. The cost is the extra visits of equal-bound nodes, which only
// exact ties produce (lattices, duplicated points), and three more registers per lane.
#include "knn_tree.hpp"
#include <cfloat>
#include <climits>
#include <rocprim/device/device_radix_sort.hpp>

namespace c3dgs {

static size_t knn_sort_temp_bytes(size_t p)
{
    size_t temp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, temp, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                    (uint32_t*)nullptr, p, 0u, 63u);
    return temp < 256 ? 256 : temp;
}

KnnLayout knn_layout(int P)
{
    KnnLayout L{};
    const size_t p = (size_t)(P > 0 ? P : 1);
    L.nleaf = (int)((p + KNN_LEAF - 1) / KNN_LEAF);
    L.npow = 1;
    L.levels = 1;
    while (L.npow < L.nleaf) { L.npow <<= 1; L.levels++; }
    size_t o = 0;
    L.box = o;          o = align_up(o + 32);
    L.codes = o;        o = align_up(o + p * 8);
    L.codes_sorted = o; o = align_up(o + p * 8);
    L.ids = o;          o = align_up(o + p * 4);
    L.ids_sorted = o;   o = align_up(o + p * 4);
    L.pts = o;          o = align_up(o + p * 16);
    L.nodes = o;        o = align_up(o + (size_t)2 * L.npow * 32);   // 2*npow - 1 nodes of {lo, hi} float4
    L.temp = o;         L.temp_bytes = knn_sort_temp_bytes(p);
    o = align_up(o + L.temp_bytes);
    L.total = o;
    return L;
}

size_t knn_workspace_bytes(int P) { return knn_layout(P).total; }

__global__ void __launch_bounds__(256)
knn_bbox(int P, const float* __restrict__ xyz, uint32_t* __restrict__ box /*[6] ordered ints: min xyz, max xyz*/)
{
    float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float v = xyz[3 * (size_t)i + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
        }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(&box[a], f2ord(mn[a]));
            atomicMax(&box[3 + a], f2ord(mx[a]));
        }
}

// Morton code of each point over the bounding box (the quantisation is knn_tree.hpp's knn_axis_cell).
__global__ void __launch_bounds__(256)
knn_codes(int P, const float* __restrict__ xyz, const uint32_t* __restrict__ box, uint64_t* __restrict__ codes,
          uint32_t* __restrict__ ids)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint64_t code = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        code |= knn_split_by_3(knn_axis_cell(xyz[3 * (size_t)i + a], ord2f(box[a]), ord2f(box[3 + a]))) << a;
    codes[i] = code;
    ids[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256)
knn_gather(int P, const float* __restrict__ xyz, const uint32_t* __restrict__ ids_sorted, float4* __restrict__ pts)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= P) return;
    const size_t i = ids_sorted[s];
    pts[s] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
}

// Leaf boxes: one lane per sorted point, 32 lanes per leaf. Slots of the padded level past the last point get the empty
// box {lo = +inf, hi = -inf}, whose bound is +inf.
__global__ void __launch_bounds__(256)
knn_leaf_bounds(int P, int npow, const float4* __restrict__ pts, float4* __restrict__ nodes)
{
    const int s = blockIdx.x * 256 + threadIdx.x;              // grid covers npow * KNN_LEAF lanes
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (s < P) { lo = pts[s]; hi = lo; }
#pragma unroll
    for (int o = KNN_LEAF / 2; o > 0; o >>= 1) {
        lo.x = fminf(lo.x, __shfl_xor(lo.x, o)); lo.y = fminf(lo.y, __shfl_xor(lo.y, o)); lo.z = fminf(lo.z, __shfl_xor(lo.z, o));
        hi.x = fmaxf(hi.x, __shfl_xor(hi.x, o)); hi.y = fmaxf(hi.y, __shfl_xor(hi.y, o)); hi.z = fmaxf(hi.z, __shfl_xor(hi.z, o));
    }
    const int leaf = s / KNN_LEAF;
    if ((s & (KNN_LEAF - 1)) == 0 && leaf < npow) {
        nodes[2 * (size_t)leaf] = lo;
        nodes[2 * (size_t)leaf + 1] = hi;
    }
}

// One tree level from the level below: node k is the union of children 2k and 2k + 1.
__global__ void __launch_bounds__(256)
knn_node_bounds(int n, const float4* __restrict__ child, float4* __restrict__ parent)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float4 alo = child[4 * (size_t)k], ahi = child[4 * (size_t)k + 1];
    const float4 blo = child[4 * (size_t)k + 2], bhi = child[4 * (size_t)k + 3];
    parent[2 * (size_t)k] = make_float4(fminf(alo.x, blo.x), fminf(alo.y, blo.y), fminf(alo.z, blo.z), 0.f);
    parent[2 * (size_t)k + 1] = make_float4(fmaxf(ahi.x, bhi.x), fmaxf(ahi.y, bhi.y), fmaxf(ahi.z, bhi.z), 0.f);
}

struct KnnBest {
    using Out = float* __restrict__;                             // [P]: ((d0 + d1) + d2) / 3
    static constexpr bool kIndices = false;
    float d0, d1, d2;
    static __device__ __forceinline__ KnnBest empty() { return { INFINITY, INFINITY, INFINITY }; }
    __device__ __forceinline__ void consider(float d, const uint32_t* __restrict__, int) { insert(d); }
    __device__ __forceinline__ bool visits(float bound) const { return bound < d2; }
    __device__ __forceinline__ void insert(float d)
    {
        if (d < d2) {
            if (d < d1) {
                d2 = d1;
                if (d < d0) { d1 = d0; d0 = d; } else d1 = d;
            } else d2 = d;
        }
    }
};

// The three smallest (distance, original index) pairs in lexicographic order (see the head of the file).
struct KnnNeighboursOut { int32_t* idx; float* d2; };           // [P,3] each
struct KnnBestIdx {
    using Out = KnnNeighboursOut;
    static constexpr bool kIndices = true;
    float d0, d1, d2;
    int i0, i1, i2;
    static __device__ __forceinline__ KnnBestIdx empty() { return { INFINITY, INFINITY, INFINITY, INT_MAX, INT_MAX, INT_MAX }; }
    __device__ __forceinline__ void consider(float d, const uint32_t* __restrict__ ids_sorted, int j)
    {
        if (!(d <= d2)) return;
        const int id = (int)ids_sorted[j];
        if (d < d2 || id < i2) {
            if (d < d1 || (d == d1 && id < i1)) {
                d2 = d1; i2 = i1;
                if (d < d0 || (d == d0 && id < i0)) { d1 = d0; i1 = i0; d0 = d; i0 = id; } else { d1 = d; i1 = id; }
            } else { d2 = d; i2 = id; }
        }
    }
    __device__ __forceinline__ bool visits(float bound) const { return bound <= d2; }
    __device__ __forceinline__ void store(Out out, size_t id, int P) const   // missing slots: idx -1 (their d is FLT_MAX)
    {
        out.idx[3 * id] = P < 2 ? -1 : i0; out.idx[3 * id + 1] = P < 3 ? -1 : i1; out.idx[3 * id + 2] = P < 4 ? -1 : i2;
        out.d2[3 * id] = d0; out.d2[3 * id + 1] = d1; out.d2[3 * id + 2] = d2;
    }
};

// every point of leaf `leaf` except the query and the seed window (already counted)
template <class Best>
__device__ __forceinline__ void knn_scan_leaf(int P, int leaf, int s, const float4* __restrict__ pts,
                                              const uint32_t* __restrict__ ids_sorted, const float4 q, Best& b)
{
    const int j1 = min(P, (leaf + 1) * KNN_LEAF);
    for (int j = leaf * KNN_LEAF; j < j1; j++) {
        if (j >= s - KNN_WINDOW && j <= s + KNN_WINDOW) continue;
        b.consider(knn_d2(pts[j], q), ids_sorted, j);
        if (b.d2 == 0.f) return;
    }
}

template <class Best>
__global__ void __launch_bounds__(256)
knn_query(int P, int npow, int levels, const float4* __restrict__ pts, const float4* __restrict__ nodes,
          const uint32_t* __restrict__ ids_sorted, typename Best::Out out)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= P) return;
    const float4 q = pts[s];
    Best b = Best::empty();
    for (int j = max(0, s - KNN_WINDOW); j <= min(P - 1, s + KNN_WINDOW); j++)
        if (j != s) b.consider(knn_d2(pts[j], q), ids_sorted, j);
    const int two_npow = 2 * npow;
    if (b.d2 > 0.f) {
        int leaf = s / KNN_LEAF;
        knn_scan_leaf(P, leaf, s, pts, ids_sorted, q, b);
        // climb: at level l the subtree of the sibling of the query's own ancestor; depth first, left child first
        for (int l0 = 0; l0 + 1 < levels && b.d2 > 0.f; l0++, leaf >>= 1) {
            int l = l0, k = leaf ^ 1;
            for (;;) {
                const float4* nd = nodes + 2 * ((size_t)knn_level_offset(two_npow, l) + k);
                if (b.visits(knn_box_d2(nd[0], nd[1], q))) {
                    if (l > 0) { l--; k <<= 1; continue; }
                    knn_scan_leaf(P, k, s, pts, ids_sorted, q, b);
                    if (b.d2 == 0.f) break;
                }
                while (l != l0 && (k & 1)) { k >>= 1; l++; }     // next node of the subtree in depth-first order
                if (l == l0) break;
                k++;
            }
        }
    }
    if (P <= KNN_WINDOW) {                                       // fewer than 3 neighbours: the missing slots are FLT_MAX
        b.d2 = FLT_MAX;
        if (P < 3) b.d1 = FLT_MAX;
        if (P < 2) b.d0 = FLT_MAX;
    }
    if constexpr (Best::kIndices) b.store(out, ids_sorted[s], P);
    else out[ids_sorted[s]] = __fdiv_rn((b.d0 + b.d1) + b.d2, 3.0f);
}

static int knn_grid(size_t n) { return (int)((n + 255) / 256); }

int run_knn_sort(int P, const float* xyz, void* workspace, hipStream_t s)
{
    const KnnLayout L = knn_layout(P);
    char* w = (char*)workspace;
    uint32_t* box = (uint32_t*)(w + L.box);
    if (hipMemsetAsync(box, 0xff, 12, s) != hipSuccess || hipMemsetAsync(box + 3, 0, 12, s) != hipSuccess) return 1;
    const int grid = knn_grid((size_t)P);
    knn_bbox<<<grid < 1024 ? grid : 1024, 256, 0, s>>>(P, xyz, box);
    knn_codes<<<grid, 256, 0, s>>>(P, xyz, box, (uint64_t*)(w + L.codes), (uint32_t*)(w + L.ids));
    size_t temp_bytes = L.temp_bytes;
    if (rocprim::radix_sort_pairs((void*)(w + L.temp), temp_bytes, (const uint64_t*)(w + L.codes), (uint64_t*)(w + L.codes_sorted),
                                  (const uint32_t*)(w + L.ids), (uint32_t*)(w + L.ids_sorted), (size_t)P, 0u, 63u, s) != hipSuccess)
        return 1;
    knn_gather<<<grid, 256, 0, s>>>(P, xyz, (const uint32_t*)(w + L.ids_sorted), (float4*)(w + L.pts));
    return 0;
}

void launch_knn_bounds(int P, void* workspace, hipStream_t s)
{
    const KnnLayout L = knn_layout(P);
    char* w = (char*)workspace;
    float4* nodes = (float4*)(w + L.nodes);
    knn_leaf_bounds<<<knn_grid((size_t)L.npow * KNN_LEAF), 256, 0, s>>>(P, L.npow, (const float4*)(w + L.pts), nodes);
    size_t off = 0;
    for (int n = L.npow / 2; n >= 1; n /= 2) {
        knn_node_bounds<<<knn_grid((size_t)n), 256, 0, s>>>(n, nodes + 2 * off, nodes + 2 * (off + 2 * (size_t)n));
        off += 2 * (size_t)n;
    }
}

void launch_knn_query(int P, const void* workspace, float* out, hipStream_t s)
{
    const KnnLayout L = knn_layout(P);
    const char* w = (const char*)workspace;
    knn_query<KnnBest><<<knn_grid((size_t)P), 256, 0, s>>>(P, L.npow, L.levels, (const float4*)(w + L.pts),
                                                            (const float4*)(w + L.nodes), (const uint32_t*)(w + L.ids_sorted), out);
}

void launch_knn_query_neighbours(int P, const void* workspace, int32_t* idx, float* d2, hipStream_t s)
{
    const KnnLayout L = knn_layout(P);
    const char* w = (const char*)workspace;
    knn_query<KnnBestIdx><<<knn_grid((size_t)P), 256, 0, s>>>(P, L.npow, L.levels, (const float4*)(w + L.pts),
                                                               (const float4*)(w + L.nodes), (const uint32_t*)(w + L.ids_sorted),
                                                               KnnNeighboursOut{ idx, d2 });
}

} // namespace c3dgs
