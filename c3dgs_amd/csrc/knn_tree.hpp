// knn_tree.hpp -- what knn.hip (the 3-NN of the points IN the tree) and nn_query.hip (the nearest neighbour of points from
// OUTSIDE it) share: the workspace layout that is the tree, the Morton quantisation, the distance and its box bound. The
// exactness argument of the bound is at the head of knn.hip; it asks nothing of where the query lies.
#pragma once
#include "common.hpp"
#include <cfloat>

namespace c3dgs {

constexpr int KNN_LEAF = 32;             // points per leaf box: half a wave, reduced with lane shuffles
constexpr int KNN_WINDOW = 3;            // sorted neighbours each side that seed the best 3

struct KnnLayout {
    int nleaf, npow, levels;             // leaves, leaves padded to a power of two, tree levels (root level = levels - 1)
    size_t box, codes, codes_sorted, ids, ids_sorted, pts, nodes, temp, temp_bytes, total;
};
KnnLayout knn_layout(int P);             // knn.hip

// first node of tree level l (level 0 = the npow leaf slots, then npow/2, ...): 2*npow - 2*npow / 2^l
__device__ __forceinline__ int knn_level_offset(int two_npow, int l) { return two_npow - (two_npow >> l); }

__device__ __forceinline__ uint64_t knn_split_by_3(uint32_t a)   // 21 bits -> every third bit of 63
{
    uint64_t x = a & 0x1FFFFFull;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// The 21-bit cell of coordinate v on an axis of the bounding box [mn, mx]. Only the ORDER matters (it decides which points share
// a leaf), not the exact quantisation: a zero-extent axis (planar, collinear or single-point clouds) or an extent that overflows
// fp32 quantises to 0 instead of producing NaN.
__device__ __forceinline__ uint32_t knn_axis_cell(float v, float mn, float mx)
{
    const float ext = mx - mn;
    const float inv = (ext > 0.f && ext <= FLT_MAX) ? 2097151.0f / ext : 0.f;
    float t = (v - mn) * inv;
    t = (t >= 0.f) ? fminf(t, 2097151.0f) : 0.f;                // also maps a NaN to 0
    return (uint32_t)t;
}

__device__ __forceinline__ float knn_d2(const float4 p, const float4 q)
{
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return dx * dx + dy * dy + dz * dz;
}

// lower bound of knn_d2(p, q) over every p in [lo, hi], with the same rounding steps (see the head of knn.hip)
__device__ __forceinline__ float knn_box_d2(const float4 lo, const float4 hi, const float4 q)
{
    const float4 c = make_float4(fminf(fmaxf(q.x, lo.x), hi.x), fminf(fmaxf(q.y, lo.y), hi.y), fminf(fmaxf(q.z, lo.z), hi.z), 0.f);
    return knn_d2(c, q);
}

} // namespace c3dgs
