// bilagrid.hpp -- the launch plan and workspace layout of the bilateral-grid kernels (bilagrid.hip), shared with the entry points
// of c_abi.hip, which size and validate with it before any device work.
#pragma once
#include "common.hpp"

namespace c3dgs {

constexpr int BG_THREADS = 256;
constexpr int BG_SLAB_PIXELS = 8192;       // pixels one gather workgroup walks: 32 per thread in front of one reduction
constexpr int BG_STAGED_LDS_BYTES = 48 * 1024;   // the per-pixel kernels stage their part of the grid in LDS up to this size
constexpr int BG_MAX_LEVELS = 8;           // luma levels a gather workgroup keeps in registers (12 accumulators each)
constexpr int BG_TV_BLOCKS = 1024;         // partial sums of the total variation, one double each
constexpr int BG_TV_PER_BLOCK = 1024;      // elements per workgroup below that cap
constexpr size_t BG_TV_WORKSPACE_BYTES = (size_t)BG_TV_BLOCKS * sizeof(double);

// An upper bound of the pixels along one axis (n pixels, ng vertices) inside one vertex's footprint as bg_footprint() cuts it:
// [floor((i - 1) n / (ng - 1)) - 1, ceil((i + 1) n / (ng - 1)) + 1], at most 2 n / (ng - 1) + 5 pixels.
inline int bg_span(int n, int ng)
{
    if (ng <= 1) return n;
    const long long s = (2LL * n + ng - 2) / (ng - 1) + 5;
    return s < n ? (int)s : n;
}

// The gather by vertex: workgroup (vertex v = j Wg + i, slab s, level chunk c) walks rows [y_lo + s slab_rows, ...) of the
// vertex's footprint and writes the row partial[((v slabs + s) L + k) 12 + m] for its `lc` levels k; the fold adds the slabs in
// order. The workspace is that table (the total variation uses its first BG_TV_WORKSPACE_BYTES bytes).
struct BilagridPlan {
    int cols, rows;            // bg_span of the two axes
    int slab_rows, slabs;      // image rows per workgroup, workgroups per vertex
    int lc, chunks;            // levels per workgroup (1, 2, 4 or 8), workgroups per vertex and slab
    long long vertices, groups;   // Hg Wg, vertices x slabs
    size_t total_bytes;
};
inline BilagridPlan bilagrid_plan(int H, int W, int L, int Hg, int Wg)
{
    BilagridPlan P;
    P.cols = bg_span(W, Wg);
    P.rows = bg_span(H, Hg);
    P.slab_rows = BG_SLAB_PIXELS / P.cols > 0 ? BG_SLAB_PIXELS / P.cols : 1;
    P.slabs = (P.rows + P.slab_rows - 1) / P.slab_rows;
    P.lc = 1;
    while (P.lc < L && P.lc < BG_MAX_LEVELS) P.lc *= 2;
    P.chunks = (L + P.lc - 1) / P.lc;
    P.vertices = (long long)Hg * Wg;
    P.groups = P.vertices * P.slabs;
    const size_t partial = (size_t)P.groups * (size_t)L * 12 * sizeof(float);
    P.total_bytes = align_up(partial > BG_TV_WORKSPACE_BYTES ? partial : BG_TV_WORKSPACE_BYTES);
    return P;
}

// bilagrid.hip
void launch_bilagrid_slice(int H, int W, int L, int Hg, int Wg, const float* grid, const float* rgb, float* out, hipStream_t s);
void launch_bilagrid_gather(int H, int W, int L, int Hg, int Wg, const BilagridPlan& plan, const float* rgb, const float* dL_dout,
                            float* partial, hipStream_t s);
void launch_bilagrid_fold(int L, int Hg, int Wg, const BilagridPlan& plan, const float* partial, float* dL_dgrid, hipStream_t s);
void launch_bilagrid_rgb_backward(int H, int W, int L, int Hg, int Wg, const float* grid, const float* rgb, const float* dL_dout,
                                  float* dL_drgb, hipStream_t s);
void launch_bilagrid_tv(int C, int L, int Hg, int Wg, const float* grids, double* partial, float* out, hipStream_t s);
void launch_bilagrid_tv_backward(int C, int L, int Hg, int Wg, const float* grids, const float* dL_dtv, float* dL_dgrids, hipStream_t s);

} // namespace c3dgs
