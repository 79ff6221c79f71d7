// geometry_metrics.hip -- the reduction behind accuracy / completeness / Chamfer / F-score (no reference counterpart): nearest-
// neighbour squared distances of one direction -> {count, sum of d, count below each threshold} as doubles on the device.
//
// Per element i:  d = sqrt_rn(d2[i]) in fp32;  counted iff d2[i] != FLT_MAX (nn_query's "no neighbour"), d <= max_dist and, with a
// box, lo <= p_i <= hi on every axis (a NaN coordinate fails);  below threshold t iff counted and d < tau_t.
// Deterministic: geometry_partial_kernel gives every workgroup a fixed set of elements (a function of N alone) and folds lanes,
// waves and the workgroup in a fixed order into one row of fp64 partials; geometry_fold_kernel, one workgroup, adds the rows in
// index order. No floating-point atomics. The counts are integers until the last store. Bound: one read of d2 (and of the
// coordinates with a box), 4 to 16 B per element: HBM.
#include "common.hpp"
#include <cfloat>

namespace c3dgs {

namespace {

constexpr int GM_BLOCK = 256, GM_PER_THREAD = 8, GM_MAX_BLOCKS = 1024, GM_ROW = 2 + C3DGS_GEOMETRY_MAX_THRESHOLDS;

struct GmParams { float lo[3], hi[3], max_dist, tau[C3DGS_GEOMETRY_MAX_THRESHOLDS]; int T, boxed; };

int gm_blocks(const int64_t N)
{
    const int64_t b = (N + (int64_t)GM_BLOCK * GM_PER_THREAD - 1) / ((int64_t)GM_BLOCK * GM_PER_THREAD);
    return (int)(b < GM_MAX_BLOCKS ? b : GM_MAX_BLOCKS);
}

__global__ void __launch_bounds__(GM_BLOCK)
geometry_partial_kernel(const int64_t N, const float* __restrict__ d2, const float* __restrict__ points, const GmParams g,
                        double* __restrict__ partials)
{
    __shared__ double s_sum[GM_BLOCK / 64];
    __shared__ unsigned long long s_cnt[GM_BLOCK / 64][GM_ROW - 1];
    double sum = 0.0;
    unsigned long long cnt[GM_ROW - 1];
#pragma unroll
    for (int t = 0; t < GM_ROW - 1; t++) cnt[t] = 0;
    for (int64_t i = (int64_t)blockIdx.x * GM_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * GM_BLOCK) {
        const float v = d2[i];
        const float d = sqrtf(v);
        bool in = v != FLT_MAX && d <= g.max_dist;
        if (in && g.boxed) {
#pragma unroll
            for (int a = 0; a < 3; a++) { const float p = points[3 * i + a]; in = in && p >= g.lo[a] && p <= g.hi[a]; }
        }
        if (!in) continue;
        sum += (double)d;
        cnt[0]++;
#pragma unroll
        for (int t = 0; t < C3DGS_GEOMETRY_MAX_THRESHOLDS; t++) if (t < g.T && d < g.tau[t]) cnt[1 + t]++;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
#pragma unroll
        for (int t = 0; t < GM_ROW - 1; t++) cnt[t] += __shfl_xor(cnt[t], o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[wave] = sum;
#pragma unroll
        for (int t = 0; t < GM_ROW - 1; t++) s_cnt[wave][t] = cnt[t];
    }
    __syncthreads();
    if (threadIdx.x < GM_ROW) {
        double* row = partials + (size_t)blockIdx.x * GM_ROW;
        if (threadIdx.x == 1) {
            double v = 0.0;
            for (int w = 0; w < GM_BLOCK / 64; w++) v += s_sum[w];
            row[1] = v;
        } else {
            const int t = threadIdx.x == 0 ? 0 : threadIdx.x - 1;
            unsigned long long c = 0;
            for (int w = 0; w < GM_BLOCK / 64; w++) c += s_cnt[w][t];
            row[threadIdx.x] = (double)c;
        }
    }
}

// out[c] = the sum over the nb rows, in row order, of column c (c < 2 + T); nb == 0 leaves zeros
__global__ void __launch_bounds__(64)
geometry_fold_kernel(const int nb, const int T, const double* __restrict__ partials, double* __restrict__ out)
{
    const int c = threadIdx.x;
    if (c >= 2 + T) return;
    double v = 0.0;
#pragma unroll 8
    for (int b = 0; b < nb; b++) v += partials[(size_t)b * GM_ROW + c];
    out[c] = v;
}

} // namespace

size_t geometry_reduce_workspace_bytes(int64_t N) { return align_up((size_t)(gm_blocks(N) > 0 ? gm_blocks(N) : 1) * GM_ROW * sizeof(double)); }

void launch_geometry_reduce(int64_t N, const float* d2, const float* points, const float* bounds, float max_dist, int T,
                            const float* thresholds, void* workspace, double* out, hipStream_t s)
{
    GmParams g{};
    g.max_dist = max_dist; g.T = T; g.boxed = (points && bounds) ? 1 : 0;
    for (int a = 0; a < 3 && g.boxed; a++) { g.lo[a] = bounds[a]; g.hi[a] = bounds[3 + a]; }
    for (int t = 0; t < T; t++) g.tau[t] = thresholds[t];
    const int nb = gm_blocks(N);
    if (nb > 0) geometry_partial_kernel<<<nb, GM_BLOCK, 0, s>>>(N, d2, points, g, (double*)workspace);
    geometry_fold_kernel<<<1, 64, 0, s>>>(nb, T, (const double*)workspace, out);
}

} // namespace c3dgs
