// metrics.hip -- forward-only, batched image metrics of the evaluation pass for gfx950 (hot loop D).
//
//   reference: utils/image_utils.py:17-19 (psnr) and utils/loss_utils.py:33-63 (ssim), as compress.py:121-163 calls them
//
// For a batch img, gt : [N, C, H, W] (fp32, contiguous) one row per image, in float64:
//   out[n] = { mean (img - gt)^2,  mean ssim_map(img, gt),  mean |img - gt| }
// SSIM: 11-tap Gaussian window sigma 1.5 normalised in fp32, zero padding 5 per channel, C1 = 0.01^2, C2 = 0.03^2.
//
// Pass 1 (metrics_tile_kernel): a 256-thread workgroup owns a 32 x 22 output tile of one (image, channel) plane, stages
// the 42 x 32 halo of both images in LDS, applies the separable window to the five moments {x, y, x^2, y^2, xy} with
// register-sliding windows (the tiling of loss.hip's forward), and sums the SSIM map, (x - y)^2 and |x - y| over its
// tile. Nothing per pixel is written: only three float64 partials per workgroup, to caller-owned scratch.
// Pass 2 (metrics_reduce_kernel): one workgroup per image adds that image's partials in a fixed order. No float atomics:
// results are bit-identical from run to run, and an image's row does not depend on the rest of the batch.
#include "common.hpp"
#include <cmath>

namespace c3dgs {
namespace {

constexpr int MR = 5;             // window radius (window_size 11)
constexpr int MW = 32, MH = 22, MHALO_W = MW + 2 * MR, MHALO_H = MH + 2 * MR;   // 42 x 32 halo
static_assert(MHALO_H * (MW / 4) == 256, "one horizontal task per thread");
constexpr int MREDUCE = 1024;

struct MetricWindow { float g[11]; };

// gaussian(11, 1.5) normalised in fp32 (utils/loss_utils.py:23-25): fp32 taps over their fp32 sum; torch's sum of the
// 11 taps is the correctly rounded one (a running fp32 sum is 1 ulp lower), so the sum is taken in double and rounded once
MetricWindow metric_window()
{
    MetricWindow w;
    double s = 0.0;
    for (int i = 0; i < 11; i++) { w.g[i] = (float)std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += w.g[i]; }
    const float sf = (float)s;
    for (int i = 0; i < 11; i++) w.g[i] = w.g[i] / sf;
    return w;
}

__global__ void __launch_bounds__(256)
metrics_tile_kernel(int H, int W, int tiles_x, int tiles_per_plane, const float* __restrict__ img, const float* __restrict__ gt,
                    const MetricWindow win, double* __restrict__ partials /*[planes * tiles_per_plane][3]*/)
{
    __shared__ float s_x[MHALO_H][MHALO_W + 1];
    __shared__ float s_y[MHALO_H][MHALO_W + 1];
    __shared__ float s_h[5][MHALO_H][MW + 1];     // horizontally filtered moments
    __shared__ double s_red[3][4];

    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    const int64_t plane_id = blk / tiles_per_plane;
    const int t = (int)(blk - plane_id * tiles_per_plane);
    const int tyi = t / tiles_x;
    const int x0 = (t - tyi * tiles_x) * MW, y0 = tyi * MH;
    const size_t plane = (size_t)plane_id * H * W;

    for (int q = tid; q < MHALO_H * MHALO_W; q += 256) {
        const int r = q / MHALO_W, col = q - r * MHALO_W;
        const int yy = y0 + r - MR, xx = x0 + col - MR;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;          // zero padding (padding = window_size // 2)
        s_x[r][col] = in ? img[plane + (size_t)yy * W + xx] : 0.f;
        s_y[r][col] = in ? gt[plane + (size_t)yy * W + xx] : 0.f;
    }
    __syncthreads();
    {   // horizontal pass: thread = (halo row, group of 4 output columns); 14 inputs feed 4 outputs
        const int r = tid >> 3, cg = (tid & 7) * 4;
        float xv[14], yv[14];
#pragma unroll
        for (int j = 0; j < 14; j++) { xv[j] = s_x[r][cg + j]; yv[j] = s_y[r][cg + j]; }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float g = win.g[k], x = xv[o + k], y = yv[o + k];
                a0 = fmaf(g, x, a0); a1 = fmaf(g, y, a1);
                a2 = fmaf(g, x * x, a2); a3 = fmaf(g, y * y, a3); a4 = fmaf(g, x * y, a4);
            }
            s_h[0][r][cg + o] = a0; s_h[1][r][cg + o] = a1; s_h[2][r][cg + o] = a2; s_h[3][r][cg + o] = a3; s_h[4][r][cg + o] = a4;
        }
    }
    __syncthreads();
    // vertical pass: thread = (column, group of 3 output rows); 13 rows feed 3 outputs
    const int tx = tid & 31, rg = (tid >> 5) * 3;
    double sqv = 0.0, ssv = 0.0, l1v = 0.0;
    float hv[5][13];
#pragma unroll
    for (int m = 0; m < 5; m++)
#pragma unroll
        for (int j = 0; j < 13; j++) hv[m][j] = (rg + j < MHALO_H) ? s_h[m][rg + j][tx] : 0.f;
#pragma unroll
    for (int o = 0; o < 3; o++) {
        const int ty = rg + o;
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float g = win.g[k];
            mu1 = fmaf(g, hv[0][o + k], mu1); mu2 = fmaf(g, hv[1][o + k], mu2);
            e11 = fmaf(g, hv[2][o + k], e11); e22 = fmaf(g, hv[3][o + k], e22);
            e12 = fmaf(g, hv[4][o + k], e12);
        }
        if (ty < MH && x0 + tx < W && y0 + ty < H) {
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;              // loss_utils.py:54-55
            const float s1 = e11 - mu1 * mu1, s2 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
            const float num = (2.f * mu1 * mu2 + C1) * (2.f * s12 + C2);
            const float den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2);
            ssv += (double)(num / den);                                        // loss_utils.py:57
            const float d = s_x[ty + MR][tx + MR] - s_y[ty + MR][tx + MR];
            sqv += (double)(d * d);
            l1v += (double)fabsf(d);
        }
    }
    // fixed-order block reduction -> three partials of this workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sqv += __shfl_xor(sqv, o); ssv += __shfl_xor(ssv, o); l1v += __shfl_xor(l1v, o); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = sqv; s_red[1][tid >> 6] = ssv; s_red[2][tid >> 6] = l1v; }
    __syncthreads();
    if (tid < 3) partials[blk * 3 + tid] = (s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]);
}

// one workgroup per image: its C * tiles_per_plane partial rows, summed in a fixed order, divided by C * H * W
// (adding 0.0 for a missing row leaves a sum unchanged, so the order is that of the rows alone)
__global__ void __launch_bounds__(MREDUCE)
metrics_reduce_kernel(int rows_per_image, double inv_count, const double* __restrict__ partials, double* __restrict__ out)
{
    __shared__ double s_red[3][MREDUCE / 64];
    const int tid = threadIdx.x;
    const double* p = partials + (size_t)blockIdx.x * rows_per_image * 3;
    double a = 0.0, b = 0.0, c = 0.0;
    // four rows in flight per thread (loads first, then the adds in row order): latency, not bandwidth, bounds this loop
    for (int i0 = tid; i0 < rows_per_image; i0 += 4 * MREDUCE) {
        double v[4][3];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * MREDUCE;
            const bool in = i < rows_per_image;
            v[u][0] = in ? p[3 * i] : 0.0; v[u][1] = in ? p[3 * i + 1] : 0.0; v[u][2] = in ? p[3 * i + 2] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { a += v[u][0]; b += v[u][1]; c += v[u][2]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = a; s_red[1][tid >> 6] = b; s_red[2][tid >> 6] = c; }
    __syncthreads();
    if (tid < 3) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < MREDUCE / 64; w++) v += s_red[tid][w];
        out[(size_t)blockIdx.x * 3 + tid] = v * inv_count;
    }
}

} // namespace

// N * C planes of tiles_per_plane workgroups each; 0 for non-positive sizes, and INT64_MAX when the count overflows
// (c_abi.hip calls this on unvalidated sizes)
int64_t image_metrics_workgroups(int N, int C, int H, int W)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t planes = (int64_t)N * C;                                            // < 2^62
    const int64_t tiles = (((int64_t)W + MW - 1) / MW) * (((int64_t)H + MH - 1) / MH);   // < 2^53
    return tiles > INT64_MAX / planes ? INT64_MAX : planes * tiles;
}

size_t image_metrics_ws_bytes(int N, int C, int H, int W)
{
    const int64_t wg = image_metrics_workgroups(N, C, H, W);
    return wg <= IMAGE_METRICS_MAX_WORKGROUPS ? (size_t)wg * 3 * sizeof(double) : 0;
}

void launch_image_metrics(int N, int C, int H, int W, const float* img, const float* gt, double* partials, double* out,
                          hipStream_t s)
{
    static const MetricWindow win = metric_window();
    const int tiles_x = (W + MW - 1) / MW, tiles_per_plane = tiles_x * ((H + MH - 1) / MH);
    const int64_t blocks = (int64_t)N * C * tiles_per_plane;
    metrics_tile_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>(H, W, tiles_x, tiles_per_plane, img, gt, win, partials);
    metrics_reduce_kernel<<<N, MREDUCE, 0, s>>>(C * tiles_per_plane, 1.0 / ((double)C * H * W), partials, out);
}

} // namespace c3dgs
