// bilagrid.hip -- per-image colour correction by a bilateral grid (gsplat's lib_bilagrid / fused_bilagrid; a grid of shape
// (1, 1, 1) is upstream 3DGS's per-image 3x4 `exposure`) for gfx950, wave64. Not in the reference. fp32 throughout.
//
// One camera's grid G [12, L, Hg, Wg] holds a row-major 3x4 affine per lattice vertex; pixel (x, y) of rgb [3, H, W] reads it at
//   gx = (x + 0.5) / W (Wg - 1),  gy = (y + 0.5) / H (Hg - 1),  z = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
// with trilinear hat weights (an axis of size 1 weighs 1) and returns A[:, :3] c + A[:, 3].
//
//   slice      one lane per pixel. A workgroup is 256 pixels of one image row: it stages the two lattice rows and the few columns
//              they reach, all levels, in LDS (3 KiB for the default grid at 1080p) and every lane reads its 8 vertices x 12
//              entries from there; where that part would not fit in 48 KiB, through the caches in flat pixel order.
//   gather     dL_dG by VERTEX, not by pixel: workgroup (vertex (j, i), row slab, level chunk) walks the pixels of the vertex's
//              footprint |gx - i| < 1, |gy - j| < 1 inside its slab, keeps w dL_dout_c (r, g, b, 1) for up to 8 luma levels in
//              registers (statically indexed: a level the pixel does not touch gets weight 0), reduces with a fixed xor
//              butterfly and, across the four waves, through LDS in wave order, and writes one row of the partial table.
//              Every row of the table is written, so nothing is cleared. A pixel is read by its 4 (x, y) vertices.
//   fold       one lane per grid element: the slabs' partial rows in slab order. Writes every element; a vertex no pixel
//              touches gets the sum of zeros.
//   rgb        dL_drgb, one lane per pixel, the slice's kernel with another epilogue: A[:, :3]^T dL_dout + (dL/dz)(L - 1)(0.299, 0.587, 0.114), the second term zero
//              where the luma was clamped and for L == 1. Skipped when the image needs no gradient.
//   tv, tv backward   the total variation of [C, 12, L, Hg, Wg]: forward differences squared, summed in double per workgroup
//              and folded in block order by a second launch; the backward is a gather of each element's up to six neighbours.
// No float atomics, global or LDS: every sum has a fixed order, the results are bitwise reproducible.
//
// The lattice coordinate along x and y is formed in INTEGERS: (2x + 1)(Wg - 1) = q 2W + r gives the cell q and the fraction
// r / 2W, so the cell is exact, the fraction carries one rounding of its own size rather than one of gx's size, and forward,
// gather and rgb agree on both bit for bit.
#include "bilagrid.hpp"

namespace c3dgs {

struct BgAxis { int i0, i1; float f; };      // the cell [i0, i1] and the weight f of i1 (1 - f of i0)

// pixel x of n along an axis of ng vertices; inv_d = 1 / (2 n) in double: the quotient's estimate is off by less than 1.
// An axis of size 1 has the one cell [0, 0] with f = 0: i1 never steps outside.
__device__ __forceinline__ BgAxis bg_axis(int x, int n, int ng, double inv_d)
{
    BgAxis a{ 0, 0, 0.f };
    if (ng <= 1) return a;
    const long long num = (2LL * x + 1) * (long long)(ng - 1), d = 2LL * n;       // < 2^32 * 2^31
    long long q = (long long)((double)num * inv_d);
    q = q < 0 ? 0 : (q > ng - 2 ? ng - 2 : q);                                     // num / d < ng - 1: the cell is inside
    long long r = num - q * d;
    if (r < 0 && q > 0) { q--; r += d; }
    else if (r >= d && q < ng - 2) { q++; r -= d; }
    const float f = (float)r / (float)d;
    a.i0 = (int)q; a.i1 = (int)q + 1;
    a.f = fminf(fmaxf(f, 0.f), 1.f);
    return a;
}

struct BgLuma { int k0, k1; float f; bool inside; };   // inside: 0 < luma < 1, where z moves with the colour

__device__ __forceinline__ BgLuma bg_luma(float r, float g, float b, int L)
{
    BgLuma z{ 0, 0, 0.f, false };
    if (L <= 1) return z;
    const float luma = 0.299f * r + 0.587f * g + 0.114f * b;
    z.inside = luma > 0.f && luma < 1.f;
    const float c = fminf(fmaxf(luma, 0.f), 1.f) * (float)(L - 1);                 // fmaxf(NaN, 0) = 0: the index stays inside
    int k = (int)floorf(c);
    k = k < 0 ? 0 : (k > L - 2 ? L - 2 : k);
    z.k0 = k; z.k1 = k + 1;
    z.f = c - (float)k;
    return z;
}

// Where a per-pixel kernel reads the 8 vertices of its cell from: kk selects the luma plane (k0, k1), jj the row (ay.i0, ay.i1),
// ii the column (ax.i0, ax.i1). Through the caches from the grid as it lies in memory, [12, L, Hg, Wg] ...
struct BgGlobalGrid {
    const float* p[2]; size_t o[2][2], row;
    __device__ __forceinline__ BgGlobalGrid(const float* grid, int L, int Hg, int Wg, const BgAxis& ax, const BgAxis& ay, const BgLuma& az)
    {
        const size_t plane = (size_t)Hg * Wg;
        row = plane * L;
        p[0] = grid + (size_t)az.k0 * plane; p[1] = grid + (size_t)az.k1 * plane;
        o[0][0] = (size_t)ay.i0 * Wg + ax.i0; o[0][1] = (size_t)ay.i0 * Wg + ax.i1;
        o[1][0] = (size_t)ay.i1 * Wg + ax.i0; o[1][1] = (size_t)ay.i1 * Wg + ax.i1;
    }
    __device__ __forceinline__ float get(int m, int kk, int jj, int ii) const { return p[kk][m * row + o[jj][ii]]; }
};
// ... or from the part of it a workgroup has staged in LDS (bilagrid_pixel_kernel<., true>): level k at k S, then the two rows, the
// nx columns from i_lo, the 12 entries of a vertex side by side
struct BgStagedGrid {
    const float* p[2]; int o[2][2];
    __device__ __forceinline__ BgStagedGrid(const float* s, int S, int nx, int i_lo, const BgAxis& ax, const BgLuma& az)
    {
        p[0] = s + az.k0 * S; p[1] = s + az.k1 * S;
        int c0 = ax.i0 - i_lo, c1 = ax.i1 - i_lo;
        c0 = c0 < 0 ? 0 : (c0 > nx - 1 ? nx - 1 : c0);                  // inside by construction (bg_staged_columns); stays inside anyway
        c1 = c1 < 0 ? 0 : (c1 > nx - 1 ? nx - 1 : c1);
        o[0][0] = c0 * 12; o[0][1] = c1 * 12; o[1][0] = (nx + c0) * 12; o[1][1] = (nx + c1) * 12;
    }
    __device__ __forceinline__ float get(int m, int kk, int jj, int ii) const { return p[kk][o[jj][ii] + m]; }
};

// A[12] at (z, y, x), and with DZ the difference of the two luma planes dA/dz[12] (bilinear in x, y)
template <bool DZ, class Grid>
__device__ __forceinline__ void bg_interp(const Grid& G, const BgAxis& ax, const BgAxis& ay, const BgLuma& az, float* A, float* dA)
{
    const float wx0 = 1.f - ax.f, wx1 = ax.f, wy0 = 1.f - ay.f, wy1 = ay.f, wz0 = 1.f - az.f, wz1 = az.f;
    const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
#pragma unroll
    for (int m = 0; m < 12; m++) {
        const float lo = w00 * G.get(m, 0, 0, 0) + w01 * G.get(m, 0, 0, 1) + w10 * G.get(m, 0, 1, 0) + w11 * G.get(m, 0, 1, 1);
        const float hi = w00 * G.get(m, 1, 0, 0) + w01 * G.get(m, 1, 0, 1) + w10 * G.get(m, 1, 1, 0) + w11 * G.get(m, 1, 1, 1);
        A[m] = wz0 * lo + wz1 * hi;
        if (DZ) dA[m] = hi - lo;
    }
}

// ------------------------------------------------------------------------------------------------ slice and dL_drgb
// One lane per pixel. BACKWARD: `out` is dL_drgb, else the sliced image (dL_dout unused).
// STAGED: a workgroup is 256 consecutive pixels of ONE image row (segs workgroups per row). They share the two lattice rows
// ay.i0, ay.i1 and, from the first pixel's column i_lo, at most nx columns (bg_staged_columns), so the workgroup copies those
// 12 L 2 nx floats into LDS once, a few loads per lane, in place of 96 loads per lane through L1, which a wave with mixed luma
// spreads over 48 cache lines per pixel (the 12 rows of a vertex lie L Hg Wg floats apart). The level stride S = 1 mod 32 keeps
// lanes that differ in level and column on different banks. Not STAGED (the staged part would not fit): pixels in flat order.
template <bool BACKWARD, bool STAGED>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_pixel_kernel(int H, int W, int L, int Hg, int Wg, int segs, int nx, int S, double inv_2w, double inv_2h,
                      const float* __restrict__ grid, const float* __restrict__ rgb, const float* __restrict__ dL_dout,
                      float* __restrict__ out)
{
    extern __shared__ float s_grid[];
    const size_t hw = (size_t)H * W;
    int x, y, i_lo = 0;
    if (STAGED) {
        y = (int)(blockIdx.x / (unsigned)segs);
        const int x0 = (int)(blockIdx.x - (unsigned)y * (unsigned)segs) * BG_THREADS;
        x = x0 + (int)threadIdx.x;
        i_lo = bg_axis(x0, W, Wg, inv_2w).i0;
    } else {
        const size_t q = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
        if (q >= hw) return;
        y = (int)(q / W); x = (int)(q - (size_t)y * W);
    }
    const BgAxis ay = bg_axis(y, H, Hg, inv_2h);
    if (STAGED) {
        const int n = 12 * L * 2 * nx;
        for (int idx = threadIdx.x; idx < n; idx += BG_THREADS) {
            const int ii = idx % nx;
            int rest = idx / nx;
            const int jj = rest & 1;
            rest >>= 1;
            const int k = rest % L, m = rest / L;
            const int i = i_lo + ii < Wg ? i_lo + ii : Wg - 1, j = jj ? ay.i1 : ay.i0;
            s_grid[k * S + (jj * nx + ii) * 12 + m] = grid[(((size_t)m * L + k) * Hg + j) * Wg + i];
        }
        __syncthreads();
        if (x >= W) return;
    }
    const size_t p = (size_t)y * W + x;
    const float r = rgb[p], g = rgb[hw + p], b = rgb[2 * hw + p];
    const BgAxis ax = bg_axis(x, W, Wg, inv_2w);
    const BgLuma az = bg_luma(r, g, b, L);
    float A[12], dA[12];
    if (STAGED) bg_interp<BACKWARD>(BgStagedGrid(s_grid, S, nx, i_lo, ax, az), ax, ay, az, A, dA);
    else bg_interp<BACKWARD>(BgGlobalGrid(grid, L, Hg, Wg, ax, ay, az), ax, ay, az, A, dA);
    if (!BACKWARD) {
        out[p] = A[0] * r + A[1] * g + A[2] * b + A[3];
        out[hw + p] = A[4] * r + A[5] * g + A[6] * b + A[7];
        out[2 * hw + p] = A[8] * r + A[9] * g + A[10] * b + A[11];
    } else {
        const float d0 = dL_dout[p], d1 = dL_dout[hw + p], d2 = dL_dout[2 * hw + p];
        float dz = 0.f;                                                // dL/dz (L - 1): zero where the clamp holds z still
        if (az.inside)
            dz = (d0 * (dA[0] * r + dA[1] * g + dA[2] * b + dA[3]) + d1 * (dA[4] * r + dA[5] * g + dA[6] * b + dA[7])
                  + d2 * (dA[8] * r + dA[9] * g + dA[10] * b + dA[11])) * (float)(L - 1);
        out[p] = A[0] * d0 + A[4] * d1 + A[8] * d2 + dz * 0.299f;
        out[hw + p] = A[1] * d0 + A[5] * d1 + A[9] * d2 + dz * 0.587f;
        out[2 * hw + p] = A[2] * d0 + A[6] * d1 + A[10] * d2 + dz * 0.114f;
    }
}

// The columns 256 consecutive pixels of a row can reach from their first pixel's cell: the cell index
// floor((2x + 1)(Wg - 1) / 2W) grows by at most floor(255 (Wg - 1) / W) + 1 over 255 pixels, and the last cell has a right vertex.
static int bg_staged_columns(int W, int Wg)
{
    if (Wg <= 1) return 1;
    const long long nx = 255LL * (Wg - 1) / W + 3;
    return nx < Wg ? (int)nx : Wg;
}

template <bool BACKWARD>
static void launch_bilagrid_pixels(int H, int W, int L, int Hg, int Wg, const float* grid, const float* rgb, const float* dL_dout,
                                   float* out, hipStream_t s)
{
    const double iw = 1.0 / (2.0 * W), ih = 1.0 / (2.0 * H);
    const int nx = bg_staged_columns(W, Wg);
    const long long base = 24LL * nx, S = base + (((1 - base) % 32) + 32) % 32;          // >= base, = 1 mod 32
    const long long lds_bytes = (long long)L * S * 4, segs = ((long long)W + BG_THREADS - 1) / BG_THREADS;
    if (lds_bytes <= BG_STAGED_LDS_BYTES && segs * H < (1LL << 31)) {
        bilagrid_pixel_kernel<BACKWARD, true><<<(unsigned)(segs * H), BG_THREADS, (size_t)lds_bytes, s>>>(
            H, W, L, Hg, Wg, (int)segs, nx, (int)S, iw, ih, grid, rgb, dL_dout, out);
    } else {
        const size_t hw = (size_t)H * W;
        bilagrid_pixel_kernel<BACKWARD, false><<<(unsigned)((hw + BG_THREADS - 1) / BG_THREADS), BG_THREADS, 0, s>>>(
            H, W, L, Hg, Wg, 1, nx, (int)S, iw, ih, grid, rgb, dL_dout, out);
    }
}

void launch_bilagrid_slice(int H, int W, int L, int Hg, int Wg, const float* grid, const float* rgb, float* out, hipStream_t s)
{
    launch_bilagrid_pixels<false>(H, W, L, Hg, Wg, grid, rgb, nullptr, out, s);
}

void launch_bilagrid_rgb_backward(int H, int W, int L, int Hg, int Wg, const float* grid, const float* rgb, const float* dL_dout,
                                  float* dL_drgb, hipStream_t s)
{
    launch_bilagrid_pixels<true>(H, W, L, Hg, Wg, grid, rgb, dL_dout, dL_drgb, s);
}

// ------------------------------------------------------------------------------------------------ dL_dgrid: gather by vertex
// the pixels [lo, hi] along an axis that can weigh vertex i (a superset: the weight decides); exact in 64-bit integers
__device__ __forceinline__ void bg_footprint(int i, int n, int ng, int* lo, int* hi)
{
    if (ng <= 1) { *lo = 0; *hi = n - 1; return; }
    const long long den = ng - 1;
    long long a = (long long)(i - 1) * n, b = (long long)(i + 1) * n;
    a = (a >= 0 ? a / den : -((-a + den - 1) / den)) - 1;               // floor - 1
    b = (b + den - 1) / den + 1;                                        // ceil + 1
    *lo = a < 0 ? 0 : (int)a;
    *hi = b > n - 1 ? n - 1 : (int)b;
}

// the weight of vertex i for a pixel whose cell is `a`
__device__ __forceinline__ float bg_weight(const BgAxis& a, int i, int ng)
{
    if (ng <= 1) return 1.f;
    return i == a.i0 ? 1.f - a.f : (i == a.i1 ? a.f : 0.f);
}

template <int LC>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_gather_kernel(int H, int W, int L, int Hg, int Wg, int slabs, int slab_rows, double inv_2w, double inv_2h,
                       const float* __restrict__ rgb, const float* __restrict__ dL_dout, float* __restrict__ partial)
{
    __shared__ float s_red[BG_THREADS / 64][LC * 12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long group = blockIdx.x;
    const int v = (int)(group / slabs), slab = (int)(group - (long long)v * slabs);
    const int j = v / Wg, i = v - j * Wg;
    const int kb = blockIdx.y * LC;
    int x_lo, x_hi, y_lo, y_hi;
    bg_footprint(i, W, Wg, &x_lo, &x_hi);
    bg_footprint(j, H, Hg, &y_lo, &y_hi);
    const long long y_first = (long long)y_lo + (long long)slab * slab_rows;
    long long y_last = y_first + slab_rows - 1;
    if (y_last > y_hi) y_last = y_hi;
    const int ncols = x_hi - x_lo + 1;
    const long long npix = y_last >= y_first ? (y_last - y_first + 1) * ncols : 0;      // <= slab_rows x cols
    const size_t hw = (size_t)H * W;

    float acc[LC][12];
#pragma unroll
    for (int q = 0; q < LC; q++)
#pragma unroll
        for (int m = 0; m < 12; m++) acc[q][m] = 0.f;

    for (long long t = threadIdx.x; t < npix; t += BG_THREADS) {
        const int ry = (int)(t / ncols);
        const int x = x_lo + (int)(t - (long long)ry * ncols), y = (int)y_first + ry;
        const BgAxis ax = bg_axis(x, W, Wg, inv_2w), ay = bg_axis(y, H, Hg, inv_2h);
        const float wxy = bg_weight(ax, i, Wg) * bg_weight(ay, j, Hg);
        if (wxy == 0.f) continue;
        const size_t p = (size_t)y * W + x;
        const float r = rgb[p], g = rgb[hw + p], b = rgb[2 * hw + p];
        const BgLuma az = bg_luma(r, g, b, L);
        const int rel = az.k0 - kb;
        if (rel < -1 || rel >= LC) continue;                            // neither of the pixel's two levels is in this chunk
        const float w0 = L <= 1 ? 1.f : 1.f - az.f, w1 = L <= 1 ? 0.f : az.f;
        const float v0 = wxy * dL_dout[p], v1 = wxy * dL_dout[hw + p], v2 = wxy * dL_dout[2 * hw + p];
#pragma unroll
        for (int q = 0; q < LC; q++) {
            const float w = q == rel ? w0 : (q == rel + 1 ? w1 : 0.f);
            const float c0 = w * v0, c1 = w * v1, c2 = w * v2;
            acc[q][0] += c0 * r; acc[q][1] += c0 * g; acc[q][2] += c0 * b; acc[q][3] += c0;
            acc[q][4] += c1 * r; acc[q][5] += c1 * g; acc[q][6] += c1 * b; acc[q][7] += c1;
            acc[q][8] += c2 * r; acc[q][9] += c2 * g; acc[q][10] += c2 * b; acc[q][11] += c2;
        }
    }
#pragma unroll
    for (int q = 0; q < LC; q++)
#pragma unroll
        for (int m = 0; m < 12; m++) {
            float a = acc[q][m];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
            if (lane == 0) s_red[wave][q * 12 + m] = a;
        }
    __syncthreads();
    if (threadIdx.x < LC * 12) {
        const int q = threadIdx.x / 12, m = threadIdx.x - q * 12, k = kb + q;
        float a = s_red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < BG_THREADS / 64; w++) a += s_red[w][threadIdx.x];
        if (k < L) partial[((size_t)group * L + k) * 12 + m] = a;
    }
}

void launch_bilagrid_gather(int H, int W, int L, int Hg, int Wg, const BilagridPlan& plan, const float* rgb, const float* dL_dout,
                            float* partial, hipStream_t s)
{
    const dim3 grid((unsigned)plan.groups, (unsigned)plan.chunks);
    const double iw = 1.0 / (2.0 * W), ih = 1.0 / (2.0 * H);
#define C3DGS_BG_GATHER(LC)                                                                                                    \
    bilagrid_gather_kernel<LC><<<grid, BG_THREADS, 0, s>>>(H, W, L, Hg, Wg, plan.slabs, plan.slab_rows, iw, ih, rgb, dL_dout, partial)
    switch (plan.lc) {
    case 1: C3DGS_BG_GATHER(1); break;
    case 2: C3DGS_BG_GATHER(2); break;
    case 4: C3DGS_BG_GATHER(4); break;
    default: C3DGS_BG_GATHER(8); break;
    }
#undef C3DGS_BG_GATHER
}

// dL_dgrid[m, k, v] = sum over the slabs, in slab order, of partial[((v slabs + s) L + k) 12 + m]
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_fold_kernel(long long n, int L, long long vertices, int slabs, const float* __restrict__ partial, float* __restrict__ dL_dgrid)
{
    const long long e = (long long)blockIdx.x * BG_THREADS + threadIdx.x;
    if (e >= n) return;
    const long long per_row = (long long)L * vertices;
    const int m = (int)(e / per_row);
    const long long rem = e - (long long)m * per_row;
    const int k = (int)(rem / vertices);
    const long long v = rem - (long long)k * vertices;
    float a = 0.f;
    for (int s = 0; s < slabs; s++) a += partial[((size_t)(v * slabs + s) * L + k) * 12 + m];
    dL_dgrid[e] = a;
}

void launch_bilagrid_fold(int L, int Hg, int Wg, const BilagridPlan& plan, const float* partial, float* dL_dgrid, hipStream_t s)
{
    const long long n = 12LL * L * Hg * Wg;
    bilagrid_fold_kernel<<<(unsigned)((n + BG_THREADS - 1) / BG_THREADS), BG_THREADS, 0, s>>>(n, L, plan.vertices, plan.slabs, partial,
                                                                                             dL_dgrid);
}

// ------------------------------------------------------------------------------------------------ total variation
// the sum of a double over the workgroup, in a fixed order, valid in thread 0
__device__ __forceinline__ double bg_block_sum(double a, double* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    if (lane == 0) s_w[wave] = a;
    __syncthreads();
    double t = s_w[0];
#pragma unroll
    for (int w = 1; w < BG_THREADS / 64; w++) t += s_w[w];
    return t;
}

// sx, sy, sz = 1 / (C 12 x the lattice positions of one camera's differences along the axis), 0 for an axis of size 1
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_tv_kernel(long long n, int L, int Hg, int Wg, const float* __restrict__ X, double sx, double sy, double sz,
                   double* __restrict__ partial)
{
    __shared__ double s_w[BG_THREADS / 64];
    const long long stride = (long long)gridDim.x * BG_THREADS, plane = (long long)Hg * Wg;
    double acc = 0.0;
    for (long long e = (long long)blockIdx.x * BG_THREADS + threadIdx.x; e < n; e += stride) {
        const int i = (int)(e % Wg), j = (int)((e / Wg) % Hg), k = (int)((e / plane) % L);
        const double x = (double)X[e];
        if (i + 1 < Wg) { const double d = (double)X[e + 1] - x; acc += d * d * sx; }
        if (j + 1 < Hg) { const double d = (double)X[e + Wg] - x; acc += d * d * sy; }
        if (k + 1 < L) { const double d = (double)X[e + plane] - x; acc += d * d * sz; }
    }
    const double t = bg_block_sum(acc, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(BG_THREADS)
bilagrid_tv_fold_kernel(int nb, const double* __restrict__ partial, float* __restrict__ out)
{
    __shared__ double s_w[BG_THREADS / 64];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += BG_THREADS) acc += partial[b];
    const double t = bg_block_sum(acc, s_w);
    if (threadIdx.x == 0) out[0] = (float)t;
}

static void bg_tv_scales(int C, int L, int Hg, int Wg, double* sx, double* sy, double* sz)
{
    const double c12 = 12.0 * C;
    *sx = Wg > 1 ? 1.0 / (c12 * L * Hg * (Wg - 1)) : 0.0;
    *sy = Hg > 1 ? 1.0 / (c12 * L * (Hg - 1) * Wg) : 0.0;
    *sz = L > 1 ? 1.0 / (c12 * (L - 1) * Hg * Wg) : 0.0;
}

void launch_bilagrid_tv(int C, int L, int Hg, int Wg, const float* grids, double* partial, float* out, hipStream_t s)
{
    const long long n = (long long)C * 12 * L * Hg * Wg;
    long long nb = (n + BG_TV_PER_BLOCK - 1) / BG_TV_PER_BLOCK;
    if (nb > BG_TV_BLOCKS) nb = BG_TV_BLOCKS;
    double sx, sy, sz;
    bg_tv_scales(C, L, Hg, Wg, &sx, &sy, &sz);
    bilagrid_tv_kernel<<<(unsigned)nb, BG_THREADS, 0, s>>>(n, L, Hg, Wg, grids, sx, sy, sz, partial);
    bilagrid_tv_fold_kernel<<<1, BG_THREADS, 0, s>>>((int)nb, partial, out);
}

// d tv / dX[e] = sum over the axes of 2 s_axis ((X[e] - X[e - 1]) - (X[e + 1] - X[e])), each neighbour where it exists
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_tv_backward_kernel(long long n, int L, int Hg, int Wg, const float* __restrict__ X, float cx, float cy, float cz,
                            const float* __restrict__ dL_dtv, float* __restrict__ dX)
{
    const long long e = (long long)blockIdx.x * BG_THREADS + threadIdx.x;
    if (e >= n) return;
    const long long plane = (long long)Hg * Wg;
    const int i = (int)(e % Wg), j = (int)((e / Wg) % Hg), k = (int)((e / plane) % L);
    const float x = X[e];
    float t = 0.f;
    if (i > 0) t += cx * (x - X[e - 1]);
    if (i + 1 < Wg) t -= cx * (X[e + 1] - x);
    if (j > 0) t += cy * (x - X[e - Wg]);
    if (j + 1 < Hg) t -= cy * (X[e + Wg] - x);
    if (k > 0) t += cz * (x - X[e - plane]);
    if (k + 1 < L) t -= cz * (X[e + plane] - x);
    dX[e] = dL_dtv[0] * t;
}

void launch_bilagrid_tv_backward(int C, int L, int Hg, int Wg, const float* grids, const float* dL_dtv, float* dL_dgrids, hipStream_t s)
{
    const long long n = (long long)C * 12 * L * Hg * Wg;
    double sx, sy, sz;
    bg_tv_scales(C, L, Hg, Wg, &sx, &sy, &sz);
    bilagrid_tv_backward_kernel<<<(unsigned)((n + BG_THREADS - 1) / BG_THREADS), BG_THREADS, 0, s>>>(
        n, L, Hg, Wg, grids, (float)(2.0 * sx), (float)(2.0 * sy), (float)(2.0 * sz), dL_dtv, dL_dgrids);
}

} // namespace c3dgs
