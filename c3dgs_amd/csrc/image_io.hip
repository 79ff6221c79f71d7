// image_io.hip -- the ground-truth image of a camera (scene/cameras.py:67-92, Camera.original_image): decoded 8-bit texels
// [Hs][Ws][C] -> planar fp32 [3][Hd][Wd] in [0, 1] at the camera's resolution, in ONE pass. The reference does this on the host per
// access (decode, to float, premultiply alpha, flip, cv2.resize, permute, clamp); here the bytes are on the device once and
// this kernel is everything between them and the loss (DESIGN.md "Ground-truth images").
//
// The contract (include/c3dgs_hip.h), every step one separately rounded fp32 operation unless fp64 is stated:
//     texel     v = fl(float(u) / 255)                          correctly rounded
//     alpha     a = fl(float(u_a) / 255), v = v * a             C == 4
//     bg        v = v * a + bg[c] * (1 - a)                     C == 4 and bg given
//     flip      texel (y, x) is read from (Hs-1-y, Ws-1-x)      an index remap in front of the resize
//     resize    OpenCV's documented INTER_LINEAR: per axis, in fp64, scale = 1 / (dst / src), f = float((d + 0.5) * scale - 0.5),
//               s = floor(f), f -= s, clamped to the edge with weight 0; horizontal pass on both rows, then the vertical pass
//     output    clamp to [0, 1], planar
// Compiled with -ffp-contract=off, so a * b + c stays two roundings.
//
// fl(u / 255) without a division: q = fl(u * r), e = fma(-q, 255, u) (exact), result = fma(e, r, q) with r = fl(1 / 255) is the
// correctly rounded quotient for every u in 0..255 (checked exhaustively in rational arithmetic, tests/test_image_ref_cpu.py);
// the 64 quotients a lane needs would otherwise be 64 division sequences and the VALU, not HBM, would set the time.
//
// Work split: 256 threads = 64 lanes x 4 rows; a lane owns four consecutive output pixels of one row, so each plane leaves
// as one 16-byte store per lane (scalar stores where the row ends inside the four or the address is not 16-byte aligned).
// Source texels are fetched as the ALIGNED dwords that hold them (one, or two when the texel straddles a dword boundary):
// never three byte loads per tap. Every dword read holds at least one byte of `src`, so no page `src` does not own is
// touched, whatever the alignment of `src`; nothing outside `out` is written. Byte offsets into `src` are 64-bit.
// fp64: the two scales are formed on the host; a lane does one multiply and one subtract per axis coordinate.
// No LDS, no atomics: bit-identical from run to run.
#include "common.hpp"

namespace c3dgs {

constexpr int IO_PX = 4;          // output pixels of one lane
constexpr int IO_ROWS = 4;        // output rows of one workgroup (one per wave)

__device__ __forceinline__ float io_unit(uint32_t u)            // fl(float(u) / 255), u in 0..255
{
    const float r = 0x1.010102p-8f;                             // fl(1 / 255)
    const float x = (float)u, q = x * r;
    return __fmaf_rn(__fmaf_rn(-q, 255.0f, x), r, q);
}

// the C bytes at src + off, in the low bits, from the aligned dwords that hold them
template <int C>
__device__ __forceinline__ uint32_t io_fetch(const uint8_t* __restrict__ src, long long off)
{
    const uintptr_t a = (uintptr_t)src + (uintptr_t)off;
    const uint32_t* p = (const uint32_t*)(a & ~(uintptr_t)3);
    const uint32_t sh = ((uint32_t)a & 3u) * 8u;
    const uint32_t w0 = p[0];
    const uint32_t w1 = (sh + 8u * C > 32u) ? p[1] : 0u;        // only when a byte of the texel lives there
    return (uint32_t)(((((uint64_t)w1) << 32) | w0) >> sh);
}

template <int C, bool BG>
__device__ __forceinline__ void io_texel(uint32_t bits, const float (&bg)[3], float (&v)[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = io_unit((bits >> (8 * c)) & 255u);
    if (C == 4) {
        const float a = io_unit(bits >> 24), na = 1.0f - a;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[c] = v[c] * a;
            if (BG) v[c] = v[c] + bg[c] * na;
        }
    }
}

// source tap and weight of destination coordinate d on an axis of `n` source texels (cv::resize, INTER_LINEAR)
__device__ __forceinline__ void io_tap(int d, double scale, int n, int& s0, int& s1, float& f)
{
    f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    int s = (int)fl;
    f -= fl;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= n - 1) { s = n - 1; f = 0.0f; }
    s0 = s;
    s1 = s + 1 < n ? s + 1 : n - 1;
}

template <int C, bool BG>
__global__ void __launch_bounds__(64 * IO_ROWS)
image_from_u8_kernel(int Hs, int Ws, const uint8_t* __restrict__ src, int flip, const float* __restrict__ bgp, int Hd, int Wd,
                     double scale_y, double scale_x, float* __restrict__ out)
{
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * IO_PX;
    const int y = blockIdx.y * IO_ROWS + (threadIdx.x >> 6);
    if (x0 >= Wd || y >= Hd) return;
    float bg[3] = { 0.0f, 0.0f, 0.0f };
    if (BG) { bg[0] = bgp[0]; bg[1] = bgp[1]; bg[2] = bgp[2]; }

    int r0, r1;
    float fy;
    io_tap(y, scale_y, Hs, r0, r1, fy);
    if (flip) { r0 = Hs - 1 - r0; r1 = Hs - 1 - r1; }
    const long long row0 = (long long)r0 * Ws, row1 = (long long)r1 * Ws;
    const float gy = 1.0f - fy;

    float o[3][IO_PX];
#pragma unroll
    for (int k = 0; k < IO_PX; k++) {
        const int x = x0 + k < Wd ? x0 + k : Wd - 1;            // lanes past the row end repeat its last pixel and store nothing
        int c0, c1;
        float fx;
        io_tap(x, scale_x, Ws, c0, c1, fx);
        if (flip) { c0 = Ws - 1 - c0; c1 = Ws - 1 - c1; }
        const float gx = 1.0f - fx;
        float t00[3], t01[3], t10[3], t11[3];
        io_texel<C, BG>(io_fetch<C>(src, (row0 + c0) * C), bg, t00);
        io_texel<C, BG>(io_fetch<C>(src, (row0 + c1) * C), bg, t01);
        io_texel<C, BG>(io_fetch<C>(src, (row1 + c0) * C), bg, t10);
        io_texel<C, BG>(io_fetch<C>(src, (row1 + c1) * C), bg, t11);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float h0 = t00[c] * gx + t01[c] * fx;
            const float h1 = t10[c] * gx + t11[c] * fx;
            const float v = h0 * gy + h1 * fy;
            o[c][k] = fminf(fmaxf(v, 0.0f), 1.0f);
        }
    }

    const int n = Wd - x0 < IO_PX ? Wd - x0 : IO_PX;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float* p = out + ((size_t)c * Hd + y) * Wd + x0;
        if (n == IO_PX && ((uintptr_t)p & 15) == 0) {
            *(float4*)p = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < IO_PX; k++)
                if (k < n) p[k] = o[c][k];
        }
    }
}

void launch_image_from_u8(int Hs, int Ws, int C, const uint8_t* src, int flip, const float* bg, int Hd, int Wd, float* out,
                          hipStream_t s)
{
    const double scale_y = 1.0 / ((double)Hd / (double)Hs), scale_x = 1.0 / ((double)Wd / (double)Ws);
    const dim3 grid((Wd + 64 * IO_PX - 1) / (64 * IO_PX), (Hd + IO_ROWS - 1) / IO_ROWS);
    const dim3 block(64 * IO_ROWS);
    if (C == 3)
        image_from_u8_kernel<3, false><<<grid, block, 0, s>>>(Hs, Ws, src, flip, nullptr, Hd, Wd, scale_y, scale_x, out);
    else if (bg)
        image_from_u8_kernel<4, true><<<grid, block, 0, s>>>(Hs, Ws, src, flip, bg, Hd, Wd, scale_y, scale_x, out);
    else
        image_from_u8_kernel<4, false><<<grid, block, 0, s>>>(Hs, Ws, src, flip, nullptr, Hd, Wd, scale_y, scale_x, out);
}

} // namespace c3dgs
