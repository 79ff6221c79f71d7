// normals.hip -- the per-Gaussian passes and the image stencil of the normal maps, for gfx950. The reference's rasterizer has no
// counterpart. (The two blend replays are render_normal.hip and render_maps_backward.hip.)
//
//   gaussian_normals_kernel        one lane per Gaussian, behind preprocess on the forward's stream: n_g (gsgrad.hpp: the
//                                  shortest axis in view space, facing the camera) -> out[g] = {n_x, n_y, n_z, sigma (m + 1)},
//                                  so that the backward re-derives neither the axis nor the sign. EVERY row is written, the rows
//                                  preprocess culled included: they hold the definition's value for the Gaussian as well.
//   normal_backward_fold_kernel    behind backward_preprocess, beside depth_backward_fold_kernel (render_maps_backward.hip, whose
//                                  lists, grid and time-out rule it has): one lane per LISTED Gaussian folds the flagged slots of
//                                  its run of the dn plane, dL/dn_g = sum over tiles of sum_pix w gN, chains it to the quaternion
//                                  (gsgrad.hpp: normal_grad_to_quat) and ADDS into dL_drotations: the Gaussian's own row, or
//                                  with g_indices the codebook row through scatter_add_scale_rot().
//   depth_to_normal_kernel         one thread per pixel: the normal of the surface z(x, y) of view-space depths,
//   depth_to_normal_backward_kernel    P(x, y) = z(x, y) ((x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, 1), fx = W / (2 tan_fovx)
//                                  (the inverse of gsmath.hpp's ndc2pix); interior pixels
//                                  n = normalize(cross(P(x, y + 1) - P(x, y - 1), P(x + 1, y) - P(x - 1, y))), c / max(|c|, 1e-12),
//                                  the one-pixel border 0. The backward is a GATHER: a pixel re-evaluates the at most four
//                                  stencils that read it. No atomics; both are bitwise reproducible.
#include "common.hpp"
#include "gsgrad.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

__global__ void __launch_bounds__(256)
gaussian_normals_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                        const int64_t* __restrict__ g_indices, const float* __restrict__ view, float4* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t gi = g_indices ? (size_t)g_indices[i] : (size_t)i;
    const int m = smallest_axis(scales[3 * gi], scales[3 * gi + 1], scales[3 * gi + 2]);
    const float4 q = *reinterpret_cast<const float4*>(rotations + 4 * gi);
    float v[3];
    normal_from_quat(q.x, q.y, q.z, q.w, m, view, v);
    const f3 mean = { means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2] };
    const f3 p = xform4x3(mean, view);
    const float sigma = (v[0] * p.x + v[1] * p.y + v[2] * p.z > 0.f) ? -1.f : 1.f;
    out[i] = make_float4(sigma * v[0], sigma * v[1], sigma * v[2], sigma * (float)(m + 1));
}

// what a slot of the dn plane holds, with the three helpers fold_slot_run() asks for
__device__ __forceinline__ void fold_zero(NormalSlot& v) { v.x = 0.f; v.y = 0.f; v.z = 0.f; }
__device__ __forceinline__ void fold_add(NormalSlot& acc, const NormalSlot& v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; }
__device__ __forceinline__ NormalSlot fold_shfl_xor(const NormalSlot& v, int o)
{
    NormalSlot r = { __shfl_xor(v.x, o), __shfl_xor(v.y, o), __shfl_xor(v.z, o) };
    return r;
}

__global__ void __launch_bounds__(256)
normal_backward_fold_kernel(int P, const uint32_t* __restrict__ live_count, const uint32_t* __restrict__ live_ids,
                            const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base,
                            const NormalSlot* __restrict__ dn_plane, const uint8_t* __restrict__ touched,
                            const float4* __restrict__ normals, const float* __restrict__ rotations,
                            const int64_t* __restrict__ g_indices, const float* __restrict__ view, float* __restrict__ dL_drotations,
                            const uint32_t* __restrict__ sort_err)
{
    __shared__ float s_dq[256][4];
    __shared__ int32_t s_gi[256];
    const ListedGaussian lg = listed_gaussian(live_count, live_ids);
    if (!lg.wave_has_work) return;
    const int i = lg.i, lane = threadIdx.x & 63;
    const bool mine = lg.live && i < P;
    const bool poisoned = *sort_err != 0u;
    NormalSlot sum = { 0.f, 0.f, 0.f };
    if (!poisoned) {
        SlotRun run = { 0u, 0u };
        if (mine) run = slot_run(i, inst_offset, block_base);
        sum = fold_slot_run(run, dn_plane, touched, lane);
    }
    s_gi[threadIdx.x] = -1;
    if (mine) {
        const size_t gi = g_indices ? (size_t)g_indices[i] : (size_t)i;
        const float4 q = *reinterpret_cast<const float4*>(rotations + 4 * gi);
        const float w = normals[i].w;                            // sigma (m + 1)
        const int m = (int)fabsf(w) - 1;
        const float g[3] = { sum.x, sum.y, sum.z };
        float dq[4];
        normal_grad_to_quat(q.x, q.y, q.z, q.w, m, w < 0.f ? -1.f : 1.f, view, g, dq);
        if (poisoned) dq[0] = dq[1] = dq[2] = dq[3] = __uint_as_float(0x7fc00000u);
        if (g_indices) {
            s_gi[threadIdx.x] = (int32_t)gi;
#pragma unroll
            for (int c = 0; c < 4; c++) s_dq[threadIdx.x][c] = dq[c];
        } else {
            float* dst = dL_drotations + 4 * (size_t)i;
#pragma unroll
            for (int c = 0; c < 4; c++) dst[c] += dq[c];
        }
    }
    if (g_indices) {
        wave_lds_fence();
        scatter_add_scale_rot(s_gi, nullptr, s_dq, nullptr, dL_drotations);
    }
}

// ---- the stencil
// a = P(x, y + 1) - P(x, y - 1), b = P(x + 1, y) - P(x - 1, y) of the interior pixel (x, y)
__device__ __forceinline__ void stencil_edges(const float* __restrict__ z, int W, int H, float rfx, float rfy, int x, int y,
                                              float a[3], float b[3])
{
    // pixel centres about the principal point are exact in fp32; each ray coordinate is one product with 1 / f
    const float hx = (float)x + 0.5f - 0.5f * (float)W, hy = (float)y + 0.5f - 0.5f * (float)H;
    const float zu = z[(size_t)W * (y - 1) + x], zd = z[(size_t)W * (y + 1) + x];
    const float zl = z[(size_t)W * y + x - 1], zr = z[(size_t)W * y + x + 1];
    a[2] = zd - zu; a[0] = (hx * rfx) * a[2]; a[1] = ((hy + 1.0f) * rfy) * zd - ((hy - 1.0f) * rfy) * zu;
    b[2] = zr - zl; b[1] = (hy * rfy) * b[2]; b[0] = ((hx + 1.0f) * rfx) * zr - ((hx - 1.0f) * rfx) * zl;
}
__device__ __forceinline__ void cross3(const float a[3], const float b[3], float c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ void __launch_bounds__(256)
depth_to_normal_kernel(int W, int H, const float* __restrict__ z, float rfx, float rfy, float* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    float n[3] = { 0.f, 0.f, 0.f };
    if (x >= 1 && y >= 1 && x < W - 1 && y < H - 1) {
        float a[3], b[3], c[3];
        stencil_edges(z, W, H, rfx, rfy, x, y, a, b);
        cross3(a, b, c);
        const float len = fmaxf(sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), 1e-12f);
        n[0] = c[0] / len; n[1] = c[1] / len; n[2] = c[2] / len;
    }
    const size_t n_pix = (size_t)W * H, pix = (size_t)W * y + x;
    out[pix] = n[0]; out[n_pix + pix] = n[1]; out[2 * n_pix + pix] = n[2];
}

// the stencil centred at interior (cx, cy) with the gradient g of its normal: ga = dL/da, gb = dL/db
__device__ __forceinline__ void stencil_grad(const float* __restrict__ z, const float* __restrict__ gN, int W, int H, float rfx,
                                             float rfy, int cx, int cy, float ga[3], float gb[3])
{
    float a[3], b[3], c[3], gc[3];
    stencil_edges(z, W, H, rfx, rfy, cx, cy, a, b);
    cross3(a, b, c);
    const size_t n_pix = (size_t)W * H, pix = (size_t)W * cy + cx;
    const float g[3] = { gN[pix], gN[n_pix + pix], gN[2 * n_pix + pix] };
    const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (len > 1e-12f) {
        const float n[3] = { c[0] / len, c[1] / len, c[2] / len };
        const float d = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
#pragma unroll
        for (int k = 0; k < 3; k++) gc[k] = (g[k] - n[k] * d) / len;
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) gc[k] = g[k] / 1e-12f;
    }
    cross3(b, gc, ga);
    cross3(gc, a, gb);
}

__global__ void __launch_bounds__(256)
depth_to_normal_backward_kernel(int W, int H, const float* __restrict__ z, const float* __restrict__ gN, float rfx, float rfy,
                                float* __restrict__ dL_dz)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    float gp[3] = { 0.f, 0.f, 0.f };                             // dL/dP(x, y)
    float ga[3], gb[3];
    const bool col_in = x >= 1 && x < W - 1, row_in = y >= 1 && y < H - 1;
    if (col_in && y - 1 >= 1 && y - 1 < H - 1) {                 // the stencil above reads this pixel as P(cx, cy + 1)
        stencil_grad(z, gN, W, H, rfx, rfy, x, y - 1, ga, gb);
        gp[0] += ga[0]; gp[1] += ga[1]; gp[2] += ga[2];
    }
    if (col_in && y + 1 >= 1 && y + 1 < H - 1) {                 // the one below as P(cx, cy - 1)
        stencil_grad(z, gN, W, H, rfx, rfy, x, y + 1, ga, gb);
        gp[0] -= ga[0]; gp[1] -= ga[1]; gp[2] -= ga[2];
    }
    if (row_in && x - 1 >= 1 && x - 1 < W - 1) {                 // the one to the left as P(cx + 1, cy)
        stencil_grad(z, gN, W, H, rfx, rfy, x - 1, y, ga, gb);
        gp[0] += gb[0]; gp[1] += gb[1]; gp[2] += gb[2];
    }
    if (row_in && x + 1 >= 1 && x + 1 < W - 1) {                 // the one to the right as P(cx - 1, cy)
        stencil_grad(z, gN, W, H, rfx, rfy, x + 1, y, ga, gb);
        gp[0] -= gb[0]; gp[1] -= gb[1]; gp[2] -= gb[2];
    }
    const float rx = ((float)x + 0.5f - 0.5f * (float)W) * rfx, ry = ((float)y + 0.5f - 0.5f * (float)H) * rfy;
    dL_dz[(size_t)W * y + x] = rx * gp[0] + ry * gp[1] + gp[2];
}

void launch_gaussian_normals(int P, const float* means3D, const float* scales, const float* rotations, const int64_t* g_indices,
                             const float* view, float* out, hipStream_t s)
{
    if (P <= 0) return;
    gaussian_normals_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, means3D, scales, rotations, g_indices, view,
                                                            reinterpret_cast<float4*>(out));
}

void launch_normal_backward_fold(int P, const GeomPtrs& g, const BwdPtrs& w, const NormalSlot* dn_plane, const float* normals,
                                 const float* rotations, const int64_t* g_indices, const float* view, float* dL_drotations,
                                 const uint32_t* sort_err, hipStream_t s)
{
    if (P <= 0) return;
    const int n_lists = (P + BWD_LIST - 1) / BWD_LIST;
    normal_backward_fold_kernel<<<n_lists * (BWD_LIST / 256), 256, 0, s>>>(P, w.live_count, w.live_ids, g.inst_offset, g.block_base,
                                                                           dn_plane, w.touched,
                                                                           reinterpret_cast<const float4*>(normals), rotations,
                                                                           g_indices, view, dL_drotations, sort_err);
}

static inline dim3 stencil_grid(int W, int H) { return dim3((W + 63) / 64, (H + 3) / 4); }

void launch_depth_to_normal(int W, int H, const float* z, float tan_fovx, float tan_fovy, float* out, hipStream_t s)
{
    const float fx = W / (2.0f * tan_fovx), fy = H / (2.0f * tan_fovy);
    depth_to_normal_kernel<<<stencil_grid(W, H), 256, 0, s>>>(W, H, z, 1.0f / fx, 1.0f / fy, out);
}

void launch_depth_to_normal_backward(int W, int H, const float* z, const float* dL_dnormal, float tan_fovx, float tan_fovy,
                                     float* dL_dz, hipStream_t s)
{
    const float fx = W / (2.0f * tan_fovx), fy = H / (2.0f * tan_fovy);
    depth_to_normal_backward_kernel<<<stencil_grid(W, H), 256, 0, s>>>(W, H, z, dL_dnormal, 1.0f / fx, 1.0f / fy, dL_dz);
}

} // namespace c3dgs
