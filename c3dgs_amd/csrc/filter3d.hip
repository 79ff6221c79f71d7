// filter3d.hip -- the 3D smoothing filter of Mip-Splatting for gfx950 (no reference counterpart): a per-Gaussian world-space
// low-pass sized by the highest sampling rate (focal / depth) at which any training camera sees the Gaussian, computed by two
// kernels and applied by two more around the unchanged rasterizer.
//
// THE FILTER (filter3d_dist_kernel, filter3d_finish_kernel). Camera c is one 16-float row of a device table:
//     m[0..11] = rows 0..2 of the world -> camera matrix V_c (row-major, 4 entries each), m[12] = fx, m[13] = fy, m[14] = W, m[15] = H.
// For Gaussian i at p, in fp32, every operation rounded on its own in the order written (this file is compiled with
// preprocess.hip's flags: no contraction; division correctly rounded):
//     x = ((m0 px + m1 py) + m2 pz) + m3,  y and z likewise from m4.. and m8..
//     u = (x / z) fx + W 0.5,              v = (y / z) fy + H 0.5
//     valid = z > 0.2 and -0.15 W <= u <= 1.15 W and -0.15 H <= v <= 1.15 H
//     dist_i = min over the valid c of z;  seen_i = some c is valid;  focal = max over ALL c of fx
//     a Gaussian no camera sees takes the maximum of dist over the seen ones, 0 when nobody is seen at all
//     filter_3D_i = (dist_i / focal) float(sqrt(0.2))
// One lane per Gaussian holds p in registers and loops over the table; the camera index is the loop counter and the table a
// const restrict kernel argument, so the rows arrive by scalar loads into SGPRs, any C. The maximum over the seen Gaussians is
// an integer atomicMax on the bit pattern of the positive floats (one per wave, after a wave reduction): order-independent, so
// the whole result is bitwise reproducible. Launches: one 8-byte clear of the workspace, the two kernels; no host read.
//
// APPLY (filter3d_apply_kernel). With f = filter_3D_i (a constant), the row's scales sc_k (its codebook row with g_indices), its
// scale factor sf (1 without g_indices), mod = sf scale_modifier and Sigma = cov3d_from_scale_rot(sc, mod, rot):
//     Sigma' = Sigma + (scale_modifier f)^2 I   (elements 0, 3, 5 of the 6-vector: scale_modifier^2 R diag(s^2 + f^2) R^T for an
//                                               orthonormal R, upstream's s' = sqrt(s^2 + f^2) under the modifier)
//     s_k = sf sc_k,  r_k = s_k^2 / (s_k^2 + f^2)  (1 where f == 0),  coef = sqrt((r_0 r_1) r_2),  o' = o coef
// With a caller's covariance (cov3D_precomp of the rows) Sigma is that covariance, the scales serve the opacity factor alone and
// the rotations are not read; its gradient is dL/dSigma' itself, so the backward then chains g' only.
// A row with f == 0 gets Sigma and o back bit for bit. With `visible` / `rank` (the fused indexed path: the inputs are the
// visible subset, row rank[i] for model row i with visible[i]) the kernel runs one lane per MODEL row and reads filter_3D[i].
//
// BACKWARD (filter3d_apply_backward_kernel), for rows where dL_dcov3D' or g' = dL/do' is non-zero (others are not touched: the
// caller hands in zeros): dL/dSigma = dL/dSigma' element for element, chained to scales, rotations and scale factors by
// gsgrad.hpp's cov3d_grad_to_scale_rot(), which backward_preprocess.hip restates and tests/test_gsgrad_gpu.py holds it to (its
// factor 1/2 on the off-diagonal elements; exact derivatives with respect to the scale_modifier, as aa_opacity.hip has them);
// dL/do = coef g'; dL/ds_k += o g' coef f^2 / (s_k (s_k^2 + f^2)) unless s_k == 0 or f == 0, distributed to sc_k (x sf) and
// sf (x sc_k). All in fp32. P-sized outputs are plain stores (one lane owns one row); the codebook-sized outputs of the indexed form are scatter-ADDED by gsgrad.hpp's scatter_add_scale_rot(), so those rows are
// NOT bitwise reproducible.
#include "common.hpp"
#include "gsgrad.hpp"

namespace c3dgs {

namespace {

constexpr float F3_NEAR = 0.2f;
constexpr float F3_SQRT_02 = 0.44721359549995793f;      // float(sqrt(0.2))

__global__ void __launch_bounds__(256) filter3d_dist_kernel(const int P, const int C, const float* __restrict__ xyz,
                                                            const float* __restrict__ cams, float* __restrict__ dist_out,
                                                            uint32_t* __restrict__ ws)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t si = (size_t)min(i, P - 1);               // lanes past P repeat the last row and write nothing
    const float px = xyz[3 * si], py = xyz[3 * si + 1], pz = xyz[3 * si + 2];
    float dist = INFINITY, focal = -INFINITY;
    for (int c = 0; c < C; c++) {
        const float* __restrict__ m = cams + 16 * (size_t)c;
        const float x = m[0] * px + m[1] * py + m[2] * pz + m[3];
        const float y = m[4] * px + m[5] * py + m[6] * pz + m[7];
        const float z = m[8] * px + m[9] * py + m[10] * pz + m[11];
        const float fx = m[12], fy = m[13], W = m[14], H = m[15];
        const float u = x / z * fx + W * 0.5f;
        const float v = y / z * fy + H * 0.5f;
        const bool valid = z > F3_NEAR && u >= -0.15f * W && u <= 1.15f * W && v >= -0.15f * H && v <= 1.15f * H;
        dist = valid ? fminf(dist, z) : dist;
        focal = fmaxf(focal, fx);
    }
    // the largest dist of the wave's seen rows (z > 0.2: positive floats order like their bit patterns)
    uint32_t top = (i < P && dist < INFINITY) ? __float_as_uint(dist) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, o));
    if ((threadIdx.x & 63) == 0 && top != 0u) atomicMax(ws, top);
    if (i == 0) ws[1] = __float_as_uint(focal);
    if (i < P) dist_out[i] = dist;
}

__global__ void __launch_bounds__(256) filter3d_finish_kernel(const int P, const uint32_t* __restrict__ ws,
                                                              float* __restrict__ filter, uint8_t* __restrict__ seen)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float far = __uint_as_float(ws[0]), focal = __uint_as_float(ws[1]);
    const float d = filter[i];
    const bool s = d < INFINITY;
    filter[i] = (s ? d : far) / focal * F3_SQRT_02;
    if (seen) seen[i] = s ? 1 : 0;
}

struct F3Args {
    int n, P_model;                  // output rows; model rows (the lanes with `visible`)
    const float* opacities; const float* scales; const float* rotations; const float* scale_factors; const int64_t* g_indices;
    const float* cov3D_in;           // the caller's covariance in place of the one scales and rotations build, or null
    const float* filter; const uint8_t* visible; const int32_t* rank;
    float scale_modifier;
};

struct F3Row {
    size_t j;                        // output row
    float f;
    ScaleRotRow g;                   // scales, rotation, codebook row, scale factor; Sigma before the filter
    float s[3], r[3], coef;          // s_k = sf sc_k
};

// lane t -> its output row and filter value; false: the lane has no row
__device__ __forceinline__ bool f3_row(const F3Args& a, const int t, F3Row& w)
{
    if (a.visible) {
        if (t >= a.P_model || !a.visible[t]) return false;
        w.j = (size_t)a.rank[t];
        if (w.j >= (size_t)a.n) return false;
    } else {
        if (t >= a.n) return false;
        w.j = (size_t)t;
    }
    w.f = a.filter[t];
    load_scale_rot_row(a.cov3D_in, a.scales, a.rotations, a.scale_factors, a.g_indices, w.j, a.scale_modifier, w.g);
    const float f2 = w.f * w.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        w.s[k] = w.g.sf * w.g.sc[k];
        const float s2 = w.s[k] * w.s[k];
        w.r[k] = w.f == 0.f ? 1.f : s2 / (s2 + f2);
    }
    w.coef = sqrtf(w.r[0] * w.r[1] * w.r[2]);
    return true;
}

__global__ void __launch_bounds__(256) filter3d_apply_kernel(const F3Args a, float* __restrict__ cov3D_out,
                                                             float* __restrict__ opacity_out)
{
    F3Row w;
    if (!f3_row(a, blockIdx.x * 256 + threadIdx.x, w)) return;
    float* cov = w.g.cov3D;
    float o = a.opacities[w.j];
    if (w.f != 0.f) {
        const float mf = a.scale_modifier * w.f, add = mf * mf;
        cov[0] = cov[0] + add; cov[3] = cov[3] + add; cov[5] = cov[5] + add;
        o = o * w.coef;
    }
#pragma unroll
    for (int q = 0; q < 6; q++) cov3D_out[6 * w.j + q] = cov[q];
    opacity_out[w.j] = o;
}

struct F3Grads {
    const float* dL_dcov3D; const float* dL_dopacity_out;      // in: [n, 6], [n]
    float* dL_dopacity; float* dL_dscales; float* dL_drotations; float* dL_dscale_factors;
};

template <bool INDEXED>
__global__ void __launch_bounds__(256) filter3d_apply_backward_kernel(const F3Args a, const F3Grads o)
{
    // the indexed form parks what goes to the codebook rows here; -1: this lane adds nothing
    __shared__ float s_ds[INDEXED ? 256 : 1][3];
    __shared__ float s_dq[INDEXED ? 256 : 1][4];
    __shared__ int32_t s_gi[INDEXED ? 256 : 1];
    if (INDEXED) s_gi[threadIdx.x] = -1;

    F3Row w;
    if (f3_row(a, blockIdx.x * 256 + threadIdx.x, w)) {
        float dcov[6];
        bool any = false;
#pragma unroll
        for (int q = 0; q < 6; q++) { dcov[q] = o.dL_dcov3D ? o.dL_dcov3D[6 * w.j + q] : 0.f; any |= dcov[q] != 0.f; }   // (null with cov3D_in)
        const float gp = o.dL_dopacity_out ? o.dL_dopacity_out[w.j] : 0.f;
        if (any || gp != 0.f) {
            if (o.dL_dopacity) o.dL_dopacity[w.j] = w.coef * gp;
            // Sigma -> scale / rotation; d_s is with respect to the SCALED scale mod sc_k
            const float mod = w.g.sf * a.scale_modifier;
            const float s[3] = { mod * w.g.sc[0], mod * w.g.sc[1], mod * w.g.sc[2] };
            float d_s[3], dq[4];
            cov3d_grad_to_scale_rot(dcov, s, w.g.rot.x, w.g.rot.y, w.g.rot.z, w.g.rot.w, d_s, dq);
            // through coef, with respect to s_k = sf sc_k: d coef / d s_k = coef f^2 / (s_k (s_k^2 + f^2))
            float d_c[3] = { 0.f, 0.f, 0.f };
            if (w.f != 0.f && gp != 0.f) {
                const float og = a.opacities[w.j] * gp, f2 = w.f * w.f;
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (w.s[k] != 0.f) d_c[k] = og * w.coef * f2 / (w.s[k] * (w.s[k] * w.s[k] + f2));
            }
            // to the row sc_k: d_s mod + d_c sf; to the factor sf: scale_modifier sum d_s sc_k + sum d_c sc_k
            float drow[3];
#pragma unroll
            for (int k = 0; k < 3; k++) drow[k] = d_s[k] * mod + d_c[k] * w.g.sf;
            if (INDEXED) {
#pragma unroll
                for (int q = 0; q < 3; q++) s_ds[threadIdx.x][q] = drow[q];
                s_dq[threadIdx.x][0] = dq[0]; s_dq[threadIdx.x][1] = dq[1]; s_dq[threadIdx.x][2] = dq[2]; s_dq[threadIdx.x][3] = dq[3];
                s_gi[threadIdx.x] = (int32_t)w.g.gi;
                if (o.dL_dscale_factors)
                    o.dL_dscale_factors[w.j] = a.scale_modifier * (d_s[0] * w.g.sc[0] + d_s[1] * w.g.sc[1] + d_s[2] * w.g.sc[2]) +
                                               (d_c[0] * w.g.sc[0] + d_c[1] * w.g.sc[1] + d_c[2] * w.g.sc[2]);
            } else {
                if (o.dL_dscales) { o.dL_dscales[3 * w.j] = drow[0]; o.dL_dscales[3 * w.j + 1] = drow[1]; o.dL_dscales[3 * w.j + 2] = drow[2]; }
                if (o.dL_drotations) *reinterpret_cast<float4*>(o.dL_drotations + 4 * w.j) = make_float4(dq[0], dq[1], dq[2], dq[3]);
            }
        }
    }

    if (INDEXED) {
        // each wave scatter-adds what its own 64 lanes parked: wave-level ordering of the LDS traffic is all that is needed
        wave_lds_fence();
        scatter_add_scale_rot(s_gi, s_ds, s_dq, o.dL_dscales, o.dL_drotations);
    }
}

F3Args f3_args(const c3dgs_filter3d_rows& p)
{
    F3Args a;
    a.n = p.n; a.P_model = p.P_model;
    a.opacities = p.opacities; a.scales = p.scales; a.rotations = p.rotations;
    a.g_indices = p.g_indices; a.scale_factors = p.g_indices ? p.scale_factors : nullptr;
    a.cov3D_in = p.cov3D_precomp;
    a.filter = p.filter_3D; a.visible = p.visible; a.rank = p.visible ? p.rank : nullptr;
    a.scale_modifier = p.scale_modifier;
    return a;
}

} // namespace

void launch_filter3d_dist(int P, int C, const float* xyz, const float* cams, float* filter, uint32_t* ws, hipStream_t s)
{
    filter3d_dist_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, C, xyz, cams, filter, ws);
}

void launch_filter3d_finish(int P, const uint32_t* ws, float* filter, uint8_t* seen, hipStream_t s)
{
    filter3d_finish_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, ws, filter, seen);
}

void launch_filter3d_apply(const c3dgs_filter3d_rows& p, float* cov3D_out, float* opacity_out, hipStream_t s)
{
    const F3Args a = f3_args(p);
    const int lanes = a.visible ? a.P_model : a.n;
    if (lanes <= 0) return;
    filter3d_apply_kernel<<<(lanes + 255) / 256, 256, 0, s>>>(a, cov3D_out, opacity_out);
}

void launch_filter3d_apply_backward(const c3dgs_filter3d_rows& p, const c3dgs_filter3d_grads& g, hipStream_t s)
{
    const F3Args a = f3_args(p);
    const int lanes = a.visible ? a.P_model : a.n;
    if (lanes <= 0) return;
    F3Grads o;
    o.dL_dcov3D = a.cov3D_in ? nullptr : g.dL_dcov3D;       // the caller's covariance takes its gradient as it is, not through here
    o.dL_dopacity_out = g.dL_dopacity_out; o.dL_dopacity = g.dL_dopacity;
    o.dL_dscales = g.dL_dscales; o.dL_drotations = g.dL_drotations; o.dL_dscale_factors = a.g_indices ? g.dL_dscale_factors : nullptr;
    const int grid = (lanes + 255) / 256;
    if (a.g_indices) filter3d_apply_backward_kernel<true><<<grid, 256, 0, s>>>(a, o);
    else filter3d_apply_backward_kernel<false><<<grid, 256, 0, s>>>(a, o);
}

} // namespace c3dgs
