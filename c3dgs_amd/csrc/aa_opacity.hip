// aa_opacity.hip -- antialiased rasterization for gfx950: the opacity compensation of the 0.3 px^2 low-pass, two kernels
// around the unchanged rasterizer (no reference counterpart; upstream 3DGS `antialiasing`, Mip-Splatting, gsplat "antialiased").
// cov2d() dilates every projected covariance by h = 0.3 and leaves the opacity alone, so a Gaussian far smaller than a pixel is
// drawn with the energy of a much larger one. With (a0, b, c0) the covariance BEFORE the low-pass (gsmath.hpp: cov2d_raw),
//     D0 = a0 c0 - b b,   D1 = (a0 + h)(c0 + h) - b b,   r = D0 / D1,   rho = sqrt(max(0.000025, r)),   o' = o rho
// and the rasterizer runs on o'. rho depends on the per-Gaussian projection alone, so the forward takes o' as its opacity input
// and the backward's dL/do' is chained here:
//   aa_opacity_kernel           (one lane per Gaussian, all P, no LDS): o'[P] and, when asked, rho[P];
//   aa_opacity_backward_kernel  (one lane per Gaussian, working where radii > 0 and g' != 0, behind the whole backward on its stream): rewrites
//       dL_dopacity = rho g' in place and ADDS the terms through rho (dL/drho = o g') to dL_dmeans3D, dL_dcov3D, dL_dscales,
//       dL_drotations, dL_dscale_factors with backward_preprocess.hip's chain from (dL/da, dL/db, dL/dc) on (T, J, the clamped
//       t.x, t.y held constant). It recomputes the covariance; nothing but the opacity gradient comes from the forward.
// rho is finite for every row: a row preprocess.hip's near-plane test culls, one with D1 == 0 and one with a non-finite D0, D1
// or r get rho = 1 and no gradient through rho; r <= 0.000025 gets the floor and no gradient through rho either.
// rho itself and every decision are fp32, the forward's own operations in the forward's order (this file is compiled with
// preprocess.hip's flags). The CHAIN through rho is evaluated in double from the same fp32 inputs: D0 = a0 c0 - b b cancels on
// a needle (b b within a part in 10^4 of a0 c0), and the derivative of r amplifies the rounding of a0, b, c0 by that factor -- in
// fp32 the scale gradient of a needle scene came out 3e-3 from the float64 derivative, in double at fp32 rounding of the sum.
// The kernel stays bound by its scattered rows: ~300 double operations per visible Gaussian.
// Everything P-sized is a plain read-modify-write (one lane owns one row). The codebook-sized outputs of the indexed form are
// scatter-ADDED the way backward_preprocess.hip does it: factors parked in LDS, then the wave walks its 64 Gaussians so that
// adjacent lanes of one atomic instruction cover whole codebook rows (MI355X_MICROARCH.md, Global float atomics).
#include "common.hpp"
#include "gsmath.hpp"

namespace c3dgs {

namespace {

constexpr float AA_H = 0.3f;              // the low-pass of cov2d()
constexpr float AA_FLOOR = 0.000025f;     // of r: rho >= 0.005

struct AaArgs {
    int P, W, H;
    const float* means3D; const float* opacities; const float* scales; const float* scale_factors; const float* rotations;
    const float* cov3D_precomp; const int64_t* g_indices;
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    int prefiltered;
};

struct AaRow {
    float rho;                 // 1 where the row does not depend on the projection (see `live`)
    bool live;                 // rho = sqrt(r) with r above the floor: the only rows with a gradient through rho
    bool clamp_x, clamp_y;     // t.x / t.y was clamped at 1.3 tan_fov: no gradient through that coordinate
    f3 m;
    float sc[3]; float4 rot; float sf; size_t gi;      // scale / rotation form: the row, its codebook index, its scale factor (or 1)
    float cov3D[6];
};

// rho of Gaussian i, and the inputs the backward chains through
__device__ __forceinline__ void aa_row(const AaArgs& a, const int i, const float* __restrict__ view, AaRow& w)
{
    const size_t si = (size_t)i;
    w.rho = 1.f; w.live = false; w.clamp_x = w.clamp_y = false;
    w.m = { a.means3D[3 * si], a.means3D[3 * si + 1], a.means3D[3 * si + 2] };
    w.gi = si; w.sf = 1.f;
    w.sc[0] = w.sc[1] = w.sc[2] = 0.f; w.rot = make_float4(1, 0, 0, 0);
    if (a.cov3D_precomp) {
#pragma unroll
        for (int q = 0; q < 6; q++) w.cov3D[q] = a.cov3D_precomp[6 * si + q];
    } else {
        float mod = a.scale_modifier;
        if (a.g_indices) { w.gi = (size_t)a.g_indices[i]; w.sf = a.scale_factors[i]; mod = w.sf * a.scale_modifier; }
        w.sc[0] = a.scales[3 * w.gi]; w.sc[1] = a.scales[3 * w.gi + 1]; w.sc[2] = a.scales[3 * w.gi + 2];
        w.rot = *reinterpret_cast<const float4*>(a.rotations + 4 * w.gi);
        cov3d_from_scale_rot(w.sc[0], w.sc[1], w.sc[2], mod, w.rot, w.cov3D);
    }
    const f3 p_view = xform4x3(w.m, view);
    if (!a.prefiltered && p_view.z <= 0.01f) return;               // preprocess.hip's near-plane test
    const Cov2D cv = cov2d_raw(w.m, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, w.cov3D, view);
    const float limx = 1.3f * a.tan_fovx, limy = 1.3f * a.tan_fovy;
    w.clamp_x = cv.txtz < -limx || cv.txtz > limx;
    w.clamp_y = cv.tytz < -limy || cv.tytz > limy;
    const float D0 = cv.a * cv.c - cv.b * cv.b;
    const float D1 = (cv.a + AA_H) * (cv.c + AA_H) - cv.b * cv.b;
    if (!isfinite(D0) || !isfinite(D1) || D1 == 0.0f) return;
    const float r = D0 / D1;
    if (!isfinite(r)) return;
    w.rho = sqrtf(fmaxf(AA_FLOOR, r));
    w.live = r > AA_FLOOR;
}

__global__ void __launch_bounds__(256) aa_opacity_kernel(const AaArgs a, const float* __restrict__ view,
                                                         float* __restrict__ opacity_out, float* __restrict__ rho_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    AaRow w;
    aa_row(a, i, view, w);
    opacity_out[i] = a.opacities[i] * w.rho;
    if (rho_out) rho_out[i] = w.rho;
}

// What the chain through rho adds for one live row, in double from the row's fp32 inputs; `dL_drho` = o g'.
// false: the double evaluation finds no r > 0 to differentiate (a row within rounding of D0 = 0): nothing is added.
struct AaChain { double dcov[6], dmean[3], d_s[3], dq[4]; };

__device__ __forceinline__ bool aa_chain(const AaArgs& a, const AaRow& w, const float* __restrict__ view, const double dL_drho,
                                         const bool scale_rot, AaChain& c)
{
    const double h = (double)AA_H;
    double v[12];                                                  // view[4 k + j], k = 0..2: rotation rows of world -> camera
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) v[3 * k + j] = (double)view[4 * k + j];
    const double mx = w.m.x, my = w.m.y, mz = w.m.z;
    const double t0 = v[0] * mx + v[3] * my + v[6] * mz + (double)view[12];
    const double t1 = v[1] * mx + v[4] * my + v[7] * mz + (double)view[13];
    const double tz = v[2] * mx + v[5] * my + v[8] * mz + (double)view[14];
    const double fx = (double)a.W / (2.0 * (double)a.tan_fovx), fy = (double)a.H / (2.0 * (double)a.tan_fovy);
    const double limx = (double)1.3f * (double)a.tan_fovx, limy = (double)1.3f * (double)a.tan_fovy;
    const double tx = w.clamp_x ? (t0 < 0 ? -limx : limx) * tz : t0;
    const double ty = w.clamp_y ? (t1 < 0 ? -limy : limy) * tz : t1;
    const double iz = 1.0 / tz, iz2 = iz * iz, iz3 = iz2 * iz;
    const double J[2][3] = { { fx * iz, 0.0, -fx * tx * iz2 }, { 0.0, fy * iz, -fy * ty * iz2 } };
    double A[2][3];                                                // upper 2x3 of J * R_w2c
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int k = 0; k < 3; k++) A[q][k] = J[q][0] * v[3 * k] + J[q][1] * v[3 * k + 1] + J[q][2] * v[3 * k + 2];

    // Sigma, and for the scale / rotation form L = Rm diag(s) with Sigma = L L^T
    double Sg[3][3], Rm[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } }, s[3] = { 0, 0, 0 };
    const double qr = w.rot.x, qx = w.rot.y, qy = w.rot.z, qz = w.rot.w;
    if (scale_rot) {
        const double mod = (double)w.sf * (double)a.scale_modifier;
        s[0] = mod * w.sc[0]; s[1] = mod * w.sc[1]; s[2] = mod * w.sc[2];
        Rm[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz); Rm[0][1] = 2.0 * (qx * qy - qr * qz); Rm[0][2] = 2.0 * (qx * qz + qr * qy);
        Rm[1][0] = 2.0 * (qx * qy + qr * qz); Rm[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz); Rm[1][2] = 2.0 * (qy * qz - qr * qx);
        Rm[2][0] = 2.0 * (qx * qz - qr * qy); Rm[2][1] = 2.0 * (qy * qz + qr * qx); Rm[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
#pragma unroll
        for (int u = 0; u < 3; u++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 3; j++) acc += (Rm[u][j] * s[j]) * (Rm[k][j] * s[j]);
                Sg[u][k] = acc;
            }
    } else {
        Sg[0][0] = w.cov3D[0]; Sg[0][1] = Sg[1][0] = w.cov3D[1]; Sg[0][2] = Sg[2][0] = w.cov3D[2];
        Sg[1][1] = w.cov3D[3]; Sg[1][2] = Sg[2][1] = w.cov3D[4]; Sg[2][2] = w.cov3D[5];
    }
    double AS[2][3];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int k = 0; k < 3; k++) AS[q][k] = A[q][0] * Sg[0][k] + A[q][1] * Sg[1][k] + A[q][2] * Sg[2][k];
    const double a0 = AS[0][0] * A[0][0] + AS[0][1] * A[0][1] + AS[0][2] * A[0][2];
    const double b = AS[0][0] * A[1][0] + AS[0][1] * A[1][1] + AS[0][2] * A[1][2];
    const double c0 = AS[1][0] * A[1][0] + AS[1][1] * A[1][1] + AS[1][2] * A[1][2];
    const double D0 = a0 * c0 - b * b, D1 = (a0 + h) * (c0 + h) - b * b;
    const double r = D0 / D1;
    if (!(r > 0.0) || !isfinite(r)) return false;

    // dL/drho -> r -> (a0, b, c0)
    const double dL_dr = dL_drho * (0.5 / sqrt(r));
    const double iD1sq = 1.0 / (D1 * D1);
    const double dL_da = dL_dr * (c0 * D1 - D0 * (c0 + h)) * iD1sq;
    const double dL_dc = dL_dr * (a0 * D1 - D0 * (a0 + h)) * iD1sq;
    const double dL_db = dL_dr * (-2.0 * b * (D1 - D0)) * iD1sq;

    // (a0, b, c0) -> cov3D / mean: backward_preprocess.hip (b)
    const double Gm[2][2] = { { dL_da, 0.5 * dL_db }, { 0.5 * dL_db, dL_dc } };
    double S3[3][3];
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int k = u; k < 3; k++) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int p = 0; p < 2; p++) acc += A[q][u] * Gm[q][p] * A[p][k];
            S3[u][k] = acc;
        }
    c.dcov[0] = S3[0][0]; c.dcov[3] = S3[1][1]; c.dcov[5] = S3[2][2];
    c.dcov[1] = 2.0 * S3[0][1]; c.dcov[2] = 2.0 * S3[0][2]; c.dcov[4] = 2.0 * S3[1][2];

    double dA[2][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        dA[0][k] = 2.0 * AS[0][k] * dL_da + AS[1][k] * dL_db;
        dA[1][k] = 2.0 * AS[1][k] * dL_dc + AS[0][k] * dL_db;
    }
    const double dJ00 = v[0] * dA[0][0] + v[3] * dA[0][1] + v[6] * dA[0][2];
    const double dJ02 = v[2] * dA[0][0] + v[5] * dA[0][1] + v[8] * dA[0][2];
    const double dJ11 = v[1] * dA[1][0] + v[4] * dA[1][1] + v[7] * dA[1][2];
    const double dJ12 = v[2] * dA[1][0] + v[5] * dA[1][1] + v[8] * dA[1][2];
    const double dtx = w.clamp_x ? 0.0 : -fx * iz2 * dJ02;
    const double dty = w.clamp_y ? 0.0 : -fy * iz2 * dJ12;
    const double dtz = -fx * iz2 * dJ00 - fy * iz2 * dJ11 + 2.0 * fx * tx * iz3 * dJ02 + 2.0 * fy * ty * iz3 * dJ12;
    c.dmean[0] = v[0] * dtx + v[1] * dty + v[2] * dtz;
    c.dmean[1] = v[3] * dtx + v[4] * dty + v[5] * dtz;
    c.dmean[2] = v[6] * dtx + v[7] * dty + v[8] * dtz;

    // cov3D -> scale / rotation: backward_preprocess.hip, dL/dL = 2 G L; d_s is with respect to the SCALED scale s
    if (scale_rot) {
        const double G3[3][3] = { { c.dcov[0], 0.5 * c.dcov[1], 0.5 * c.dcov[2] },
                                  { 0.5 * c.dcov[1], c.dcov[3], 0.5 * c.dcov[4] },
                                  { 0.5 * c.dcov[2], 0.5 * c.dcov[4], c.dcov[5] } };
        double Q[3][3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double col[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < 3; q++) acc += G3[k][q] * (Rm[q][j] * s[j]);
                col[k] = 2.0 * acc;
            }
            c.d_s[j] = Rm[0][j] * col[0] + Rm[1][j] * col[1] + Rm[2][j] * col[2];
#pragma unroll
            for (int k = 0; k < 3; k++) Q[k][j] = col[k] * s[j];
        }
        c.dq[0] = 2 * qz * (Q[1][0] - Q[0][1]) + 2 * qy * (Q[0][2] - Q[2][0]) + 2 * qx * (Q[2][1] - Q[1][2]);
        c.dq[1] = 2 * qy * (Q[0][1] + Q[1][0]) + 2 * qz * (Q[0][2] + Q[2][0]) + 2 * qr * (Q[2][1] - Q[1][2]) - 4 * qx * (Q[2][2] + Q[1][1]);
        c.dq[2] = 2 * qx * (Q[0][1] + Q[1][0]) + 2 * qr * (Q[0][2] - Q[2][0]) + 2 * qz * (Q[2][1] + Q[1][2]) - 4 * qy * (Q[2][2] + Q[0][0]);
        c.dq[3] = 2 * qr * (Q[1][0] - Q[0][1]) + 2 * qx * (Q[0][2] + Q[2][0]) + 2 * qy * (Q[2][1] + Q[1][2]) - 4 * qz * (Q[1][1] + Q[0][0]);
    }
    return true;
}

template <bool INDEXED>
__global__ void __launch_bounds__(256) aa_opacity_backward_kernel(const AaArgs a, const int32_t* __restrict__ radii,
                                                                  const c3dgs_raster_grads o, const float* __restrict__ view)
{
    // the indexed form parks what goes to the codebook rows here; -1: this lane adds nothing
    __shared__ float s_ds[INDEXED ? 256 : 1][3];
    __shared__ float s_dq[INDEXED ? 256 : 1][4];
    __shared__ int32_t s_gi[INDEXED ? 256 : 1];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t si = (size_t)i;
    if (INDEXED) s_gi[threadIdx.x] = -1;

    // A culled Gaussian's gradients are zero already. So are those of a visible one no pixel blended (about two thirds of the
    // visible ones on a dense view: sum_partials_kernel wrote them exact zeros): rho x 0 and the terms through rho, all factors of
    // g' = 0, change no bit, so such a row costs its two 4-byte reads and nothing else.
    const float gp = (i < a.P && radii[i] > 0) ? o.dL_dopacity[si] : 0.f;      // the rasterizer's dL/do'
    if (gp != 0.f) {
        AaRow w;
        aa_row(a, i, view, w);
        o.dL_dopacity[si] = w.rho * gp;
        const bool scale_rot = a.scales != nullptr;
        AaChain c;
        if (w.live && aa_chain(a, w, view, (double)a.opacities[si] * (double)gp, scale_rot, c)) {
            if (o.dL_dcov3D)
#pragma unroll
                for (int q = 0; q < 6; q++) o.dL_dcov3D[6 * si + q] += (float)c.dcov[q];
            if (o.dL_dmeans3D)
#pragma unroll
                for (int q = 0; q < 3; q++) o.dL_dmeans3D[3 * si + q] += (float)c.dmean[q];
            if (scale_rot) {
                // exact derivatives: scale = sf x scale_modifier x the row (sf = 1 without g_indices)
                const double mod = (double)w.sf * (double)a.scale_modifier;
                if (INDEXED) {
#pragma unroll
                    for (int q = 0; q < 3; q++) s_ds[threadIdx.x][q] = (float)(c.d_s[q] * mod);
#pragma unroll
                    for (int q = 0; q < 4; q++) s_dq[threadIdx.x][q] = (float)c.dq[q];
                    s_gi[threadIdx.x] = (int32_t)w.gi;
                    if (o.dL_dscale_factors)
                        o.dL_dscale_factors[si] += (float)((double)a.scale_modifier * (c.d_s[0] * w.sc[0] + c.d_s[1] * w.sc[1] + c.d_s[2] * w.sc[2]));
                } else {
                    if (o.dL_dscales)
#pragma unroll
                        for (int q = 0; q < 3; q++) o.dL_dscales[3 * si + q] += (float)(c.d_s[q] * mod);
                    if (o.dL_drotations) {
                        float4* dst = reinterpret_cast<float4*>(o.dL_drotations + 4 * si);
                        const float4 t = *dst;
                        *dst = make_float4(t.x + (float)c.dq[0], t.y + (float)c.dq[1], t.z + (float)c.dq[2], t.w + (float)c.dq[3]);
                    }
                }
            }
        }
    }

    if (INDEXED) {
        // each wave scatter-adds what its own 64 lanes parked: wave-level ordering of the LDS traffic is all that is needed
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
        if (o.dL_dscales)
#pragma unroll
            for (int it = 0; it < 3; it++) {
                const int q = it * 64 + lane, j = q / 3, c = q - 3 * j;
                const int32_t gi = s_gi[wbase + j];
                if (gi >= 0) atomicAdd(o.dL_dscales + 3 * (size_t)gi + c, s_ds[wbase + j][c]);
            }
        if (o.dL_drotations)
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int q = it * 64 + lane, j = q >> 2, c = q & 3;
                const int32_t gi = s_gi[wbase + j];
                if (gi >= 0) atomicAdd(o.dL_drotations + 4 * (size_t)gi + c, s_dq[wbase + j][c]);
            }
    }
}

AaArgs aa_args(const c3dgs_raster_params& p)
{
    AaArgs a;
    a.P = p.P; a.W = p.W; a.H = p.H;
    a.means3D = p.means3D; a.opacities = p.opacities; a.scales = p.scales; a.rotations = p.rotations;
    a.cov3D_precomp = p.cov3D_precomp;
    a.g_indices = p.cov3D_precomp ? nullptr : p.g_indices;
    a.scale_factors = a.g_indices ? p.scale_factors : nullptr;
    a.tan_fovx = p.tan_fovx; a.tan_fovy = p.tan_fovy;
    a.focal_y = p.H / (2.0f * p.tan_fovy);
    a.focal_x = p.W / (2.0f * p.tan_fovx);
    a.scale_modifier = p.scale_modifier;
    a.prefiltered = p.prefiltered;
    return a;
}

} // namespace

void launch_aa_opacity(const c3dgs_raster_params& p, float* opacity_out, float* rho, hipStream_t s)
{
    if (p.P <= 0) return;
    aa_opacity_kernel<<<(p.P + 255) / 256, 256, 0, s>>>(aa_args(p), p.viewmatrix, opacity_out, rho);
}

void launch_aa_opacity_backward(const c3dgs_raster_params& p, const int32_t* radii, const c3dgs_raster_grads& gr, hipStream_t s)
{
    if (p.P <= 0) return;
    const AaArgs a = aa_args(p);
    const int grid = (p.P + 255) / 256;
    if (a.g_indices) aa_opacity_backward_kernel<true><<<grid, 256, 0, s>>>(a, radii, gr, p.viewmatrix);
    else aa_opacity_backward_kernel<false><<<grid, 256, 0, s>>>(a, radii, gr, p.viewmatrix);
}

} // namespace c3dgs
