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
//       dL_drotations, dL_dscale_factors with gsgrad.hpp's chain from (dL/da, dL/db, dL/dc): conic_grad_to_cov3d,
//       conic_grad_to_mean, cov3d_grad_to_scale_rot, in double (backward_preprocess.hip restates the three in fp32).
//       It recomputes the covariance; nothing but the opacity gradient comes from the forward.
// rho is finite for every row: a row preprocess.hip's near-plane test culls, one with D1 == 0 and one with a non-finite D0, D1
// or r get rho = 1 and no gradient through rho; r <= 0.000025 gets the floor and no gradient through rho either.
// rho itself and every decision are fp32, the forward's own operations in the forward's order (this file is compiled with
// preprocess.hip's flags). The CHAIN through rho is evaluated in double from the same fp32 inputs: D0 = a0 c0 - b b cancels on
// a needle (b b within a part in 10^4 of a0 c0), and the derivative of r amplifies the rounding of a0, b, c0 by that factor -- in
// fp32 the scale gradient of a needle scene came out 3e-3 from the float64 derivative, in double at fp32 rounding of the sum.
// The kernel stays bound by its scattered rows: ~300 double operations per visible Gaussian.
// Everything P-sized is a plain read-modify-write (one lane owns one row). The codebook-sized outputs of the indexed form are
// scatter-ADDED by gsgrad.hpp's scatter_add_scale_rot(), as backward_preprocess.hip's are.
#include "common.hpp"
#include "gsgrad.hpp"

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
    ScaleRotRow g;             // scales, rotation, codebook row, scale factor (or their neutral values) and Sigma
};

// rho of Gaussian i, and the inputs the backward chains through
__device__ __forceinline__ void aa_row(const AaArgs& a, const int i, const float* __restrict__ view, AaRow& w)
{
    const size_t si = (size_t)i;
    w.rho = 1.f; w.live = false; w.clamp_x = w.clamp_y = false;
    w.m = { a.means3D[3 * si], a.means3D[3 * si + 1], a.means3D[3 * si + 2] };
    load_scale_rot_row(a.cov3D_precomp, a.scales, a.rotations, a.scale_factors, a.g_indices, si, a.scale_modifier, w.g);
    const f3 p_view = xform4x3(w.m, view);
    if (!a.prefiltered && p_view.z <= 0.01f) return;               // preprocess.hip's near-plane test
    const Cov2D cv = cov2d_raw(w.m, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, w.g.cov3D, view);
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
    double v[3][3];                                                // view[4 k + j]: the rotation of world -> camera, column major
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) v[k][j] = (double)view[4 * k + j];
    const double mx = w.m.x, my = w.m.y, mz = w.m.z;
    const double t0 = v[0][0] * mx + v[1][0] * my + v[2][0] * mz + (double)view[12];
    const double t1 = v[0][1] * mx + v[1][1] * my + v[2][1] * mz + (double)view[13];
    const double tz = v[0][2] * mx + v[1][2] * my + v[2][2] * mz + (double)view[14];
    const double fx = (double)a.W / (2.0 * (double)a.tan_fovx), fy = (double)a.H / (2.0 * (double)a.tan_fovy);
    const double limx = (double)1.3f * (double)a.tan_fovx, limy = (double)1.3f * (double)a.tan_fovy;
    const double tx = w.clamp_x ? (t0 < 0 ? -limx : limx) * tz : t0;
    const double ty = w.clamp_y ? (t1 < 0 ? -limy : limy) * tz : t1;
    const double iz = 1.0 / tz, iz2 = iz * iz;
    const double J[2][3] = { { fx * iz, 0.0, -fx * tx * iz2 }, { 0.0, fy * iz, -fy * ty * iz2 } };
    double A[2][3];                                                // upper 2x3 of J * R_w2c
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int k = 0; k < 3; k++) A[q][k] = J[q][0] * v[k][0] + J[q][1] * v[k][1] + J[q][2] * v[k][2];

    // Sigma, and for the scale / rotation form L = Rm diag(s) with Sigma = L L^T
    double Sg[3][3], s[3] = { 0, 0, 0 };
    const double qr = w.g.rot.x, qx = w.g.rot.y, qy = w.g.rot.z, qz = w.g.rot.w;
    if (scale_rot) {
        const double mod = (double)w.g.sf * (double)a.scale_modifier;
        s[0] = mod * w.g.sc[0]; s[1] = mod * w.g.sc[1]; s[2] = mod * w.g.sc[2];
        double Rm[3][3];
        quat_to_rot(qr, qx, qy, qz, Rm);
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
        Sg[0][0] = w.g.cov3D[0]; Sg[0][1] = Sg[1][0] = w.g.cov3D[1]; Sg[0][2] = Sg[2][0] = w.g.cov3D[2];
        Sg[1][1] = w.g.cov3D[3]; Sg[1][2] = Sg[2][1] = w.g.cov3D[4]; Sg[2][2] = w.g.cov3D[5];
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

    // (a0, b, c0) -> cov3D / mean -> scale / rotation: gsgrad.hpp; d_s is with respect to the SCALED scale s
    conic_grad_to_cov3d(A, dL_da, dL_db, dL_dc, c.dcov);
    conic_grad_to_mean(A, Sg, v, fx, fy, tx, ty, tz, w.clamp_x, w.clamp_y, dL_da, dL_db, dL_dc, c.dmean);
    if (scale_rot) cov3d_grad_to_scale_rot(c.dcov, s, qr, qx, qy, qz, c.d_s, c.dq);
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
                const double mod = (double)w.g.sf * (double)a.scale_modifier;
                if (INDEXED) {
#pragma unroll
                    for (int q = 0; q < 3; q++) s_ds[threadIdx.x][q] = (float)(c.d_s[q] * mod);
#pragma unroll
                    for (int q = 0; q < 4; q++) s_dq[threadIdx.x][q] = (float)c.dq[q];
                    s_gi[threadIdx.x] = (int32_t)w.g.gi;
                    if (o.dL_dscale_factors)
                        o.dL_dscale_factors[si] += (float)((double)a.scale_modifier * (c.d_s[0] * w.g.sc[0] + c.d_s[1] * w.g.sc[1] + c.d_s[2] * w.g.sc[2]));
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
        wave_lds_fence();
        scatter_add_scale_rot(s_gi, s_ds, s_dq, o.dL_dscales, o.dL_drotations);
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
