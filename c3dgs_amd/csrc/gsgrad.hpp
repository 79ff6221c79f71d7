// gsgrad.hpp -- the per-Gaussian gradient chains and row loads that more than one kernel needs, for gfx950: one definition
// each, inlined where it is called.
//
// Same contract as gsmath.hpp: translation units that include this file are compiled with -ffp-contract=off, so an fp32
// instantiation is the same sequence of single IEEE operations wherever it is inlined and two kernels that call one function
// on the same inputs produce the same bits. The chains are templates over the scalar type: fp32 for filter3d.hip, double for the
// chain through rho of aa_opacity.hip. backward_preprocess_kernel calls sh_view_dir_grad(), wave_lds_fence() and
// scatter_add_scale_rot() and RESTATES the conic and covariance chains and the SH row load in place, each with a pointer to
// its function here: called, they cost the hot kernel time or scratch (profiles/gsgrad/README.md). An edit to a chain here is
// owed to that kernel too; tests/test_gsgrad_gpu.py fails when the covariance chains part.
// Nothing here touches global gradient memory except scatter_add_scale_rot().
#pragma once
#include "gsmath.hpp"

namespace c3dgs {

// ---- loads

// A Gaussian's first NC SH coefficients from its row of M * 3 floats: 16-byte loads where every row is 16-byte aligned and NC
// is whole float4s (M = 4, 16), scalar loads otherwise. For preprocess_kernel; backward_preprocess_kernel restates it, and
// pose_sums_kernel keeps plain scalar loads (both for their registers: profiles/gsgrad/README.md).
template <int NC>
__device__ __forceinline__ void load_sh_row(const float* shp, const int M, float c[NC])
{
    if ((M * 3) % 4 == 0 && NC % 4 == 0) {
#pragma unroll
        for (int q = 0; q < NC / 4; q++) {
            const float4 v = reinterpret_cast<const float4*>(shp)[q];
            c[4 * q] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < NC; q++) c[q] = shp[q];
    }
}

// Row i in whichever form the caller's model has: a covariance of its own (cov3D_precomp), or scales and rotations, which are
// the row's own or, with g_indices, codebook row gi under the per-Gaussian scale factor sf. Sigma is built as preprocess_kernel
// builds it. What a form does not have keeps its neutral value (sc = 0, rot = identity, sf = 1, gi = i). Every pointer that is
// not null is read: scales next to a covariance serve filter3d.hip's opacity factor. aa_opacity.hip and pose_grad.hip, which
// read no scales for a caller's covariance, rely on the C ABI for that: it accepts exactly one of cov3D_precomp and the scale /
// rotation pair there, and aa_args() drops g_indices with a covariance.
struct ScaleRotRow {
    size_t gi; float sf;
    float sc[3]; float4 rot;
    float cov3D[6];
};
__device__ __forceinline__ void load_scale_rot_row(const float* cov3D_precomp, const float* scales, const float* rotations,
                                                   const float* scale_factors, const int64_t* g_indices, const size_t i,
                                                   const float scale_modifier, ScaleRotRow& w)
{
    w.gi = i; w.sf = 1.f;
    w.sc[0] = w.sc[1] = w.sc[2] = 0.f; w.rot = make_float4(1, 0, 0, 0);
    if (g_indices) { w.gi = (size_t)g_indices[i]; w.sf = scale_factors[i]; }
    if (scales) { w.sc[0] = scales[3 * w.gi]; w.sc[1] = scales[3 * w.gi + 1]; w.sc[2] = scales[3 * w.gi + 2]; }
    if (cov3D_precomp) {
#pragma unroll
        for (int q = 0; q < 6; q++) w.cov3D[q] = cov3D_precomp[6 * i + q];
    } else {
        w.rot = *reinterpret_cast<const float4*>(rotations + 4 * w.gi);
        cov3d_from_scale_rot(w.sc[0], w.sc[1], w.sc[2], w.sf * scale_modifier, w.rot, w.cov3D);
    }
}

// ---- SH colour -> view direction (reference backward.cu:20-139 without the coefficient gradients, and dnormvdv,
// auxiliary.h:107-117). c = the Gaussian's coefficients, d0 = mean - campos (not normalised), g = dL/dcolour with the clamped
// channels zeroed; out = that share of dL/dmean. DEG 0 has no direction term: out is a sum of zero products.
template <int DEG>
__device__ __forceinline__ void sh_view_dir_grad(const float* c, const f3 d0, const float g[3], float out[3])
{
    const float len = sqrtf(d0.x * d0.x + d0.y * d0.y + d0.z * d0.z);
    const float x = d0.x / len, y = d0.y / len, z = d0.z / len;
    float dx[3] = { 0, 0, 0 }, dy[3] = { 0, 0, 0 }, dz[3] = { 0, 0, 0 };
    if (DEG > 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            dx[ch] = -SH_C1 * c[3 * 3 + ch];
            dy[ch] = -SH_C1 * c[1 * 3 + ch];
            dz[ch] = SH_C1 * c[2 * 3 + ch];
        }
    }
    if (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float s4 = c[4 * 3 + ch], s5 = c[5 * 3 + ch], s6 = c[6 * 3 + ch], s7 = c[7 * 3 + ch], s8 = c[8 * 3 + ch];
            dx[ch] += SH_C2_0 * y * s4 + SH_C2_2 * 2.f * -x * s6 + SH_C2_3 * z * s7 + SH_C2_4 * 2.f * x * s8;
            dy[ch] += SH_C2_0 * x * s4 + SH_C2_1 * z * s5 + SH_C2_2 * 2.f * -y * s6 + SH_C2_4 * 2.f * -y * s8;
            dz[ch] += SH_C2_1 * y * s5 + SH_C2_2 * 2.f * 2.f * z * s6 + SH_C2_3 * x * s7;
        }
        if (DEG > 2) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float s9 = c[9 * 3 + ch], s10 = c[10 * 3 + ch], s11 = c[11 * 3 + ch], s12 = c[12 * 3 + ch],
                            s13 = c[13 * 3 + ch], s14 = c[14 * 3 + ch], s15 = c[15 * 3 + ch];
                dx[ch] += SH_C3_0 * s9 * 3.f * 2.f * xy + SH_C3_1 * s10 * yz + SH_C3_2 * s11 * -2.f * xy +
                          SH_C3_3 * s12 * -3.f * 2.f * xz + SH_C3_4 * s13 * (-3.f * xx + 4.f * zz - yy) +
                          SH_C3_5 * s14 * 2.f * xz + SH_C3_6 * s15 * 3.f * (xx - yy);
                dy[ch] += SH_C3_0 * s9 * 3.f * (xx - yy) + SH_C3_1 * s10 * xz + SH_C3_2 * s11 * (-3.f * yy + 4.f * zz - xx) +
                          SH_C3_3 * s12 * -3.f * 2.f * yz + SH_C3_4 * s13 * -2.f * xy + SH_C3_5 * s14 * -2.f * yz +
                          SH_C3_6 * s15 * -3.f * 2.f * xy;
                dz[ch] += SH_C3_1 * s10 * xy + SH_C3_2 * s11 * 4.f * 2.f * yz + SH_C3_3 * s12 * 3.f * (2.f * zz - xx - yy) +
                          SH_C3_4 * s13 * 4.f * 2.f * xz + SH_C3_5 * s14 * (xx - yy);
            }
        }
    }
    const float ddx = dx[0] * g[0] + dx[1] * g[1] + dx[2] * g[2];
    const float ddy = dy[0] * g[0] + dy[1] * g[1] + dy[2] * g[2];
    const float ddz = dz[0] * g[0] + dz[1] * g[1] + dz[2] * g[2];
    const float sum2 = d0.x * d0.x + d0.y * d0.y + d0.z * d0.z;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    out[0] = ((+sum2 - d0.x * d0.x) * ddx - d0.y * d0.x * ddy - d0.z * d0.x * ddz) * invsum32;
    out[1] = (-d0.x * d0.y * ddx + (sum2 - d0.y * d0.y) * ddy - d0.z * d0.y * ddz) * invsum32;
    out[2] = (-d0.x * d0.z * ddx - d0.y * d0.z * ddy + (sum2 - d0.z * d0.z) * ddz) * invsum32;
}

// ---- conic -> Sigma / mean (reference backward.cu:144-274 in matrix form). cov2D = A Sigma A^T (+ the low-pass) with A the
// upper 2x3 of J R_w2c (reference T[i][j] == A[i][j]); (dL_da, dL_db, dL_dc) are the gradients of its entries (0,0), (0,1), (1,1).
// Two functions, because backward_preprocess_kernel stores dL/dSigma, and skips it where its conic has no inverse, between them.

// dL/dSigma as the six-vector: A^T G A, an off-diagonal element counting both of its positions
template <class T>
__device__ __forceinline__ void conic_grad_to_cov3d(const T A[2][3], const T dL_da, const T dL_db, const T dL_dc, T dcov[6])
{
    const T Gm[2][2] = { { dL_da, T(0.5) * dL_db }, { T(0.5) * dL_db, dL_dc } };
    T S3[3][3];
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = u; v < 3; v++) {
            T s = 0;
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int w = 0; w < 2; w++) s += A[q][u] * Gm[q][w] * A[w][v];
            S3[u][v] = s;
        }
    dcov[0] = S3[0][0]; dcov[3] = S3[1][1]; dcov[5] = S3[2][2];
    dcov[1] = T(2) * S3[0][1]; dcov[2] = T(2) * S3[0][2]; dcov[4] = T(2) * S3[1][2];
}

// dL/dmean through A = J(t) R_w2c. Sg = Sigma as a full matrix, Rv[k][j] = view[4 k + j] (the rotation of the column-major
// world -> camera matrix), t = the view-space mean with x and y clamped as cov2d() clamps them; a clamped coordinate passes no
// gradient (the reference's x_grad_mul / y_grad_mul).
template <class T>
__device__ __forceinline__ void conic_grad_to_mean(const T A[2][3], const T Sg[3][3], const T Rv[3][3], const T fx, const T fy,
                                                   const T tx, const T ty, const T t_z, const bool clamp_x, const bool clamp_y,
                                                   const T dL_da, const T dL_db, const T dL_dc, T dmean[3])
{
    T AS[2][3], dA[2][3];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int v = 0; v < 3; v++) AS[q][v] = A[q][0] * Sg[0][v] + A[q][1] * Sg[1][v] + A[q][2] * Sg[2][v];
#pragma unroll
    for (int v = 0; v < 3; v++) {
        dA[0][v] = 2 * AS[0][v] * dL_da + AS[1][v] * dL_db;
        dA[1][v] = 2 * AS[1][v] * dL_dc + AS[0][v] * dL_db;
    }
    const T dJ00 = Rv[0][0] * dA[0][0] + Rv[1][0] * dA[0][1] + Rv[2][0] * dA[0][2];
    const T dJ02 = Rv[0][2] * dA[0][0] + Rv[1][2] * dA[0][1] + Rv[2][2] * dA[0][2];
    const T dJ11 = Rv[0][1] * dA[1][0] + Rv[1][1] * dA[1][1] + Rv[2][1] * dA[1][2];
    const T dJ12 = Rv[0][2] * dA[1][0] + Rv[1][2] * dA[1][1] + Rv[2][2] * dA[1][2];
    const T x_grad_mul = clamp_x ? T(0) : T(1), y_grad_mul = clamp_y ? T(0) : T(1);
    const T tz = T(1) / t_z, tz2 = tz * tz, tz3 = tz2 * tz;
    const T dtx = x_grad_mul * -fx * tz2 * dJ02;
    const T dty = y_grad_mul * -fy * tz2 * dJ12;
    const T dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2 * fx * tx) * tz3 * dJ02 + (2 * fy * ty) * tz3 * dJ12;
    dmean[0] = Rv[0][0] * dtx + Rv[0][1] * dty + Rv[0][2] * dtz;
    dmean[1] = Rv[1][0] * dtx + Rv[1][1] * dty + Rv[1][2] * dtz;
    dmean[2] = Rv[2][0] * dtx + Rv[2][1] * dty + Rv[2][2] * dtz;
}

// ---- Sigma -> scale / rotation (reference backward.cu:278-341 / backward_indexed.cu:206-282)

// the standard rotation matrix of the quaternion (r, x, y, z), not normalised: cov3d_from_scale_rot()'s entries
template <class T>
__device__ __forceinline__ void quat_to_rot(const T r, const T x, const T y, const T z, T Rm[3][3])
{
    Rm[0][0] = T(1) - T(2) * (y * y + z * z); Rm[0][1] = T(2) * (x * y - r * z); Rm[0][2] = T(2) * (x * z + r * y);
    Rm[1][0] = T(2) * (x * y + r * z); Rm[1][1] = T(1) - T(2) * (x * x + z * z); Rm[1][2] = T(2) * (y * z - r * x);
    Rm[2][0] = T(2) * (x * z - r * y); Rm[2][1] = T(2) * (y * z + r * x); Rm[2][2] = T(1) - T(2) * (x * x + y * y);
}

// L = Rm diag(s), Sigma = L L^T, dL/dL = 2 G L with G = dcov as a full matrix (half of each off-diagonal element). s is the
// SCALED scale (modifier and scale factor included) and d_s the gradient with respect to it: each caller distributes d_s to its
// own inputs. dq is the gradient of the quaternion as stored.
template <class T>
__device__ __forceinline__ void cov3d_grad_to_scale_rot(const T dcov[6], const T s[3], const T r, const T x, const T y, const T z,
                                                        T d_s[3], T dq[4])
{
    T Rm[3][3];
    quat_to_rot(r, x, y, z, Rm);
    const T G3[3][3] = { { dcov[0], T(0.5) * dcov[1], T(0.5) * dcov[2] },
                         { T(0.5) * dcov[1], dcov[3], T(0.5) * dcov[4] },
                         { T(0.5) * dcov[2], T(0.5) * dcov[4], dcov[5] } };
    T Q[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        T col[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            T accv = 0;
#pragma unroll
            for (int q = 0; q < 3; q++) accv += G3[k][q] * (Rm[q][j] * s[j]);
            col[k] = T(2) * accv;
        }
        d_s[j] = Rm[0][j] * col[0] + Rm[1][j] * col[1] + Rm[2][j] * col[2];
#pragma unroll
        for (int k = 0; k < 3; k++) Q[k][j] = col[k] * s[j];
    }
    dq[0] = 2 * z * (Q[1][0] - Q[0][1]) + 2 * y * (Q[0][2] - Q[2][0]) + 2 * x * (Q[2][1] - Q[1][2]);
    dq[1] = 2 * y * (Q[0][1] + Q[1][0]) + 2 * z * (Q[0][2] + Q[2][0]) + 2 * r * (Q[2][1] - Q[1][2]) - 4 * x * (Q[2][2] + Q[1][1]);
    dq[2] = 2 * x * (Q[0][1] + Q[1][0]) + 2 * r * (Q[0][2] - Q[2][0]) + 2 * z * (Q[2][1] + Q[1][2]) - 4 * y * (Q[2][2] + Q[0][0]);
    dq[3] = 2 * r * (Q[1][0] - Q[0][1]) + 2 * x * (Q[0][2] + Q[2][0]) + 2 * y * (Q[2][1] + Q[1][2]) - 4 * z * (Q[1][1] + Q[0][0]);
}

// ---- the per-Gaussian normal (normals.hip): the shortest axis of the Gaussian, in view space, facing the camera.
// m = the index of the smallest entry of the RAW scale row (no modifier, no scale factor: multiplying first can round two scales
// into a tie and pick another axis than an exact comparison does), the lowest index on a tie; c = column m of quat_to_rot(q),
// q as stored; v = R_view c / |c| (the zero vector where |c| == 0), R_view[i][k] = view[4 k + i]; n = sigma v with sigma = -1 where
// v . p > 0 for the view-space mean p, else +1. m and sigma are piecewise constant: the only gradient is the one to q.
__device__ __forceinline__ int smallest_axis(const float s0, const float s1, const float s2)
{
    int m = 0;
    float v = s0;
    if (s1 < v) { m = 1; v = s1; }
    if (s2 < v) m = 2;
    return m;
}

// column m of quat_to_rot(q) and its length
template <class T>
__device__ __forceinline__ T rot_column(const T r, const T x, const T y, const T z, const int m, T c[3])
{
    T Rm[3][3];
    quat_to_rot(r, x, y, z, Rm);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = m == 0 ? Rm[k][0] : (m == 1 ? Rm[k][1] : Rm[k][2]);
    return sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
}

// v = R_view c / |c|: the normal up to its sign
template <class T>
__device__ __forceinline__ void normal_from_quat(const T r, const T x, const T y, const T z, const int m, const float* view, T v[3])
{
    T c[3];
    const T len = rot_column(r, x, y, z, m, c);
    const T inv = len > T(0) ? T(1) / len : T(0);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = c[k] * inv;
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = T(view[i]) * c[0] + T(view[4 + i]) * c[1] + T(view[8 + i]) * c[2];
}

// g = dL/dn -> dq = dL/dq as stored, through n = sigma R_view c / |c|, the 1 / |c| included; zero where |c| == 0
template <class T>
__device__ __forceinline__ void normal_grad_to_quat(const T r, const T x, const T y, const T z, const int m, const T sigma,
                                                    const float* view, const T g[3], T dq[4])
{
    T c[3], gh[3], gc[3];
    const T len = rot_column(r, x, y, z, m, c);
    const T inv = len > T(0) ? T(1) / len : T(0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c[k] = c[k] * inv;
        gh[k] = sigma * (T(view[4 * k]) * g[0] + T(view[4 * k + 1]) * g[1] + T(view[4 * k + 2]) * g[2]);
    }
    const T d = c[0] * gh[0] + c[1] * gh[1] + c[2] * gh[2];
#pragma unroll
    for (int k = 0; k < 3; k++) gc[k] = (gh[k] - c[k] * d) * inv;
    if (m == 0) {           // c = (1 - 2 (y y + z z), 2 (x y + r z), 2 (x z - r y))
        dq[0] = 2 * z * gc[1] - 2 * y * gc[2];
        dq[1] = 2 * y * gc[1] + 2 * z * gc[2];
        dq[2] = -4 * y * gc[0] + 2 * x * gc[1] - 2 * r * gc[2];
        dq[3] = -4 * z * gc[0] + 2 * r * gc[1] + 2 * x * gc[2];
    } else if (m == 1) {    // c = (2 (x y - r z), 1 - 2 (x x + z z), 2 (y z + r x))
        dq[0] = -2 * z * gc[0] + 2 * x * gc[2];
        dq[1] = 2 * y * gc[0] - 4 * x * gc[1] + 2 * r * gc[2];
        dq[2] = 2 * x * gc[0] + 2 * z * gc[2];
        dq[3] = -2 * r * gc[0] - 4 * z * gc[1] + 2 * y * gc[2];
    } else {                // c = (2 (x z + r y), 2 (y z - r x), 1 - 2 (x x + y y))
        dq[0] = 2 * y * gc[0] - 2 * x * gc[1];
        dq[1] = 2 * z * gc[0] - 2 * r * gc[1] - 4 * x * gc[2];
        dq[2] = 2 * r * gc[0] + 2 * z * gc[1] - 4 * y * gc[2];
        dq[3] = 2 * x * gc[0] + 2 * y * gc[1];
    }
}

// ---- codebook-sized gradients of the indexed model are scatter-ADDED. One lane per Gaussian would issue each atomic with 64
// lanes in 64 different rows, the slowest shape for the chip's memory-side float atomics (MI355X_MICROARCH.md, Global float
// atomics). So every lane parks its row (s_gi: codebook row, -1 = nothing to add), its three scale and four rotation terms in the
// workgroup's LDS arrays, the wave orders its LDS traffic with wave_lds_fence(), and then walks its own 64 entries here so that
// adjacent lanes of one atomic instruction cover whole rows.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void scatter_add_scale_rot(const int32_t* s_gi, const float (*s_ds)[3], const float (*s_dq)[4],
                                                      float* dL_dscales, float* dL_drotations)
{
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    if (dL_dscales)
#pragma unroll
        for (int it = 0; it < 3; it++) {
            const int q = it * 64 + lane, j = q / 3, c = q - 3 * j;
            const int32_t gi = s_gi[wbase + j];
            if (gi >= 0) atomicAdd(dL_dscales + 3 * (size_t)gi + c, s_ds[wbase + j][c]);
        }
    if (dL_drotations)
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int q = it * 64 + lane, j = q >> 2, c = q & 3;
            const int32_t gi = s_gi[wbase + j];
            if (gi >= 0) atomicAdd(dL_drotations + 4 * (size_t)gi + c, s_dq[wbase + j][c]);
        }
}

} // namespace c3dgs
