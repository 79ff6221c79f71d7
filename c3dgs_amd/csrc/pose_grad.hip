// pose_grad.hip -- the exact gradient of the render with respect to the camera's 7-element pose (qx, qy, qz, qw, tx, ty, tz),
// from what a finished backward already holds (gfx950). No reference counterpart: the reference's pose gradient chains only
// dL/dmeans2D through a projection formula (DGR-NC __init__.py:674-844; rasterizer.camera_pose_jacobian_sum restates it).
//
// The image depends on the pose only through p_i = R mu_i + t, the view-space covariance R Sigma_i R^T and the SH view
// direction mu_i - c with c = -R^-1 t (R, t: what camera_from_pose_kernel builds; R is NOT assumed orthonormal). With
//     g_i    = dL/dmu_i                        the backward's complete dL_dmeans3D (the t-clamp's semantics are inside it)
//     G_i    = dL/dSigma_i as a full matrix    dL_dcov3D: its off-diagonal entries already count both symmetric positions
//     gdir_i = the part of g_i that came through the SH view direction (what backward_preprocess adds last)
// the gradient is, exactly (DESIGN.md "Exact pose gradient"),
//     dL/dt = R^-T sum_i g_i
//     dL/dR = R^-T [ sum_i (g_i - gdir_i) mu_i^T + sum_i (G_i + G_i^T) Sigma_i + (sum_i gdir_i) c^T ]
// and dL/dpose follows through the entries of the unnormalised-quaternion matrix. Two kernels:
//   pose_sums_kernel (stage A, one lane per Gaussian): the 24 numbers S_g (3), S_d (3), M1 (9), M2 (9) of its Gaussian, reduced
//       over the wave by a fixed butterfly and over the workgroup's four waves through LDS; one 96-byte row per workgroup.
//   pose_fold_kernel (stage B, one workgroup): folds the rows in double in an order that depends on their number alone; one
//       lane then applies R^-T, the c^T term and the quaternion chain and stores seven floats.
// No atomics: the result is bitwise reproducible from run to run.
#include "common.hpp"
#include "gsgrad.hpp"    // sh_view_dir_grad, load_scale_rot_row; includes gsmath.hpp

namespace c3dgs {

constexpr int POSE_SUMS = 24;                          // S_g | S_d | M1 (row major) | M2 (row major)
constexpr int POSE_FOLD_ROWS = 1024 / POSE_SUMS;       // 42 rows of the workspace per sweep of stage B's 1024 threads
constexpr int POSE_FOLD_THREADS = POSE_FOLD_ROWS * POSE_SUMS;   // 1008 of them work

struct PoseArgs {
    int P, M;
    float scale_modifier;
    const float* means3D; const float* dL_dmeans3D; const float* dL_dcov3D; const float* dL_dcolors;
    const float* sh; const int64_t* sh_indices;
    const float* cov3D_precomp; const float* scales; const float* rotations; const float* scale_factors; const int64_t* g_indices;
    const uint8_t* clamped; const int32_t* radii;
    float* rows;                                       // [n_blocks][POSE_SUMS]
};

// World -> camera rotation, its inverse and the camera centre from the pose, as camera_from_pose_kernel (preprocess.hip) forms
// them: the matrix entries with that kernel's fp32 operations (this file is built with -ffp-contract=off), the inverse by
// adjugate in double, campos rounded to fp32 -- the very values the backward's SH direction was taken from.
struct PoseCamera { double R[3][3], inv[3][3]; float campos[3]; };
__device__ __forceinline__ PoseCamera pose_camera(const float* __restrict__ pose)
{
    const float x = pose[0], y = pose[1], z = pose[2], w = pose[3], tx = pose[4], ty = pose[5], tz = pose[6];
    const float d2 = y * y + z * z + x * x;
    PoseCamera o;
    o.R[0][0] = 1.0f + 2.0f * (x * x - d2); o.R[0][1] = 2.0f * (x * y - w * z);        o.R[0][2] = 2.0f * (x * z + w * y);
    o.R[1][0] = 2.0f * (x * y + w * z);        o.R[1][1] = 1.0f + 2.0f * (y * y - d2); o.R[1][2] = 2.0f * (y * z - w * x);
    o.R[2][0] = 2.0f * (x * z - w * y);        o.R[2][1] = 2.0f * (y * z + w * x);        o.R[2][2] = 1.0f + 2.0f * (z * z - d2);
    const double a = o.R[0][0], b = o.R[0][1], c = o.R[0][2], d = o.R[1][0], e = o.R[1][1], f = o.R[1][2], g = o.R[2][0],
                 h = o.R[2][1], k = o.R[2][2];
    const double A = e * k - f * h, B = -(d * k - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    o.inv[0][0] = A / det; o.inv[0][1] = -(b * k - c * h) / det; o.inv[0][2] = (b * f - c * e) / det;
    o.inv[1][0] = B / det; o.inv[1][1] = (a * k - c * g) / det;  o.inv[1][2] = -(a * f - c * d) / det;
    o.inv[2][0] = C / det; o.inv[2][1] = -(a * h - b * g) / det; o.inv[2][2] = (a * e - b * d) / det;
#pragma unroll
    for (int r = 0; r < 3; r++) o.campos[r] = (float)-(o.inv[r][0] * (double)tx + o.inv[r][1] * (double)ty + o.inv[r][2] * (double)tz);
    return o;
}

// ---- stage A. DEG = the active SH degree, 0 when the colours were precomputed or the degree is 0 (gdir is zero then and
// neither dL_dcolors, the clamped byte nor the SH row is read).
// Of a dense view's Gaussians about a tenth is ever blended; every other row of the three gradients is exact zeros. Such a
// lane stops at its 48 bytes of gradients (+ 4 of radii): no mean, no covariance gather, no SH row. A blended one reads its
// 192-byte SH row only if its colour gradient is not all zero. That keeps the pass near the cost of streaming the gradient rows.
template <int DEG>
__global__ void __launch_bounds__(256) pose_sums_kernel(const PoseArgs a, const float* __restrict__ pose)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * 256 + t;
    const size_t si = (size_t)i;
    float v[POSE_SUMS];
#pragma unroll
    for (int k = 0; k < POSE_SUMS; k++) v[k] = 0.f;

    if (i < a.P && a.radii[i] > 0) {
        const float g[3] = { a.dL_dmeans3D[3 * si], a.dL_dmeans3D[3 * si + 1], a.dL_dmeans3D[3 * si + 2] };
        float dc[6];
#pragma unroll
        for (int q = 0; q < 6; q++) dc[q] = a.dL_dcov3D[6 * si + q];
        float dcol[3] = { 0.f, 0.f, 0.f };
        if (DEG > 0) { dcol[0] = a.dL_dcolors[3 * si]; dcol[1] = a.dL_dcolors[3 * si + 1]; dcol[2] = a.dL_dcolors[3 * si + 2]; }
        const bool any_geom = g[0] != 0.f || g[1] != 0.f || g[2] != 0.f || dc[0] != 0.f || dc[1] != 0.f || dc[2] != 0.f ||
                              dc[3] != 0.f || dc[4] != 0.f || dc[5] != 0.f;
        const bool any_col = dcol[0] != 0.f || dcol[1] != 0.f || dcol[2] != 0.f;
        if (any_geom || any_col) {
            const f3 m = { a.means3D[3 * si], a.means3D[3 * si + 1], a.means3D[3 * si + 2] };
            ScaleRotRow w;                                         // Sigma exactly as preprocess_kernel builds it
            load_scale_rot_row(a.cov3D_precomp, a.scales, a.rotations, a.scale_factors, a.g_indices, si, a.scale_modifier, w);
            const float* cov3D = w.cov3D;
            float gdir[3] = { 0.f, 0.f, 0.f };
            if (DEG > 0 && any_col) {
                constexpr int NC = (DEG + 1) * (DEG + 1) * 3;
                const size_t row = a.sh_indices ? (size_t)a.sh_indices[i] : si;
                // scalar loads, not gsgrad.hpp's load_sh_row(): with its 16-byte loads the degree-3 kernel needs 136 VGPRs and
                // three waves per SIMD fit instead of four (0.118 -> 0.141 ms at P = 3M, profiles/gsgrad/README.md)
                const float* shp = a.sh + row * (size_t)a.M * 3;
                float c[NC];
#pragma unroll
                for (int q = 0; q < NC; q++) c[q] = shp[q];
                const uint8_t cl = a.clamped[i];
                const float gc[3] = { (cl & 1) ? 0.f : dcol[0], (cl & 2) ? 0.f : dcol[1], (cl & 4) ? 0.f : dcol[2] };
                const PoseCamera cam = pose_camera(pose);
                const f3 d0 = { m.x - cam.campos[0], m.y - cam.campos[1], m.z - cam.campos[2] };
                sh_view_dir_grad<DEG>(c, d0, gc, gdir);
            }
            const float mu[3] = { m.x, m.y, m.z };
            const float Sg[3][3] = { { cov3D[0], cov3D[1], cov3D[2] }, { cov3D[1], cov3D[3], cov3D[4] }, { cov3D[2], cov3D[4], cov3D[5] } };
            // G + G^T: twice the diagonal; an off-diagonal entry of the six already is the sum of its two positions
            const float G2[3][3] = { { 2.f * dc[0], dc[1], dc[2] }, { dc[1], 2.f * dc[3], dc[4] }, { dc[2], dc[4], 2.f * dc[5] } };
#pragma unroll
            for (int r = 0; r < 3; r++) {
                v[r] = g[r];
                v[3 + r] = gdir[r];
                const float gp = g[r] - gdir[r];
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    v[6 + 3 * r + q] = gp * mu[q];
                    v[15 + 3 * r + q] = G2[r][0] * Sg[0][q] + G2[r][1] * Sg[1][q] + G2[r][2] * Sg[2][q];
                }
            }
        }
    }

    // the wave's 64 lanes by a fixed butterfly, then the four waves in ascending order: the order of every float sum is the
    // network's, not the timing's
    __shared__ float s_w[4][POSE_SUMS];
#pragma unroll
    for (int k = 0; k < POSE_SUMS; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < POSE_SUMS; k++) s_w[wave][k] = v[k];
    }
    __syncthreads();
    if (t < POSE_SUMS) a.rows[(size_t)blockIdx.x * POSE_SUMS + t] = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
}

// ---- stage B: thread (r, k) = (t / 24, t % 24) adds rows r, r + 42, r + 84, ... of column k in double (a sweep of the 1008
// working threads is 42 whole rows: consecutive floats, coalesced); column k's 42 partial sums are then added in ascending r.
// Which rows meet in which order depends on n_rows alone. Lane 0 finishes.
__global__ void __launch_bounds__(1024) pose_fold_kernel(int n_rows, const float* __restrict__ rows, const float* __restrict__ pose,
                                                         float* __restrict__ out)
{
    __shared__ double s_part[POSE_FOLD_ROWS][POSE_SUMS];
    __shared__ double s_sum[POSE_SUMS];
    const int t = threadIdx.x;
    if (t < POSE_FOLD_THREADS) {
        const int r = t / POSE_SUMS, k = t - r * POSE_SUMS;
        double acc = 0.0;
#pragma unroll 8
        for (int row = r; row < n_rows; row += POSE_FOLD_ROWS) acc += (double)rows[(size_t)row * POSE_SUMS + k];
        s_part[r][k] = acc;
    }
    __syncthreads();
    if (t < POSE_SUMS) {
        double acc = 0.0;
        for (int r = 0; r < POSE_FOLD_ROWS; r++) acc += s_part[r][t];
        s_sum[t] = acc;
    }
    __syncthreads();
    if (t != 0) return;

    const PoseCamera cam = pose_camera(pose);
    const double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
    const double* Sg = s_sum;
    const double* Sd = s_sum + 3;
    // S = M1 + M2 + S_d c^T, then dL/dR = R^-T S and dL/dt = R^-T S_g
    double S[3][3], D[3][3], dt[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) S[r][q] = s_sum[6 + 3 * r + q] + s_sum[15 + 3 * r + q] + Sd[r] * (double)cam.campos[q];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int q = 0; q < 3; q++) D[r][q] = cam.inv[0][r] * S[0][q] + cam.inv[1][r] * S[1][q] + cam.inv[2][r] * S[2][q];
        dt[r] = cam.inv[0][r] * Sg[0] + cam.inv[1][r] * Sg[1] + cam.inv[2][r] * Sg[2];
    }
    // through the entries of quat_to_mat: R00 = 1 - 2 (y^2 + z^2), R01 = 2 (x y - w z), R02 = 2 (x z + w y), R10 = 2 (x y + w z),
    // R11 = 1 - 2 (x^2 + z^2), R12 = 2 (y z - w x), R20 = 2 (x z - w y), R21 = 2 (y z + w x), R22 = 1 - 2 (x^2 + y^2)
    const double dqx = 2.0 * (y * (D[0][1] + D[1][0]) + z * (D[0][2] + D[2][0]) + w * (D[2][1] - D[1][2])) - 4.0 * x * (D[1][1] + D[2][2]);
    const double dqy = 2.0 * (x * (D[0][1] + D[1][0]) + z * (D[1][2] + D[2][1]) + w * (D[0][2] - D[2][0])) - 4.0 * y * (D[0][0] + D[2][2]);
    const double dqz = 2.0 * (x * (D[0][2] + D[2][0]) + y * (D[1][2] + D[2][1]) + w * (D[1][0] - D[0][1])) - 4.0 * z * (D[0][0] + D[1][1]);
    const double dqw = 2.0 * (z * (D[1][0] - D[0][1]) + y * (D[0][2] - D[2][0]) + x * (D[2][1] - D[1][2]));
    // + 0.0: a sum of signed zeros (nothing visible) comes out as +0
    out[0] = (float)(dqx + 0.0); out[1] = (float)(dqy + 0.0); out[2] = (float)(dqz + 0.0); out[3] = (float)(dqw + 0.0);
    out[4] = (float)(dt[0] + 0.0); out[5] = (float)(dt[1] + 0.0); out[6] = (float)(dt[2] + 0.0);
}

size_t pose_grad_workspace_bytes(int P)
{
    const size_t n_rows = ((size_t)(P > 0 ? P : 1) + 255) / 256;
    return align_up(n_rows * POSE_SUMS * sizeof(float));
}

void launch_pose_sums(const PoseGradIn& in, float* rows, hipStream_t s)
{
    PoseArgs a;
    a.P = in.P; a.M = in.M; a.scale_modifier = in.scale_modifier;
    a.means3D = in.means3D; a.dL_dmeans3D = in.dL_dmeans3D; a.dL_dcov3D = in.dL_dcov3D; a.dL_dcolors = in.dL_dcolors;
    a.sh = in.sh; a.sh_indices = in.sh_indices; a.cov3D_precomp = in.cov3D_precomp; a.scales = in.scales; a.rotations = in.rotations;
    a.scale_factors = in.scale_factors; a.g_indices = in.g_indices; a.clamped = in.clamped; a.radii = in.radii; a.rows = rows;
    const int grid = (in.P + 255) / 256;
    switch (in.sh ? in.D : 0) {
        case 0: pose_sums_kernel<0><<<grid, 256, 0, s>>>(a, in.pose); break;
        case 1: pose_sums_kernel<1><<<grid, 256, 0, s>>>(a, in.pose); break;
        case 2: pose_sums_kernel<2><<<grid, 256, 0, s>>>(a, in.pose); break;
        default: pose_sums_kernel<3><<<grid, 256, 0, s>>>(a, in.pose); break;
    }
}

void launch_pose_fold(int P, const float* rows, const float* pose, float* out, hipStream_t s)
{
    pose_fold_kernel<<<1, 1024, 0, s>>>((P + 255) / 256, rows, pose, out);
}

} // namespace c3dgs
