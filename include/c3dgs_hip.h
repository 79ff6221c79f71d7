/*
 * c3dgs_hip.h -- C ABI of libc3dgs_hip.so: the MI355X (gfx950) rasterizer + VQ hot path.
 *
 * This is the drop-in boundary for the reference's two native extensions
 *   diff_gaussian_rasterization*._C   (submodules/diff-gaussian-rasterization/ext.cpp:15-21,
 *                                      signatures rasterize_points.h:18-122)
 *   weighted_distance._C              (submodules/weighted_distance/ext.cpp:4-6)
 * restated with plain pointers and sizes: no torch types, no C++ types, no CUDA/HIP types.
 * Every pointer is a DEVICE pointer unless marked "host". `stream` is a hipStream_t passed as
 * void* (NULL = the default stream). Every function returns 0 on success and a non-zero
 * C3DGS_E_* code on failure; c3dgs_last_error() then returns a message (thread-local).
 *
 * "Empty tensor" semantics of the reference (torch.Tensor([]) -> data_ptr()==nullptr,
 * forward.cu:214,250; backward.cu:390,394) are kept: an absent optional input is a NULL pointer.
 */
#ifndef C3DGS_HIP_H
#define C3DGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C3DGS_ABI_VERSION 4

enum {
    C3DGS_OK = 0,
    C3DGS_E_INVALID = 1, /* bad shape / missing or contradictory arguments (reference: AT_ERROR)   */
    C3DGS_E_HIP = 2,     /* a HIP runtime or kernel error (reference: CHECK_CUDA under debug=True) */
    C3DGS_E_ALLOC = 3    /* a resize callback returned NULL                                         */
};

/* Scratch buffers are owned by the caller and grown through a callback, exactly like the
 * reference's std::function<char*(size_t)> resize lambdas (rasterize_points.cu:27-33,74-79;
 * rasterizer.h:31-34). The callback must return a device pointer to at least `bytes` bytes,
 * 256-byte aligned, that stays valid until the matching backward has run. */
typedef void* (*c3dgs_resize_fn)(void* user, size_t bytes);

/* Inputs shared by forward and backward (reference: the positional arguments of
 * RasterizeGaussiansCUDA / RasterizeGaussiansIndexedCUDA, rasterize_points.cu:35-56,
 * rasterize_points_indexed.cu:35-59). */
typedef struct c3dgs_raster_params {
    int32_t P;      /* Gaussians passed in                                                   */
    int32_t D;      /* active SH degree (0..3)                                               */
    int32_t M;      /* SH coefficients per row = sh.size(1); 0 when sh is absent             */
    int32_t W, H;   /* image size                                                            */
    int32_t SHS;    /* rows of the SH codebook   (indexed variant; else == P or 0)           */
    int32_t GS;     /* rows of the scale/rotation codebooks (indexed variant; else == P or 0) */
    const float* background;     /* [3]                                                      */
    const float* means3D;        /* [P,3]                                                    */
    const float* sh;             /* [P,M,3] | indexed: [SHS,M,3] | NULL                      */
    const float* colors_precomp; /* [P,3] | NULL        (exactly one of sh / colors_precomp) */
    const float* opacities;      /* [P]                                                      */
    const float* scales;         /* [P,3] | indexed: [GS,3] | NULL                           */
    const float* scale_factors;  /* indexed only: [P]                                        */
    const float* rotations;      /* [P,4] | indexed: [GS,4] | NULL   (r,x,y,z), not normalised */
    const float* cov3D_precomp;  /* [P,6] | NULL   (exactly one of scales+rotations / cov3D)  */
    const int64_t* sh_indices;   /* indexed only: [P]                                        */
    const int64_t* g_indices;    /* indexed only: [P]                                        */
    const float* viewmatrix;     /* [16] world->camera, transposed (m[0],m[4],m[8],m[12] = row 0) */
    const float* projmatrix;     /* [16] viewmatrix @ projection, same layout                */
    const float* campos;         /* [3]                                                      */
    float tan_fovx, tan_fovy;
    float scale_modifier;
    int32_t prefiltered;
    int32_t clamp_color;
    int32_t debug;               /* non-zero: synchronise and check after every stage        */
} c3dgs_raster_params;

/* Gradient outputs (reference: the tensors allocated in RasterizeGaussiansBackward*CUDA,
 * rasterize_points.cu:153-162, rasterize_points_indexed.cu:166-176). The callee writes EVERY
 * element of every non-NULL output (zeros for culled Gaussians), so the caller may pass
 * uninitialised memory. A NULL pointer skips that output. */
typedef struct c3dgs_raster_grads {
    float* dL_dmeans2D;       /* [P,3]  (z component is always 0)                             */
    float* dL_dcolors;        /* [P,3]                                                        */
    float* dL_dopacity;       /* [P]                                                          */
    float* dL_dmeans3D;       /* [P,3]                                                        */
    float* dL_dcov3D;         /* [P,6]                                                        */
    float* dL_dsh;            /* [P,M,3] | indexed: [SHS,M,3] (scatter-added)                 */
    float* dL_dscales;        /* [P,3]   | indexed: [GS,3]    (scatter-added)                 */
    float* dL_dscale_factors; /* indexed only: [P]                                            */
    float* dL_drotations;     /* [P,4]   | indexed: [GS,4]    (scatter-added)                 */
} c3dgs_raster_grads;

/* ---- camera set-up of the reference's autograd wrappers, on the device (DGR-NC .../__init__.py:32-40 quat_to_mat,
 * :19-30 getProjectionMatrix, :152-172 `extrinsic @ getProjectionMatrix(intrinsic)` and `extrinsic.inverse()[3, :3]`).
 * extrinsic_vector = device float[7] (qx, qy, qz, qw, tx, ty, tz), read in stream order -- the matrices always belong
 * to the pose's CURRENT values, whatever wrote them. inv_tan_half_fov* = 1 / tan(FoV / 2) as fp32 (the two
 * intrinsic-dependent entries of getProjectionMatrix). Outputs: viewmatrix[16], projmatrix[16] (both transposed like
 * the reference's), campos[3]. */
int c3dgs_camera_from_pose(const float* extrinsic_vector, float inv_tan_half_fovx, float inv_tan_half_fovy,
                           float* viewmatrix, float* projmatrix, float* campos, void* stream);

/* ---- _C.mark_visible (rasterize_points.cu:202-221 -> rasterizer_impl.cu:54-66,141-149) ---- */
int c3dgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                       uint8_t* present /*[P] bool*/, void* stream);
/* The same test from the camera's POSE (device pointer to qx, qy, qz, qw, tx, ty, tz: what GaussianRasterizer*.markVisible is
 * handed, DGR-NC __init__.py:937-949): the matrix entries the test reads are formed per thread with the fp32 operations of
 * c3dgs_camera_from_pose, so the flags equal c3dgs_camera_from_pose + c3dgs_mark_visible bit for bit, in one launch. */
int c3dgs_mark_visible_pose(int32_t P, const float* means3D, const float* extrinsic_vector, uint8_t* present /*[P] bool*/,
                            void* stream);

/* ---- _C.rasterize_gaussians (rasterize_points.cu:35-117 -> rasterizer_impl.cu:194-334) ----
 * p->sh_indices, p->g_indices, p->scale_factors must be NULL.
 * out_color [3,H,W] and radii [P] are fully written. *num_rendered (host) receives R. */
int c3dgs_rasterize_gaussians(const c3dgs_raster_params* p,
                              c3dgs_resize_fn geom_resize, void* geom_user,
                              c3dgs_resize_fn binning_resize, void* binning_user,
                              c3dgs_resize_fn image_resize, void* image_user,
                              float* out_color, int32_t* radii, int32_t* num_rendered /*host*/, void* stream);

/* ---- _C.rasterize_gaussians_indexed (rasterize_points_indexed.cu:35-123 -> rasterizer_impl.cu:440-586) */
int c3dgs_rasterize_gaussians_indexed(const c3dgs_raster_params* p,
                                      c3dgs_resize_fn geom_resize, void* geom_user,
                                      c3dgs_resize_fn binning_resize, void* binning_user,
                                      c3dgs_resize_fn image_resize, void* image_user,
                                      float* out_color, int32_t* radii, int32_t* num_rendered /*host*/, void* stream);

/* ---- _C.rasterize_gaussians_backward (rasterize_points.cu:119-200 -> rasterizer_impl.cu:338-435) ----
 * geom/binning/image buffers are the ones the forward filled; R is the forward's num_rendered.
 * `workspace_resize` provides the backward's own scratch (per-instance partial sums). */
int c3dgs_rasterize_gaussians_backward(const c3dgs_raster_params* p, const int32_t* radii,
                                       const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                       int32_t R, const float* dL_dout_color /*[3,H,W]*/,
                                       c3dgs_resize_fn workspace_resize, void* workspace_user,
                                       const c3dgs_raster_grads* grads, void* stream);

/* ---- _C.rasterize_gaussians_backward_indexed (rasterize_points_indexed.cu:125-218 -> rasterizer_impl.cu:590-697) */
int c3dgs_rasterize_gaussians_backward_indexed(const c3dgs_raster_params* p, const int32_t* radii,
                                               const void* geom_buffer, const void* binning_buffer,
                                               const void* image_buffer, int32_t R, const float* dL_dout_color,
                                               c3dgs_resize_fn workspace_resize, void* workspace_user,
                                               const c3dgs_raster_grads* grads, void* stream);

/* ---- the two backward entries with gradients through the depth and alpha maps of c3dgs_render_depth
 * (csrc/render_maps_backward.hip; no reference counterpart) ----
 * The arguments of the entries above plus dL_ddepth and dL_dalpha, [H,W] fp32 device maps: dL/d(out_depth) and dL/d(out_alpha)
 * of the forward that filled the buffers. Either may be NULL (zeros). out_median is piecewise constant: no gradient.
 * With both maps NULL the call IS the entry above: the same validation, workspace request, launches and bits.
 * With a map, dL_dout_color may be NULL (the loss does not use the image): then the colour blend launch is left out. Per pixel,
 * over the entries k the forward blended, with c_k = dL_ddepth z_k + dL_dalpha:
 *   dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k),      dL/dz_g = sum over the pixels of w_k dL_ddepth
 * and from dL/dalpha_k the chain of the colour backward (its clamp, skip and stop conventions; dL_dmeans2D in its units). One blend
 * replay (stage "render_depth_backward") adds its sums into the colour backward's per-(Gaussian, tile) partial sums in front of
 * "backward_preprocess", which then writes every gradient of `grads` as always; one small launch behind it (stage
 * "depth_backward_fold") adds dL/dz_g x the depth row of p->viewmatrix into grads->dL_dmeans3D (skipped when that is NULL).
 * No float atomics beyond the colour backward's own codebook scatter-adds; without those (non-indexed) bitwise reproducible.
 * The workspace callback is asked for c3dgs_depth_backward_workspace_bytes(P, R): the backward's layout, unchanged, and behind it
 * the dL/dz plane, f32 [max(R, 1)]. The sort's time-out word set: the replay walks nothing and the fold writes NaN. */
int c3dgs_rasterize_gaussians_backward_depth(const c3dgs_raster_params* p, const int32_t* radii,
                                             const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                             int32_t R, const float* dL_dout_color /*[3,H,W] | NULL with a map*/,
                                             const float* dL_ddepth /*[H,W] | NULL*/, const float* dL_dalpha /*[H,W] | NULL*/,
                                             c3dgs_resize_fn workspace_resize, void* workspace_user,
                                             const c3dgs_raster_grads* grads, void* stream);
int c3dgs_rasterize_gaussians_backward_depth_indexed(const c3dgs_raster_params* p, const int32_t* radii,
                                                     const void* geom_buffer, const void* binning_buffer,
                                                     const void* image_buffer, int32_t R, const float* dL_dout_color,
                                                     const float* dL_ddepth, const float* dL_dalpha,
                                                     c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                     const c3dgs_raster_grads* grads, void* stream);
size_t c3dgs_depth_backward_workspace_bytes(int32_t P, int32_t R);

/* ---- the depth-distortion map of a finished forward (csrc/render_distortion.hip; no reference counterpart) ----
 * Mip-NeRF 360's distortion regulariser as 2DGS and gsplat use it. Per pixel, over the entries k = 1..m the forward blended
 * (w_k, T_k, z_k as for c3dgs_render_depth), with s_k = f(z_k):
 *   far <= 0:       raw mode, f(z) = z (near is not looked at)
 *   0 < near < far: ndc mode, f(z) = far / (far - near) * (1 - near / z), 2DGS's mapping (anything else: C3DGS_E_INVALID)
 *   out_distortion = sum_i sum_j w_i w_j |s_i - s_j| = 2 sum_k w_k (s_k A_<k - S_<k),  A_<k = 1 - T_k, S_<k = sum_{j<k} w_j s_j
 *   out_moment     = sum_k w_k s_k        (what the backward entries below take as `moment`)
 * The second form is the one evaluated: a tile's list is in ascending fp32 depth and f is increasing. There is no
 * 1/3 sum w^2 delta term. The call replays the forward's decisions, reads what c3dgs_render_depth reads and, like it, is valid
 * before or after the matching backward; no atomics, no scratch, bitwise reproducible. out_distortion is required, out_moment may
 * be NULL. P == 0 or R == 0: zeros, no blend launch. The sort's time-out word set: every output is NaN.
 * Stage name: "render_distortion". */
int c3dgs_render_distortion(int32_t P, int32_t W, int32_t H, int32_t R,
                            const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                            float near, float far, float* out_distortion /*[H,W]*/, float* out_moment /*[H,W] | NULL*/,
                            void* stream);

/* ---- the two backward entries with gradients through the depth, alpha AND distortion maps
 * (csrc/render_maps_backward.hip) ----
 * The arguments of the *_backward_depth entries plus dL_ddistortion = dL/d(out_distortion) and moment = out_moment of
 * c3dgs_render_distortion on the same forward, both [H,W] fp32, and that call's near / far.
 * With dL_ddistortion NULL the call IS the *_backward_depth entry: the same validation, workspace request, launches and bits
 * (moment, near and far are not looked at). With it, moment is required and near / far are checked as above; errors return
 * C3DGS_E_INVALID before any device work. Per pixel, with gL = dL_ddistortion, A_>k = T_{k+1} - T_{m+1} and
 * S_>k = moment - S_<k - w_k s_k:
 *   u_k         = 2 gL (s_k (A_<k - A_>k) - S_<k + S_>k)                  c_k = dL_ddepth z_k + dL_dalpha + u_k
 *   dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k)           dL/dz_k = w_k (dL_ddepth + 2 gL (A_<k - A_>k) f'(z_k))
 * ONE blend replay (stage "render_distortion_backward") serves the three maps and stands in the place of
 * "render_depth_backward", which is not launched; "depth_backward_fold" follows as there. The workspace callback is asked for
 * c3dgs_distortion_backward_workspace_bytes(P, R) == c3dgs_depth_backward_workspace_bytes(P, R). */
int c3dgs_rasterize_gaussians_backward_distortion(const c3dgs_raster_params* p, const int32_t* radii,
                                                  const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                                  int32_t R, const float* dL_dout_color /*[3,H,W] | NULL with a map*/,
                                                  const float* dL_ddepth /*[H,W] | NULL*/, const float* dL_dalpha /*[H,W] | NULL*/,
                                                  const float* dL_ddistortion /*[H,W] | NULL*/, const float* moment /*[H,W]*/,
                                                  float near, float far,
                                                  c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                  const c3dgs_raster_grads* grads, void* stream);
int c3dgs_rasterize_gaussians_backward_distortion_indexed(const c3dgs_raster_params* p, const int32_t* radii,
                                                          const void* geom_buffer, const void* binning_buffer,
                                                          const void* image_buffer, int32_t R, const float* dL_dout_color,
                                                          const float* dL_ddepth, const float* dL_dalpha,
                                                          const float* dL_ddistortion, const float* moment, float near, float far,
                                                          c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                          const c3dgs_raster_grads* grads, void* stream);
size_t c3dgs_distortion_backward_workspace_bytes(int32_t P, int32_t R);

/* ---- normal maps (csrc/normals.hip, csrc/render_normal.hip, csrc/render_maps_backward.hip; no reference counterpart) ----
 * All normals are in VIEW space: x right, y down, z forward, the frame of `viewmatrix`.
 *
 * c3dgs_gaussian_normals: one lane per Gaussian. With q = rotations[g], s = scales[g] (g_indices NULL) or the codebook rows
 * rotations[g_indices[g]], scales[g_indices[g]]:
 *   m = argmin_j s[j] on the RAW row (no scale modifier, no scale factor), the lowest j on a tie
 *   c = column m of the rotation matrix of q as preprocess builds it (q is not normalised); v = R_view c / |c|, 0 where |c| == 0
 *   n = sigma v, sigma = -1 where v . p > 0 for the view-space mean p, else +1: the normal faces the camera
 *   out_normals[g] = {n_x, n_y, n_z, sigma (m + 1)}
 * Every row is written, whether preprocess culled the Gaussian or not. Run it on the forward's stream. Stage "gaussian_normals".
 *
 * c3dgs_render_normal: out_normal[c] = sum_k w_k n_k,c over the entries the forward blended (w_k, T_k as for c3dgs_render_depth),
 * accumulated like a colour channel of the forward; not normalised, no background term. A replay of the forward's decisions,
 * valid before or after the matching backward; no atomics, bitwise reproducible. P == 0 or R == 0: zeros, no blend launch. The
 * sort's time-out word set: NaN. Stage "render_normal". */
int c3dgs_gaussian_normals(int32_t P, const float* means3D /*[P,3]*/, const float* scales, const float* rotations,
                           const int64_t* g_indices /*[P] | NULL*/, const float* viewmatrix /*[16]*/,
                           float* out_normals /*[P,4]*/, void* stream);
int c3dgs_render_normal(int32_t P, int32_t W, int32_t H, int32_t R,
                        const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                        const float* normals /*[P,4]*/, float* out_normal /*[3,H,W]*/, void* stream);

/* ---- the two backward entries with a gradient through the normal map (csrc/render_maps_backward.hip) ----
 * The arguments of the *_backward_distortion entries plus dL_dnormal = dL/d(out_normal), [3,H,W] fp32, and normals = the buffer
 * c3dgs_gaussian_normals filled for the same forward.
 * With dL_dnormal NULL the call IS the *_backward_distortion entry (normals and the three axes arguments are not looked at). With
 * it, normals is required. The fold chains to the rotations the normals were made from. axes_rotations NULL: those are
 * p->rotations under p->g_indices, the gradient goes into grads->dL_drotations, and p->cov3D_precomp must be NULL (a covariance
 * has no axes). axes_rotations not NULL: the call may blend a precomputed covariance (a filtered one, say) while the normals come
 * from these rows, [P,4] or a codebook under axes_g_indices ([P] | NULL); the gradient is ADDED into dL_daxes_rotations (required
 * then, of the shape of axes_rotations, zeroed by the caller) and grads->dL_drotations is left to the rest of the backward.
 * Violations: C3DGS_E_INVALID before any device work. Then
 *   c_k += dL_dnormal . n_k     in the recurrences of the depth / distortion entries (the pivoted ones where dL_ddistortion is set)
 * and ONE blend replay (stage "render_normal_backward") serves every map of the call: it stands in the place of
 * "render_depth_backward" / "render_distortion_backward", neither of which is launched. Behind "backward_preprocess" and
 * "depth_backward_fold", "normal_backward_fold" chains dL/dn_g = sum w_k dL_dnormal to the quaternion (the 1 / |c| included; m and
 * sigma carry no gradient, and none flows to the mean, the scales or the pose) and ADDS it into dL_drotations: the Gaussian's
 * own row, or the codebook row of the indexed entry. The workspace callback is asked for
 * c3dgs_normal_backward_workspace_bytes(P, R): the depth entries' layout and behind it three floats per slot. */
int c3dgs_rasterize_gaussians_backward_normal(const c3dgs_raster_params* p, const int32_t* radii,
                                              const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                              int32_t R, const float* dL_dout_color /*[3,H,W] | NULL with a map*/,
                                              const float* dL_ddepth /*[H,W] | NULL*/, const float* dL_dalpha /*[H,W] | NULL*/,
                                              const float* dL_dnormal /*[3,H,W] | NULL*/, const float* normals /*[P,4]*/,
                                              const float* axes_rotations /*NULL | rows x 4*/,
                                              const int64_t* axes_g_indices /*NULL | [P]*/,
                                              float* dL_daxes_rotations /*NULL | rows x 4, zeroed*/,
                                              const float* dL_ddistortion /*[H,W] | NULL*/, const float* moment /*[H,W]*/,
                                              float near, float far,
                                              c3dgs_resize_fn workspace_resize, void* workspace_user,
                                              const c3dgs_raster_grads* grads, void* stream);
int c3dgs_rasterize_gaussians_backward_normal_indexed(const c3dgs_raster_params* p, const int32_t* radii,
                                                      const void* geom_buffer, const void* binning_buffer,
                                                      const void* image_buffer, int32_t R, const float* dL_dout_color,
                                                      const float* dL_ddepth, const float* dL_dalpha,
                                                      const float* dL_dnormal, const float* normals,
                                                      const float* axes_rotations, const int64_t* axes_g_indices,
                                                      float* dL_daxes_rotations,
                                                      const float* dL_ddistortion, const float* moment, float near, float far,
                                                      c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                      const c3dgs_raster_grads* grads, void* stream);
size_t c3dgs_normal_backward_workspace_bytes(int32_t P, int32_t R);

/* ---- the normal of a depth map (csrc/normals.hip) ----
 * z[H,W] = view-space depths. P(x, y) = z(x, y) ((x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, 1) with fx = W / (2 tan_fovx),
 * fy = H / (2 tan_fovy). Interior pixels: normalize(cross(P(x, y + 1) - P(x, y - 1), P(x + 1, y) - P(x - 1, y))) with
 * normalize(c) = c / max(|c|, 1e-12): a fronto-parallel plane gives (0, 0, -1). The one-pixel border is 0 (W < 3 or H < 3: all).
 * The backward gathers, per pixel, the at most four stencils that read it: dL_dz[H,W] is written everywhere, no atomics.
 * One launch each: stages "depth_to_normal", "depth_to_normal_backward". */
int c3dgs_depth_to_normal(int32_t W, int32_t H, const float* z /*[H,W]*/, float tan_fovx, float tan_fovy,
                          float* out_normal /*[3,H,W]*/, void* stream);
int c3dgs_depth_to_normal_backward(int32_t W, int32_t H, const float* z /*[H,W]*/, const float* dL_dnormal /*[3,H,W]*/,
                                   float tan_fovx, float tan_fovy, float* dL_dz /*[H,W]*/, void* stream);

/* ---- depth, accumulated opacity and median depth of a finished forward (csrc/render_depth.hip; no reference counterpart) ----
 * geom/binning/image buffers are the ones a forward of the same P, W, H filled; R is its num_rendered. Per pixel, over the
 * entries k = 1..m the forward blended (w_k = alpha_k T_k, T_{k+1} = T_k (1 - alpha_k), T_1 = 1, z_k = the fp32 view-space
 * depth of the Gaussian):
 *   out_depth  = sum_k w_k z_k, accumulated like a colour channel of the forward; NOT normalised (divide by out_alpha)
 *   out_alpha  = 1 - T_{m+1}
 *   out_median = z_k of the first blended entry with T_{k+1} < 0.5, or 0 when T never falls below 0.5 (empty pixels too)
 * The call replays the forward's own decisions and is bitwise reproducible. It READS: the splat records and depth_keys of the
 * geometry buffer; ranges, the per-pixel / per-tile compact cuts (c3dgs_compact_layout: n_contrib_c, tile_used_c) of the image
 * buffer; the compact lists (cid, cqm) in the binning buffer's sort scratch; the device's sort time-out word (set: every
 * output is NaN, like the forward's image). It writes nothing but its outputs. The backward only reads those fields too (its
 * scratch in the image buffer is tile_order, which this call does not use), so the call is valid before or after the
 * matching backward, with the same result.
 * A NULL output is skipped; at least one must be non-NULL. P == 0 or R == 0: zeros, no blend launch. Forward-only: the
 * gradients of out_depth and out_alpha are what c3dgs_rasterize_gaussians_backward_depth(_indexed) take. Stage name: "render_depth". */
int c3dgs_render_depth(int32_t P, int32_t W, int32_t H, int32_t R,
                       const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                       float* out_depth /*[H,W] | NULL*/, float* out_alpha /*[H,W] | NULL*/,
                       float* out_median /*[H,W] | NULL*/, void* stream);

/* ---- per-Gaussian blend statistics of a finished forward (csrc/render_contrib.hip; no reference counterpart) ----
 * geom/binning/image buffers are the ones a forward of the same P, W, H filled; R is its num_rendered. For every Gaussian g,
 * over the (pixel, entry) pairs the forward BLENDED (a hit that passed the T test; the entry that only stopped a pixel is not
 * one), with w = alpha T in fp32 as c3dgs_render_depth forms it:
 *   out_weight_sum[g] = sum w      out_weight_max[g] = max w      out_hits[g] = number of such pairs
 * Rows of culled or never-blended Gaussians are exact zeros; every row of every non-NULL output is written. The call replays
 * the forward's own decisions like c3dgs_render_depth and reads what that call reads, plus block_base / inst_offset of the
 * geometry buffer (the backward's slot numbering). No float atomics: per-(Gaussian, tile) records go with plain stores to
 * `workspace` (c3dgs_contrib_workspace_bytes(P, R) bytes, 256-byte aligned; only its flag bytes are cleared, inside the call)
 * and a second kernel folds each Gaussian's run in slot order, so the result is bitwise reproducible. It writes nothing but
 * the workspace and its outputs: valid before or after the matching backward, with the same result, and the backward's own
 * workspace is not touched.
 * Sort time-out word set: every out_weight_sum / out_weight_max row is NaN, every out_hits row 0. A NULL output is skipped; at
 * least one must be non-NULL. P == 0 or R == 0: zeros, no blend launch. Argument errors return C3DGS_E_INVALID before any
 * device work. Stage name: "render_contrib" (the clear and both kernels; "render_contrib_blend" / "render_contrib_sum" are the
 * two kernels alone). */
size_t c3dgs_contrib_workspace_bytes(int32_t P, int32_t R);
int c3dgs_render_contrib(int32_t P, int32_t W, int32_t H, int32_t R,
                         const void* geom_buffer, const void* binning_buffer, const void* image_buffer, void* workspace,
                         float* out_weight_sum /*[P] | NULL*/, float* out_weight_max /*[P] | NULL*/,
                         uint32_t* out_hits /*[P] | NULL*/, void* stream);
/* One view's rows into model-sized accumulators, one launch: for model row i, r = rank[i] if visible[i] (the pair
 * c3dgs_qat_visible produces; rows not visible are left alone), or r = i when both are NULL (then P_rows == P_model):
 *   acc_sum[i] += weight_sum[r]; acc_max[i] = max(acc_max[i], weight_max[r]); acc_hits[i] += hits[r]; acc_views[i] += hits[r] > 0
 * NaN rows of a timed-out view propagate into acc_sum and acc_max. */
int c3dgs_contrib_accumulate(int32_t P_model, int32_t P_rows, const uint8_t* visible /*[P_model] | NULL*/,
                             const int32_t* rank /*[P_model] | NULL*/, const float* weight_sum, const float* weight_max,
                             const uint32_t* hits, float* acc_sum, float* acc_max, int64_t* acc_hits, uint32_t* acc_views,
                             void* stream);

/* ---- per-Gaussian error scores of a finished forward (csrc/render_error.hip; no reference counterpart) ----
 * geom/binning/image buffers are the ones a forward of the same P, W, H filled; R is its num_rendered; pixel_map is any finite
 * fp32 [H,W] map e. For every Gaussian g, over the (pixel, entry) pairs the forward BLENDED, with w = alpha T in fp32 as
 * c3dgs_render_contrib forms it:
 *   out_err_sum[g] = sum fl(w * e[pixel])
 * (two roundings per pair; the product is not fused into the sum). Rows of culled or never-blended Gaussians are exact zeros;
 * every row is written. The call reads what c3dgs_render_contrib reads, plus the map, once per pixel. It replays the forward's
 * own decisions, reduces with c3dgs_render_contrib's network, merges its waves and folds each Gaussian's run in that call's
 * order: a map of ones gives out_weight_sum's bits, and the result is bitwise reproducible (no float atomics). Per-(Gaussian,
 * tile) sums go with plain stores to `workspace` (c3dgs_error_workspace_bytes(P, R) bytes: R floats + R flag bytes, each region
 * 256-byte aligned; the base 256-byte aligned; only the flag bytes are cleared, inside the call). It writes nothing but the
 * workspace and its output: valid before or after the matching backward, with the same result; the backward's workspace and
 * c3dgs_render_contrib's are not touched.
 * Sort time-out word set: every row is NaN. P == 0 or R == 0: zeros, no blend launch. Argument errors (a NULL map, output,
 * buffer or workspace, negative sizes) return C3DGS_E_INVALID before any device work. Stage name: "render_error" (the clear and
 * both kernels; "render_error_blend" / "render_error_sum" are the two kernels alone). */
size_t c3dgs_error_workspace_bytes(int32_t P, int32_t R);
int c3dgs_render_error(int32_t P, int32_t W, int32_t H, int32_t R,
                       const void* geom_buffer, const void* binning_buffer, const void* image_buffer, void* workspace,
                       const float* pixel_map /*[H,W]*/, float* out_err_sum /*[P]*/, void* stream);
/* The usual map, one launch: out[y][x] = (|img[0][y][x] - gt[0][y][x]| + ... + |img[C-1][y][x] - gt[C-1][y][x]|) / (float)C
 * in fp32, channels added in ascending order, a correctly rounded division. img and gt are planar [C,H,W], contiguous; out is
 * [H,W]. Reads the two images, writes out and nothing else. C, H, W <= 0 or a NULL pointer: C3DGS_E_INVALID before any device
 * work. Stage name: "error_map_l1". */
int c3dgs_error_map_l1(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, float* out /*[H,W]*/, void* stream);
/* One view's row into model-sized accumulators, one launch: for model row i, r = rank[i] if visible[i] (the pair
 * c3dgs_qat_visible produces; rows not visible are left alone), or r = i when both are NULL (then P_rows == P_model):
 *   acc_max[i] = max(acc_max[i], err_sum[r]); acc_sum[i] += err_sum[r]
 * A NaN row of a timed-out view propagates into acc_max and acc_sum. */
int c3dgs_error_accumulate(int32_t P_model, int32_t P_rows, const uint8_t* visible /*[P_model] | NULL*/,
                           const int32_t* rank /*[P_model] | NULL*/, const float* err_sum, float* acc_max, float* acc_sum,
                           void* stream);

/* ---- exact gradient with respect to the camera's 7-element pose, behind a finished backward (csrc/pose_grad.hip; no reference
 * counterpart: the reference's pose gradient chains dL/dmeans2D alone through a projection formula) ----
 * pose = (qx, qy, qz, qw, tx, ty, tz) on the device, read by the call's kernels on the stream (nothing about it is cached on
 * the host); R, t, c = -R^-1 t are formed from it as c3dgs_camera_from_pose forms them, R is not assumed orthonormal. With
 * g_i = dL_dmeans3D[i], G_i = dL_dcov3D[i] as a full matrix (an off-diagonal entry of the six counts both symmetric positions),
 * gdir_i = the part of g_i that arrived through the SH view direction (recomputed from dL_dcolors, the forward's clamp flags in
 * the geometry buffer and the SH row; zero without SH or at degree 0), Sigma_i rebuilt as the forward built it:
 *   dL/dt = R^-T sum_i g_i
 *   dL/dR = R^-T [ sum_i (g_i - gdir_i) mu_i^T + sum_i (G_i + G_i^T) Sigma_i + (sum_i gdir_i) c^T ]
 * and out[7] = dL/dpose through the entries of the unnormalised-quaternion matrix. Rows with radii <= 0 are skipped. Inputs
 * are those of the forward / the outputs of its backward (dL_dcov3D and, with SH, dL_dcolors must have been written, not
 * skipped). Exactly one of cov3D_precomp and the pair (scales, rotations); g_indices and scale_factors come together (the indexed
 * path: codebook rows, scale = scale_factors x scale_modifier); sh_indices needs sh; sh needs dL_dcolors and M >= (D + 1)^2.
 * `workspace`: c3dgs_pose_grad_workspace_bytes(P) bytes (24 floats per 256 Gaussians), every word the call reads is written by
 * it first. No float atomics: bitwise reproducible. P == 0: seven zeros, no kernel. Argument errors return C3DGS_E_INVALID before
 * any device work. Stage name: "pose_grad" (both kernels; "pose_grad_sums" / "pose_grad_fold" alone). */
size_t c3dgs_pose_grad_workspace_bytes(int32_t P);
int c3dgs_pose_grad(int32_t P, int32_t D, int32_t M, float scale_modifier,
                    const float* means3D /*[P,3]*/, const float* dL_dmeans3D /*[P,3]*/, const float* dL_dcov3D /*[P,6]*/,
                    const float* dL_dcolors /*[P,3] | NULL without sh*/, const float* sh /*[SHS,M,3] | NULL*/,
                    const int64_t* sh_indices /*[P] | NULL*/, const float* cov3D_precomp /*[P,6] | NULL*/,
                    const float* scales /*[GS,3] | NULL*/, const float* rotations /*[GS,4] | NULL*/,
                    const float* scale_factors /*[P] | NULL*/, const int64_t* g_indices /*[P] | NULL*/,
                    const void* geom_buffer, const int32_t* radii /*[P]*/, const float* pose /*[7]*/, void* workspace,
                    float* out /*[7]*/, void* stream);

/* ---- antialiased rasterization: opacity compensation of the 0.3 px^2 low-pass (csrc/aa_opacity.hip; no reference counterpart:
 * upstream 3DGS `antialiasing`, Mip-Splatting, gsplat rasterize_mode="antialiased") ----
 * With (a0, b, c0) the 2D covariance the forward forms BEFORE it adds h = 0.3 to the diagonal (same T = W J, same clamp of
 * t.x, t.y at 1.3 tan_fov), in fp32, every operation rounded as the forward rounds it:
 *   D0 = a0 c0 - b b,  D1 = (a0 + h)(c0 + h) - b b,  r = D0 / D1,  rho = sqrt(max(0.000025f, r)),  opacity_out = opacity * rho
 * and the rasterizer is then called with opacity_out as p->opacities: radii, tile keys and conics are the plain render's.
 * rho is finite for every row: a row that fails the forward's near-plane test (view z <= 0.01 unless p->prefiltered), a row with
 * D1 == 0 and a row with a non-finite D0, D1 or r get rho = 1.
 * Both calls read of `p`: P, W, H, means3D, opacities (the RAW ones, also in the backward), tan_fovx, tan_fovy, scale_modifier,
 * viewmatrix, prefiltered, debug and either cov3D_precomp or scales + rotations -- rows of the latter two through g_indices,
 * multiplied by scale_factors x scale_modifier, when g_indices is not NULL (scale_factors without g_indices is ignored). SH,
 * colours, background, projmatrix and campos are ignored and may be NULL.
 * c3dgs_aa_opacity: one launch, one lane per Gaussian; writes opacity_out [P] and, when not NULL, rho [P].
 * c3dgs_aa_opacity_backward: one launch, queued BEHIND the whole backward (and its depth-map part) on the same stream, with that
 * backward's `grads` and the forward's radii. For every row with radii > 0 (the others' gradients are zero already), with g' the
 * value found in grads->dL_dopacity (the rasterizer's dL/d opacity_out): dL_dopacity is rewritten as rho g', and the terms through
 * rho -- dL/drho = opacity g', through sqrt and r to (a0, b, c0) and from there with the backward's own chain for the conic (T and
 * J, the clamped t.x, t.y held constant) -- are ADDED into whichever of dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drotations and
 * dL_dscale_factors are not NULL; these are exact derivatives (scale_modifier included). No such terms where rho = 1 by the rule
 * above or r <= 0.000025f. rho and these decisions are the fp32 values of c3dgs_aa_opacity; the terms through rho are evaluated in
 * double from the fp32 inputs and rounded once when added. A row whose g' is zero is left as it is (every term is a multiple of
 * g'). The covariance is recomputed: nothing is handed over from c3dgs_aa_opacity. P-sized outputs are plain
 * read-modify-writes; with g_indices, dL_dscales [GS,3] and dL_drotations [GS,4] are added with fp32 atomics (not reproducible
 * run to run, like the indexed backward's own). The other members of `grads` are not touched.
 * C3DGS_E_INVALID before any device work: P < 0; not exactly one of scales + rotations / cov3D_precomp; g_indices without
 * scale_factors; opacity_out NULL; grads or grads->dL_dopacity NULL; with cov3D_precomp a NULL grads->dL_dcov3D; and, for P > 0,
 * W or H <= 0 or a NULL means3D, opacities, viewmatrix or radii. P == 0 launches nothing. Stage names: "aa_opacity",
 * "aa_opacity_backward". */
int c3dgs_aa_opacity(const c3dgs_raster_params* p, float* opacity_out /*[P]*/, float* rho /*[P] | NULL*/, void* stream);
int c3dgs_aa_opacity_backward(const c3dgs_raster_params* p, const int32_t* radii /*[P]*/, const c3dgs_raster_grads* grads,
                              void* stream);

/* ---- the 3D smoothing filter of Mip-Splatting (csrc/filter3d.hip; no reference counterpart) ----
 * c3dgs_filter3d_compute: filter_3D [P] and, when not NULL, seen [P] over the camera table `cameras` [C, 16] (device memory; per
 * camera the rows 0..2 of the world -> camera matrix, row-major, then fx, fy, W, H). In fp32, each operation rounded on its own
 * in this order:  x = ((m0 px + m1 py) + m2 pz) + m3 (y, z likewise), u = (x / z) fx + W 0.5, v = (y / z) fy + H 0.5,
 * valid = z > 0.2 and -0.15 W <= u <= 1.15 W and -0.15 H <= v <= 1.15 H; dist = min over the valid cameras of z, for a Gaussian
 * no camera sees the maximum of dist over the seen ones (0 when none is seen); filter_3D = (dist / max over all cameras of fx)
 * float(sqrt(0.2)). Three stream operations (an 8-byte clear of the workspace and two kernels), no host read, no float atomics:
 * bitwise reproducible. `workspace`: c3dgs_filter3d_workspace_bytes(P) bytes, 8-byte aligned.
 * c3dgs_filter3d_apply: for the n rows of `r` (opacities [n], and either scales [n,3] + rotations [n,4] or, with g_indices [n],
 * codebooks addressed by it and scale_factors [n]), with f the row's filter value, sf its scale factor (1 without g_indices):
 *   cov3D_out = cov3D(scales, sf x scale_modifier, rotation) + (scale_modifier f)^2 on elements 0, 3, 5,
 *   s_k = sf scale_k, r_k = s_k^2 / (s_k^2 + f^2), opacity_out = opacity sqrt((r_0 r_1) r_2);
 * a row with f == 0 gets the plain covariance and its opacity bit for bit. Without `visible`, f = filter_3D[row] (filter_3D has n
 * rows). With `visible` [P_model] (bytes) and `rank` [P_model] (int32), the rows are the visible subset of a model: the kernel runs
 * one lane per model row i, and row rank[i] takes f = filter_3D[i] (filter_3D has P_model rows) where visible[i]; a rank outside
 * [0, n) is skipped. With cov3D_precomp [n,6], cov3D_out = cov3D_precomp + (scale_modifier f)^2 on elements 0, 3, 5: the scales
 * serve the opacity factor alone, rotations may be NULL, and the gradient of cov3D_precomp is dL_dcov3D itself (the backward
 * ignores g->dL_dcov3D and chains dL_dopacity_out only).
 * rotations and g->dL_drotations are read and written four floats at a time: both must be 16-byte aligned.
 * c3dgs_filter3d_apply_backward: from g->dL_dcov3D [n,6] (the gradient of cov3D_out) and g->dL_dopacity_out [n] (either may be
 * NULL = zeros), for the rows where one of them is non-zero -- the other rows of the outputs are NOT written, the caller hands in
 * zeros --: dL_dopacity = coef x dL_dopacity_out; the covariance gradient chained to scales, rotations and scale factors as the
 * rasterizer's backward chains it (exact in scale_modifier), plus the terms through coef,
 * dL/ds_k += opacity dL_dopacity_out coef f^2 / (s_k (s_k^2 + f^2)) unless s_k == 0 or f == 0. fp32 throughout. Row-sized outputs
 * are plain stores; with g_indices, dL_dscales [GS,3] and dL_drotations [GS,4] are ADDED with fp32 atomics (not reproducible run
 * to run) and dL_dscale_factors [n] is stored. NULL outputs are skipped.
 * C3DGS_E_INVALID before any device work: P or n < 0; C <= 0; for P > 0 a NULL xyz, cameras, filter_3D or workspace, or a workspace
 * that is too small or misaligned; r or g NULL; for n > 0 a NULL opacities, scales, filter_3D or (without cov3D_precomp)
 * rotations, a rotations or dL_drotations pointer that is not 16-byte aligned, g_indices without scale_factors, visible without rank or with P_model < 0, a NULL cov3D_out or opacity_out, or every output of the backward NULL.
 * P == 0 / n == 0 launch nothing. Stage names: "filter3d_compute", "filter3d_apply", "filter3d_apply_backward". */
typedef struct c3dgs_filter3d_rows {
    int32_t n, P_model;
    const float* opacities; const float* scales; const float* rotations; const float* scale_factors;
    const int64_t* g_indices;
    const float* cov3D_precomp;   /* [n,6] | NULL: the caller's covariance in place of the one scales and rotations build */
    const float* filter_3D; const uint8_t* visible; const int32_t* rank;
    float scale_modifier;
} c3dgs_filter3d_rows;
typedef struct c3dgs_filter3d_grads {
    const float* dL_dcov3D; const float* dL_dopacity_out;
    float* dL_dopacity; float* dL_dscales; float* dL_drotations; float* dL_dscale_factors;
} c3dgs_filter3d_grads;
size_t c3dgs_filter3d_workspace_bytes(int32_t P);
int c3dgs_filter3d_compute(int32_t P, int32_t C, const float* xyz /*[P,3]*/, const float* cameras /*[C,16]*/,
                           float* filter_3D /*[P]*/, uint8_t* seen /*[P] | NULL*/, void* workspace, size_t workspace_bytes,
                           void* stream);
int c3dgs_filter3d_apply(const c3dgs_filter3d_rows* r, float* cov3D_out /*[n,6]*/, float* opacity_out /*[n]*/, void* stream);
int c3dgs_filter3d_apply_backward(const c3dgs_filter3d_rows* r, const c3dgs_filter3d_grads* g, void* stream);

/* ---- mesh extraction: TSDF fusion of depth maps and marching tetrahedra (csrc/mesh.hip; no reference counterpart) ----
 * The volume: Nx x Ny x Nz lattice points at origin + (i, j, k) voxel_size, each component formed in fp32 as
 * origin + float(index) * voxel_size; fp32 planes [Nz, Ny, Nx] (x fastest, linear index (k Ny + j) Nx + i) owned by the caller and
 * zero before the first integration: tsdf, weight and optionally vol_color [3, Nz, Ny, Nx]. Nx Ny Nz <= 2^31 - 1.
 * c3dgs_tsdf_integrate: K depth maps [K, H, W] (view-space z; 0 = no measurement), optionally their colours [K, 3, H, W], and the
 * [K, 16] camera table of c3dgs_filter3d_compute (its W, H entries are the maps'). For every lattice point p and the cameras in
 * table order, in fp32, each operation rounded on its own:
 *   x = ((m0 px + m1 py) + m2 pz) + m3 (y, z likewise);  skip if z < depth_min;
 *   u = (fx x) / z + 0.5 W, v = (fy y) / z + 0.5 H;  skip unless 0 <= u < W and 0 <= v < H;  d = depth[c][int(v)][int(u)];
 *   skip unless 0 < d <= depth_max;  sdf = d - z;  skip if sdf < -sdf_trunc;  s = min(1, sdf / sdf_trunc);
 *   tsdf = (tsdf w + s) / (w + 1), each colour plane likewise with the pixel's colour;  w = w + 1.
 * One launch, no atomics, bitwise reproducible; K maps in one call give the bits of K calls of one map; a point no camera
 * updated is not stored. color and vol_color come as a pair. Stage name: "tsdf_integrate".
 * c3dgs_mesh_extract_count / c3dgs_mesh_extract_emit: marching tetrahedra over the cells whose eight corners all have weight > 0.
 * A cell is cut into the six Kuhn tetrahedra (0,0,0) -> +a -> +a+b -> (1,1,1), (a, b, c) the permutations of the axes in
 * lexicographic order; a corner is inside iff its value is < 0 (0.0 and -0.0 are outside). The vertex of the lattice edge
 * between the points a < b (linear index) is pa + t (pb - pa), t = va / (va - vb), colours likewise; it exists iff the endpoints
 * differ in sign and a valid cell contains the edge. Vertices are welded (one per edge) and ordered by the owner a, then by the
 * edge's slot +x, +y, +z, +xy, +xz, +yz, +xyz. With the path positions of the inside corners a < b and the outside ones c < d:
 * one inside corner gives (a o1, a o2, a o3), three the same about the outside corner, two give (ac, ad, bd) and (ac, bd, bc);
 * every triangle is wound so that its normal points from the negative to the positive side; zero-area triangles are kept.
 * count: two launches ("mesh_classify", "mesh_scan") and the one host read: counts[0] = vertices, counts[1] = faces (host memory;
 * the call synchronises the stream). emit: two launches ("mesh_emit_vertices", "mesh_emit_faces") that fill vertices [V, 3],
 * colors [V, 3] (with vol_color; both or neither) and faces [F, 3] for the V and F the count returned, from the SAME workspace,
 * untouched in between, and the same planes. workspace: c3dgs_mesh_extract_workspace_bytes(Nx, Ny, Nz) bytes (about five per
 * point), 256-byte aligned, content on entry irrelevant. V == 0 launches nothing. More than 2^31 - 1 vertices or faces is refused.
 * C3DGS_E_INVALID before any device work: l NULL; a dimension < 1; Nx Ny Nz > 2^31 - 1; voxel_size <= 0; a NULL tsdf or weight
 * plane; color without vol_color or the reverse; sdf_trunc <= 0; depth_min >= depth_max; K < 1; W or H < 1; NULL depth or cameras;
 * a NULL, small or misaligned workspace; NULL counts; V or F < 0; for V > 0 a NULL vertices, for F > 0 a NULL faces. */
typedef struct c3dgs_lattice {
    int32_t Nx, Ny, Nz;
    float ox, oy, oz, voxel_size;
} c3dgs_lattice;
int c3dgs_tsdf_integrate(const c3dgs_lattice* l, int32_t K, int32_t W, int32_t H, const float* depth /*[K,H,W]*/,
                         const float* color /*[K,3,H,W] | NULL*/, const float* cameras /*[K,16]*/, float sdf_trunc, float depth_min,
                         float depth_max, float* tsdf, float* weight, float* vol_color /*[3,Nz,Ny,Nx] | NULL*/, void* stream);
size_t c3dgs_mesh_extract_workspace_bytes(int32_t Nx, int32_t Ny, int32_t Nz);
int c3dgs_mesh_extract_count(const c3dgs_lattice* l, const float* tsdf, const float* weight, void* workspace,
                             size_t workspace_bytes, int64_t* counts /*host [2]*/, void* stream);
int c3dgs_mesh_extract_emit(const c3dgs_lattice* l, const float* tsdf, const float* weight, const float* vol_color /*| NULL*/,
                            void* workspace, size_t workspace_bytes, int64_t V, int64_t F, float* vertices /*[V,3]*/,
                            float* colors /*[V,3] | NULL*/, int32_t* faces /*[F,3]*/, void* stream);

/* ---- weighted_distance._C.weightedDistance (weighted_distance.cu:46-93) ----
 * coefs [N,K], codebook [C,K] row-major fp32 -> min squared distance [N] and argmin [N] (int64).
 * Exact reference semantics: fp32 k-ordered FMA chain, strict '<' (lowest index wins ties).
 * gather (optional, may be NULL): int64 [N] row indices into coefs, i.e. row n is coefs[gather[n]]
 * (fuses `features[batch]` of compression/vq.py:70). */
int c3dgs_weighted_distance(int64_t N, int32_t C, int32_t K, const float* coefs, const int64_t* gather,
                            const float* codebook, float* out_dist, int64_t* out_idx, void* stream);

/* the same with device scratch `ws` (16-byte aligned, c3dgs_weighted_distance_ws_bytes(N, C, K) bytes; less is legal):
 *   [the codebook scaled by one power of two per call and split into TWO fp16 pieces per value (v = h + l, h = fp16(v),
 *    l = fp16(v - h): 22 significant bits), laid out as matrix-core operand fragments, + the scaled ||c||^2 and the call's
 *    abs-max word][int32 list of the points whose two best candidates the fast search cannot tell apart].
 * With room for the split codebook (K = 48, 12 or 6; C >= 32) the candidate search runs on the fp16 matrix cores
 * (v_mfma_f32_32x32x16_f16) with THREE piece products per multiply (xh*ch + xh*cl + xl*ch; ~3 * 2^-22 relative error per
 * term); without, on the fp32 matrix cores. The scale puts the codebook's largest magnitude into [2^10, 2^11); whatever
 * leaves fp16's range after scaling (points far beyond the codebook's magnitude, inf, NaN) yields inf / NaN scores, fails
 * the margin test and is re-scanned exactly. Either way the winner's distance is recomputed with the reference's k-ordered
 * chain and every point inside the error margin is re-scanned exactly (listed points several per codebook pass): identical
 * results, distances and indices. */
size_t c3dgs_weighted_distance_ws_bytes(int64_t N, int32_t C, int32_t K);
int c3dgs_weighted_distance_ws(int64_t N, int32_t C, int32_t K, const float* coefs, const int64_t* gather,
                               const float* codebook, float* out_dist, int64_t* out_idx, void* ws, size_t ws_bytes,
                               void* stream);

/* ---- VectorQuantize.update, split at the point where a sharded run all-reduces (compression/vq.py:28-35) ----
 * accumulate: S[k, 0..D) += w_n * x_n ; S[k, D] += w_n for k = idx[n];  *dist_sum += sum_n dist[n] (may be NULL).
 * S [K, D+1] fp32 must be zeroed by the caller (it is the all-reduce payload). */
int c3dgs_vq_accumulate(int64_t B, int32_t K, int32_t D, const float* x, const float* w,
                        const int64_t* gather /*NULL, or row n of x and w is [gather[n]]*/,
                        const int64_t* idx, const float* dist, float* S, double* dist_sum, void* stream);

/* sums: the first half of a Lloyd step in ONE call -- clears S and *dist_sum, assigns the B (gathered) rows
 * (== c3dgs_weighted_distance into dist / idx) and accumulates them (== c3dgs_vq_accumulate).
 * ws / ws_bytes (optional): the scratch of c3dgs_weighted_distance_ws (c3dgs_weighted_distance_ws_bytes(B, K, D)); same
 * results without it. */
int c3dgs_vq_sums(int64_t B, int32_t K, int32_t D, const float* x, const float* w, const int64_t* gather,
                  const float* codebook, float* dist, int64_t* idx, float* S, double* dist_sum, void* ws, size_t ws_bytes,
                  void* stream);

/* ---- one Lloyd step of the loop of vq_features (compression/vq.py:68-77) in FIVE launches instead of eleven ----
 * The same two halves as c3dgs_vq_sums / c3dgs_vq_apply, for a loop that is the only writer of codebook, S and ws between its
 * own steps (step = 0, 1, 2, ... without gaps; ws = c3dgs_weighted_distance_ws_bytes(B, K, D) bytes, 16-byte aligned, kept
 * across the steps):
 *   step_sums(0)   = c3dgs_vq_sums (clears, abs-max + fp16 split of the codebook, search, exact re-scan, accumulation) and arms ws;
 *   step_apply(s)  = c3dgs_vq_apply's update (the same single-rounded operations, bit-identical codebooks) that ALSO leaves what
 *                    step s+1's search needs: the new codebook's fp16 split fragments and scaled ||c||^2 (scaled with the exponent
 *                    of the codebook it read; the new abs-max is gathered for the step after), S cleared, the list counter cleared;
 *   step_sums(s>0) = search + exact re-scan + accumulation only; *dist_sum must be zero on entry (it is added to). The search
 *                    checks the scale it was given against the codebook's true abs-max and sends every point through the exact
 *                    re-scan if the codebook grew 16x or shrank 64x within one update.
 * The min-distance sum (vq.py:71) is folded into the accumulation kernel. Served shapes: D = 48, 12 or 6, K >= 32
 * (c3dgs_vq_step_supported); a sharded run all-reduces S between the two halves exactly as with the unfused pair. */
int c3dgs_vq_step_supported(int32_t K, int32_t D, const float* x, const float* codebook, const void* ws, size_t ws_bytes);
int c3dgs_vq_step_sums(int32_t step, int64_t B, int32_t K, int32_t D, const float* x, const float* w, const int64_t* gather,
                       const float* codebook, float* dist, int64_t* idx, float* S, double* dist_sum, void* ws, size_t ws_bytes,
                       void* stream);
int c3dgs_vq_step_apply(int32_t step, int32_t K, int32_t D, float* S, float* codebook, float* entry_importance, float decay,
                        float alpha, float eps, int32_t scale_normalize, void* ws, size_t ws_bytes, void* stream);

/* apply: entry_importance = decay*entry_importance + alpha*S[:,D];
 *        codebook = decay*codebook + alpha * S[:, :D] / (S[:,D] + eps)        (ema_inplace, vq.py:45-46)
 * then, if scale_normalize (D>=6): codebook /= (cb[:,0]+cb[:,3]+cb[:,5])[:,None]   (vq.py:73-77). */
int c3dgs_vq_apply(int32_t K, int32_t D, const float* S, float* codebook, float* entry_importance,
                   float decay, float alpha, float eps, int32_t scale_normalize, void* stream);

/* ---- batch draws of vq_features: `batch = torch.randint(low=0, high=N, size=[vq_chunk])` on the CPU generator
 * (compression/vq.py:69) ----
 * mt19937_fill (host only, no GPU): continues at::mt19937's stream by n tempered 32-bit outputs. state = the 624 key
 * words, left / next = the generator's counters as torch.get_rng_state() serialises them (left == 1: block exhausted);
 * all three are updated so the caller can write the advanced state back. `out` may be pinned host memory.
 * draws_to_indices: out[i] = (int64) raw[i] % range on the device -- what torch's randint makes of each 32-bit output
 * for range < 2^28 (ATen uniform_int_from_to; larger ranges consume 64 bits per element and are left to torch). */
int c3dgs_mt19937_fill(uint32_t* state, int64_t* left, int64_t* next, uint32_t* out, int64_t n);
int c3dgs_draws_to_indices(int64_t n, int64_t range, const uint32_t* raw, int64_t* out, void* stream);
/* device-side address of a page-locked host buffer, or NULL when it is not mapped for the device: c3dgs_draws_to_indices may then be
 * given that address as `raw` and reads the words over the bus itself (no copy operation in the stream). */
void* c3dgs_host_buffer_device_address(const void* host_ptr);
/* the same fed from (pinned) host memory in one call: copies n raw words to raw_dev on the stream, then converts them. A rank of a
 * sharded run uploads only ITS slice of the batch's draws (raw_host + lo, n = hi - lo). */
int c3dgs_draws_upload(int64_t n, int64_t range, const uint32_t* raw_host, uint32_t* raw_dev, int64_t* out, void* stream);

/* ---- L1 + SSIM loss (reference utils/loss_utils.py:17-63, used at finetune.py:48) ----
 * forward: sums[0..63] add up to sum |img - gt|, sums[64..127] to sum ssim_map (float64, device, zeroed by the callee;
 * 64 partial accumulators each so that the per-workgroup atomics do not serialise on one address); 11x11 Gaussian
 * window sigma 1.5, zero padding, per channel. dmaps (3*C*H*W floats, may be NULL when no backward is needed)
 * receives the three partial-derivative maps the backward consumes.
 * backward: for a scalar  L = l1_coeff * mean|img-gt| + ssim_coeff * mean(ssim_map) + const  (QAT: 1-lambda, -lambda)
 * writes dL_dimg = grad_loss[0] * dL/dimg  ([C,H,W], fully written). */
int c3dgs_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, float* dmaps,
                          double* sums /*[128]*/, void* stream);
/* out[0] (float32, device) = l1_scale * sum(sums[0..63]) + ssim_scale * sum(sums[64..127]) + constant, evaluated in float64:
 * the scalar the reference assembles with torch arithmetic (finetune.py:48; l1_scale = (1 - lambda) / N, ssim_scale = -lambda / N,
 * constant = lambda), in one launch */
int c3dgs_l1_ssim_value(const double* sums /*[128], from c3dgs_l1_ssim_forward*/, double l1_scale, double ssim_scale,
                        double constant, float* out /*device [1]*/, void* stream);
int c3dgs_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, const float* dmaps,
                           const float* grad_loss /*device [1]*/, float l1_coeff, float ssim_coeff, float* dL_dimg,
                           void* stream);

/* ---- image metrics of the evaluation pass (reference compress.py:121-163: psnr of utils/image_utils.py:17-19 and ssim of
 * utils/loss_utils.py:33-63, forward only) ----
 * img, gt: [N, C, H, W] fp32 contiguous (device). out (device, float64) receives N rows of 3:
 *   out[3n] = mean (img - gt)^2,  out[3n+1] = mean ssim_map,  out[3n+2] = mean |img - gt|   (means over C * H * W)
 * out may point into a larger caller table (row v of an evaluation loop at out + 3 * v). ws: device scratch of
 * c3dgs_image_metrics_ws_bytes(N, C, H, W) bytes (8-byte aligned; 0 = sizes not served), owned by the caller and busy until
 * the stream passes the call. Deterministic: no float atomics, so rows are bit-identical from run to run and row n equals
 * the row of image n passed alone. Any H, W >= 1 (zero padding 5 as the reference's conv2d); one call serves at most
 * 2^24 - 1 tiles of 32 x 22 pixels over all planes (about 1860 images of 3 x 1080 x 1920). */
size_t c3dgs_image_metrics_ws_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int c3dgs_image_metrics(int32_t N, int32_t C, int32_t H, int32_t W, const float* img, const float* gt, void* ws, size_t ws_bytes,
                        double* out /*device [N][3]*/, void* stream);

/* ---- Morton ordering (reference GaussianModel._sort_morton, scene/gaussian_model.py:997-1003,
 * mortonEncode :1417-1432).  codes[i] = 63-bit Morton code of xyz[i] (21 bits per axis, axes in ascending-extent order),
 * order = ids sorted stably by code (int64, usable as a torch index). workspace: c3dgs_morton_workspace_bytes(P). */
size_t c3dgs_morton_workspace_bytes(int32_t P);
int c3dgs_morton_order(int32_t P, const float* xyz /*[P,3]*/, int64_t* codes /*[P]*/, int64_t* order /*[P]*/,
                       void* workspace, void* stream);

/* ---- 3-nearest-neighbour scale initialiser (simple_knn's distCUDA2, called by GaussianModel.load_ply for a point cloud
 * without scale_* properties, scene/gaussian_model.py:459).  out[i] = ((d0 + d1) + d2) / 3 where d0 <= d1 <= d2 are the
 * three smallest fp32 squared distances dx*dx + dy*dy + dz*dz (dx = x[j] - x[i], no FMA contraction) over j != i; for
 * P <= 3 the missing slots are FLT_MAX. Exact: the same bits as a brute force. xyz must be finite.
 * workspace: c3dgs_knn_workspace_bytes(P) bytes. P == 0 is a no-op that touches no pointer. */
size_t c3dgs_knn_workspace_bytes(int32_t P);
int c3dgs_knn_mean_dist2(int32_t P, const float* xyz /*[P,3]*/, float* out /*[P]*/, void* workspace, void* stream);
/* The same search with the neighbours' indices (what GaussianModel.densify_initial needs, scene/gaussian_model.py:1366-1367).
 * (d2[i,k], idx[i,k]), k = 0..2, are the three smallest (distance, index) pairs over j != i by index, in ascending
 * lexicographic order: among equal distances the lowest index wins, so the result does not depend on the search order.
 * One exception keeps coincident clouds cheap: a point with three or more other points at distance 0 reports any three of
 * them, in ascending index order, all with d2 = 0. Missing slots (P <= 3): idx = -1, d2 = FLT_MAX. The distances are those
 * c3dgs_knn_mean_dist2 averages. Same workspace, same no-op for P == 0. Added without an ABI version bump. */
int c3dgs_knn_neighbours(int32_t P, const float* xyz /*[P,3]*/, int32_t* idx /*[P,3]*/, float* d2 /*[P,3]*/, void* workspace,
                         void* stream);

/* ---- geometry evaluation: exact nearest neighbour of external queries, surface sampling, and the reduction behind accuracy /
 * completeness / Chamfer / F-score (csrc/nn_query.hip, csrc/mesh_sample.hip, csrc/geometry_metrics.hip; no reference counterpart).
 * Every fp32 expression below is one IEEE operation per operator, in the order written (no contraction), so results are bits.
 * Added without an ABI version bump.
 *
 * NEAREST NEIGHBOUR. c3dgs_nn_build sorts the P reference points and builds the box tree of the 3-NN search ("knn_sort",
 * "knn_bounds") into `index`, c3dgs_nn_index_bytes(P) bytes, 256-byte aligned, content on entry irrelevant. Queries only read
 * the index: it serves any number of c3dgs_nn_query calls until the caller overwrites it. xyz must be finite.
 * c3dgs_nn_query: with d(q, j) = dx*dx + dy*dy + dz*dz, left to right, dx = x[j] - q.x (c3dgs_knn_mean_dist2's expression),
 * (d2[i], idx[i]) is the lexicographically smallest pair (d, j) over all j: among equal distances the lowest index wins, at
 * d == 0 as well. d may be +inf where the subtraction overflows: then every d is +inf and idx = 0. P == 0, or a query with a
 * non-finite coordinate: idx = -1, d2 = FLT_MAX. Q == 0 is a no-op that touches no pointer. Exact: the bits of a brute force.
 * sort_queries != 0: the queries are walked in Morton order ("nn_query_sort": keys and a pair sort in `workspace`) and the results
 * scattered back; 0: in the caller's order. The results are the same. workspace: c3dgs_nn_query_workspace_bytes(Q) bytes,
 * 256-byte aligned, content on entry irrelevant; only the sorted form with P > 0 uses it, otherwise it may be NULL. leaves (optional, [Q]): the number of leaves scanned for each query.
 * Stage names: "nn_query_sort", "nn_query". C3DGS_E_INVALID before any device work: a negative count; for P > 0 a NULL xyz or
 * index; for Q > 0 a NULL queries, idx or d2, and where it is used a NULL workspace; a misaligned index or workspace.
 *
 * SURFACE SAMPLING at `density` points per unit area. mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
 * x ^= x >> 16 (uint32); base(f) = mix(mix(f) ^ seed); u24(x) = float(x >> 8) * 2^-24. Face f with corners a, b, c:
 *   u = b - a, v = c - a;  cx = u.y v.z - u.z v.y, cy = u.z v.x - u.x v.z, cz = u.x v.y - u.y v.x;
 *   area = 0.5 sqrt_rn((cx cx + cy cy) + cz cz);  t = area * density;  n_f = int(floor(t)) + (u24(base(f)) < t - floor(t) ? 1 : 0);
 *   a non-finite t gives n_f = 0;
 *   sample k < n_f: u1 = u24(mix(base(f) + 2k + 1)), u2 = u24(mix(base(f) + 2k + 2)); if u1 + u2 > 1: u1 = 1 - u1, u2 = 1 - u2;
 *   p = (a + u1 (b - a)) + u2 (c - a) per component.
 * c3dgs_mesh_sample_count: a 16-byte clear, two launches ("mesh_sample_count", "mesh_sample_scan") and ONE host read of the total and a flag
 * word; the call synchronises the stream. *total = the sum of n_f. C3DGS_E_INVALID with a message after the read: a vertex index
 * outside [0, V) (never dereferenced), a face with a finite t >= 2^24, a total above 2^31 - 1.
 * c3dgs_mesh_sample_emit ("mesh_sample_emit", one lane per sample): points [S,3] and face [S] for the S the count returned, from
 * the SAME workspace, untouched in between, and the same mesh, density and seed; ordered by face, then by k. It never stores past
 * S. workspace: c3dgs_mesh_sample_workspace_bytes(F) bytes, 256-byte aligned, content on entry irrelevant. F == 0: *total = 0,
 * nothing is launched; S == 0 launches nothing. C3DGS_E_INVALID before any device work: V or F < 0 (workspace_bytes: 0); S < 0 or
 * above 2^31 - 1; a density that is not finite and positive; for F > 0 a NULL vertices, faces or total, a NULL, small or misaligned
 * workspace; for S > 0 NULL points or face, or F == 0.
 *
 * REDUCTION of one direction's distances. Per element: d = sqrt_rn(d2) in fp32; counted iff d2 != FLT_MAX, d <= max_dist and,
 * with `points` [N,3] and `bounds` (host, {lo x y z, hi x y z}; both or neither), lo <= p <= hi on every axis; below threshold t
 * iff counted and d < thresholds[t] (host [T], T <= C3DGS_GEOMETRY_MAX_THRESHOLDS). out (device, 2 + T doubles): the count, the
 * fp64 sum of d, the T counts. Two launches ("geometry_reduce"), per-workgroup fp64 partials added in index order: bitwise
 * reproducible, no floating-point atomics. N == 0 gives zeros. workspace: c3dgs_geometry_reduce_workspace_bytes(N) bytes, 8-byte
 * aligned, content on entry irrelevant. C3DGS_E_INVALID before any device work: N < 0; T outside [0, 8]; thresholds NULL with
 * T > 0; NULL out; for N > 0 NULL d2, or points without bounds or the reverse; a NULL, small or misaligned workspace. */
#define C3DGS_GEOMETRY_MAX_THRESHOLDS 8
size_t c3dgs_nn_index_bytes(int32_t P);
int c3dgs_nn_build(int32_t P, const float* xyz /*[P,3]*/, void* index, void* stream);
size_t c3dgs_nn_query_workspace_bytes(int32_t Q);
int c3dgs_nn_query(int32_t P, const void* index, int32_t Q, const float* queries /*[Q,3]*/, int32_t sort_queries,
                   int32_t* idx /*[Q]*/, float* d2 /*[Q]*/, uint32_t* leaves /*[Q] | NULL*/, void* workspace, void* stream);
size_t c3dgs_mesh_sample_workspace_bytes(int32_t F);
int c3dgs_mesh_sample_count(int32_t V, const float* vertices /*[V,3]*/, int32_t F, const int32_t* faces /*[F,3]*/, float density,
                            uint32_t seed, void* workspace, size_t workspace_bytes, uint64_t* total /*host*/, void* stream);
int c3dgs_mesh_sample_emit(int32_t V, const float* vertices /*[V,3]*/, int32_t F, const int32_t* faces /*[F,3]*/, uint32_t seed,
                           const void* workspace, size_t workspace_bytes, int64_t S, float* points /*[S,3]*/,
                           int32_t* face /*[S]*/, void* stream);
size_t c3dgs_geometry_reduce_workspace_bytes(int64_t N);
int c3dgs_geometry_reduce(int64_t N, const float* d2 /*[N]*/, const float* points /*[N,3] | NULL*/,
                          const float* bounds /*host [6] | NULL*/, float max_dist, int32_t T, const float* thresholds /*host [T]*/,
                          void* workspace, size_t workspace_bytes, double* out /*device [2 + T]*/, void* stream);

/* ---- fused Adam step (the optimizer.step() that closes the QAT inner loop, finetune.py:65-66; optimizer set-up
 * scene/gaussian_model.py:296-308: torch.optim.Adam(param groups, lr=0.0, eps=1e-15), no weight decay, no amsgrad).
 * ONE launch updates up to C3DGS_ADAM_MAX_TENSORS tensors with torch's _single_tensor_adam arithmetic; the caller passes
 * per tensor step_size = lr / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t) (computed in double, as torch does). */
#define C3DGS_ADAM_MAX_TENSORS 16
typedef struct c3dgs_adam_tensor {
    float* param;            /* [n] updated in place */
    const float* grad;       /* [n]                  */
    float* exp_avg;          /* [n] first moment     */
    float* exp_avg_sq;       /* [n] second moment    */
    int64_t n;
    float step_size;
    float bias_correction2_sqrt;
} c3dgs_adam_tensor;
int c3dgs_adam_step(int32_t n_tensors, const c3dgs_adam_tensor* tensors /*host*/, double beta1, double beta2, double eps, void* stream);

/* ---- sparse Adam: the same step over the rows (Gaussians) a per-row mask lists, every other row untouched: neither loaded
 * nor stored, in any of the four arrays (upstream 3DGS's optimizer_type="sparse_adam": rows with radii > 0). Beyond the
 * reference, which has no sparse optimizer. Added without an ABI version bump: new entry points only.
 *   select: the ascending list of the listed rows and its length, built on the device (block counts -> scan -> emit; stable,
 *           no atomics, no host read). mask_kind 0: uint8, listed when != 0; 1: int32, listed when > 0 (radii as they are).
 *   step:   ONE launch per call; lane i of a tensor handles element i % row_len of row rows[i / row_len]. The launch is
 *           sized from P, the kernel reads the count from the workspace. Any row_len > 0; rows need 4-byte alignment only.
 * The workspace is the caller's, 256-byte aligned, c3dgs_sparse_adam_workspace_bytes(P) bytes: count u32 at offset 0, rows
 * u32[P] at offset 256, the select's block totals behind them. 0 <= P < 2^31. P == 0, n_tensors == 0 and a mask that lists
 * nothing are no-ops; arguments are validated before any device work. */
int c3dgs_sparse_adam_workspace_bytes(int64_t P, size_t* bytes);
int c3dgs_sparse_adam_select(int64_t P, const void* mask /*[P]*/, int32_t mask_kind /* 0: u8 != 0, 1: i32 > 0 */, void* workspace,
                             void* stream);
typedef struct c3dgs_sparse_adam_tensor {
    float* param;            /* [P, row_len] listed rows updated in place */
    const float* grad;       /* [P, row_len]                              */
    float* exp_avg;          /* [P, row_len] first moment                 */
    float* exp_avg_sq;       /* [P, row_len] second moment                */
    int64_t n;               /* P * row_len */
    float step_size;
    float bias_correction2_sqrt;
    int32_t row_len;         /* elements per row */
} c3dgs_sparse_adam_tensor;
int c3dgs_sparse_adam_step(int32_t n_tensors, const c3dgs_sparse_adam_tensor* tensors /*host*/, int64_t P, const void* workspace,
                           double beta1, double beta2, double eps, void* stream);

/* ---- adaptive density control (scene/gaussian_model.py:1187-1403: densify_and_clone / densify_and_split / prune_points /
 * densify_and_prune / add_densification_stats), non-indexed models. The reference rebuilds the scene in four passes (clone
 * cat, split cat, the split's prune, the final prune); here: classify (one code byte per row) -> plan (one scan, the source
 * map of the new scene in the reference's row order, four totals) -> apply (ONE launch writes every row of every parameter
 * tensor and both Adam moments once). Added without an ABI version bump: new entry points only.
 *
 * code bits */
#define C3DGS_ROW_KEEP 1u        /* the original row survives                                              */
#define C3DGS_ROW_CLONE 2u       /* its clone survives                                                     */
#define C3DGS_ROW_SPLIT 4u       /* selected as a split parent (counts towards S whether or not its children survive) */
#define C3DGS_ROW_CHILD_KEPT 8u  /* its N children survive (implies C3DGS_ROW_SPLIT)                        */
/* row kinds of the plan: 0 original, 1 clone, 2 + k child copy k */
#define C3DGS_KIND_ORIGINAL 0
#define C3DGS_KIND_CLONE 1
#define C3DGS_KIND_CHILD 2
/* classify: one thread per row, on the ACTIVATED quantities the reference's masks are made of (the caller runs the getters
 * in the reference's order, see DESIGN.md "Density control"):
 *   g = accum / denom, NaN -> 0 (0/0; x/0 = inf stays and selects)                                   :1337-1338
 *   clone  = sqrt(g*g) >= max_grad && max(scale_clone) <= dense_extent                               :1282-1284
 *   split  = g >= max_grad && max(scale_split) > dense_extent                                        :1232-1236
 *   pruned = opacity < min_opacity || max(scale_prune_*) > big_extent   (second term only when both scale_prune_self and
 *            scale_prune_child are given: _self for the original and its clone, _child for the N children)   :1344-1349
 *   code   = (!split && !pruned_self) | (clone && !pruned_self) << 1 | split << 2 | (split && !pruned_child) << 3
 * The reference's max_radii2D test is dead inside densify_and_prune (the postfix has zeroed it) and is not mirrored.
 * max_grad must be > 0: with max_grad <= 0 the reference's zero-padded gradients would make every clone a split parent
 * too, a corner the training loop never reaches; it is rejected with C3DGS_E_INVALID. Thresholds are the Python doubles
 * rounded to float, as torch's tensor-vs-scalar comparison rounds them. */
int c3dgs_densify_classify(int32_t P, const float* accum /*[P]*/, const float* denom /*[P]*/, const float* scale_clone /*[P,3]*/,
                           const float* scale_split /*[P,3]*/, const float* scale_prune_self /*[P,3] or NULL*/,
                           const float* scale_prune_child /*[P,3] or NULL*/, const float* opacity /*[P]*/, float max_grad,
                           float dense_extent, float min_opacity, float big_extent, uint8_t* code /*[P]*/, void* stream);
/* plan: exclusive scans of the four per-row counts and the source map in the reference's row order: surviving originals
 * in source order, surviving clones in source order, then child copy 0 of every parent whose children survive in source
 * order, copy 1, ... copy N-1. totals (device int32[4]) = {kept, clones, S, parents whose children survive}; the new
 * scene has P_new = kept + clones + N * totals[3] rows. With src == NULL only the totals are computed (the caller reads
 * them, allocates and calls again); otherwise rows j < capacity of src (source row), kind and draw_row (for a child:
 * k * S + rank of its parent among ALL S selected parents = the row of the [N*S,3] draws it consumes; -1 otherwise) are
 * written and rows beyond capacity are not touched. workspace >= c3dgs_rows_plan_workspace_bytes(P). */
size_t c3dgs_rows_plan_workspace_bytes(int32_t P);
int c3dgs_rows_plan(int32_t P, const uint8_t* code /*[P]*/, int32_t N, int64_t capacity, int32_t* src, uint8_t* kind,
                    int32_t* draw_row, int32_t* totals /*device [4]*/, void* workspace, void* stream);
/* apply: out[j] = in[src[j]] for every tensor of the table; moments copied for kind == original and zero otherwise
 * (cat_tensors_to_optimizer, :1169-1172); NULL moment pointers = no optimizer state. role 1 (xyz) and 2 (scaling) rewrite
 * child rows: xyz = R(rotation_raw[src]) (z[draw_row] * std[src]) + get_xyz[src] with R = build_rotation of the raw quaternion
 * (utils/general_utils.py:84-107) and get_xyz the parent position, rounded through fp16 when half_xyz (the reference adds
 * get_xyz, which is xyz_qa(_xyz), :1245), and scaling = std[src] / (0.8 N), or its log when log_scaling (:1247). */
#define C3DGS_ROWS_MAX_TENSORS 16
enum { C3DGS_ROLE_COPY = 0, C3DGS_ROLE_XYZ = 1, C3DGS_ROLE_SCALING = 2 };
typedef struct c3dgs_rows_tensor {
    const float* in_param;
    const float* in_exp_avg;     /* NULL together with the other three moment pointers */
    const float* in_exp_avg_sq;
    float* out_param;
    float* out_exp_avg;
    float* out_exp_avg_sq;
    int32_t row_floats;          /* 1 .. 4096 */
    int32_t role;
} c3dgs_rows_tensor;
int c3dgs_rows_apply(int32_t P, int64_t P_new, const int32_t* src /*[P_new]*/, const uint8_t* kind /*[P_new]*/,
                     const int32_t* draw_row /*[P_new]*/, int32_t n_tensors, const c3dgs_rows_tensor* tensors /*host*/,
                     int32_t N, int64_t n_draws, const float* rotation_raw /*[P,4]*/, const float* std /*[P,3]*/,
                     const float* z /*[n_draws,3]*/, int32_t log_scaling, int32_t half_xyz, void* stream);
/* stats: the per-iteration bookkeeping (train.py:101-106, :1399-1402) in one launch, no allocation, no synchronisation:
 * for rows with filter: accum += sqrt(gx*gx + gy*gy) of grad[p, 0:2] (row stride 3), denom += 1 and, with radii,
 * max_radii = max(max_radii, radii). */
int c3dgs_densify_stats(int32_t P, const float* grad /*[P,3]*/, const uint8_t* filter /*[P]*/, const int32_t* radii /*[P] or NULL*/,
                        float* accum /*[P]*/, float* denom /*[P]*/, float* max_radii /*[P] or NULL*/, void* stream);

/* ---- MCMC density control ("3D Gaussian Splatting as Markov Chain Monte Carlo", gsplat's MCMCStrategy), non-indexed models.
 * Beyond the reference, which has threshold-driven density control only. Added without an ABI version bump: new entry points
 * only. csrc/mcmc.hip. 0 <= P < 2^31; P == 0 and n == 0 are no-ops; arguments are validated before any device work.
 *
 * sample: n draws over P rows by opacity. o_i = sigmoid(raw_opacity_i) in fp32 and the INTEGER weight q_i = floor(o_i 2^20),
 *   q_i = 0 for an excluded row: the rows `dead` marks (non-zero), or, with dead == NULL and derive_dead != 0, the rows with
 *   o_i <= min_opacity, whose mask is then written to dead_out; with dead == NULL and derive_dead == 0 every row takes part.
 *   With C_i the inclusive 64-bit prefix of q and T its total, draw j (a float64 uniform in [0, 1)) has the target
 *   t_j = min(T - 1, (uint64) floor(draws[j] * (double) T)), one IEEE multiply, and sources[j] is the smallest i with
 *   C_i > t_j: a row of weight 0 is never chosen. counts[i] = the number of draws that chose i (integer atomics). The
 *   prefix is exact and independent of the scan order, so q, sources and counts are bitwise reproducible.
 *   Outputs: q u32[P], counts i32[P] (zeroed first), *T u64 (device), sources i32[n]. With T == 0 nothing has weight: every
 *   source is -1, counts stay 0 and *T == 0 reports it.
 *   reuse_weights != 0: the workspace still holds the weights and prefix of a previous call with the same P and opacities
 *   (q, *T and dead_out are not written again); counts are zeroed and the n draws are taken. A call with n == 0 and
 *   reuse_weights == 0 computes the weights alone, so that the caller can size n from the mask it derived.
 * apply: n pairs (dst_j, src_j = sources[j]), in place, P unchanged. dst_j = dst[j], or dst_base + j with dst == NULL. For
 *   a row with count > 0 and N = min(count + 1, 51):
 *     o' = 1 - (1 - o)^(1/N), clamped to [min_opacity, 1 - FLT_EPSILON]
 *     c  = o / sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)
 *   evaluated in double from the raw fp32 opacity (o itself included: near o = 1 the fp32 sigmoid has lost 1 - o; in fp32
 *   the sums are off by 1e-4 relative) and written in raw space, each value rounded once: the C3DGS_MCMC_ROLE_OPACITY tensor (row_floats 1) takes
 *   logit(o'), every float of the C3DGS_MCMC_ROLE_SCALE tensor's row (row_floats 1..3: the raw log scale, or the raw log
 *   scale factor) takes += log c. Each source gets its own values; each destination gets its source's, and with copy_rows != 0
 *   also its source's row of every C3DGS_ROLE_COPY tensor (copy_rows == 0: the caller has copied the rows already). exp_avg
 *   and exp_avg_sq of every source and destination row become zero in every tensor that has moments. All values are those
 *   from before the call: the relocation values are staged in the workspace first, the row launch reads nothing it writes.
 *   Sources and destinations must be disjoint (a destination's count is 0), which holds for dead rows (weight 0) and for
 *   appended rows. The table is c3dgs_rows_apply's: in place, so in_* == out_*; exactly one opacity and one scale tensor.
 *   Pairs with a source or destination outside [0, P) are skipped.
 * noise: xyz += Sigma xi g(o) noise_lr xyz_lr, per row, in place, with Sigma = R diag(s^2) R^T formed as R (s^2 * (R^T xi)),
 *   R of the normalised raw quaternion (r, x, y, z), s = exp(scaling), or normalize(relu(scaling)) * exp(scaling_factor) when
 *   scaling_factor is given, o = sigmoid(raw_opacity), g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))), xi [P,3] unit normals.
 * The workspace is the caller's, 256-byte aligned, c3dgs_mcmc_workspace_bytes(P) bytes, shared by sample and apply. */
#define C3DGS_MCMC_ROLE_OPACITY 3
#define C3DGS_MCMC_ROLE_SCALE 4
int c3dgs_mcmc_workspace_bytes(int64_t P, size_t* bytes);
int c3dgs_mcmc_sample(int64_t P, const float* raw_opacity /*[P]*/, const uint8_t* dead /*[P] or NULL*/, int32_t derive_dead,
                      float min_opacity, uint8_t* dead_out /*[P], with derive_dead*/, int64_t n, const double* draws /*[n]*/,
                      int32_t reuse_weights, uint32_t* q /*[P]*/, int32_t* sources /*[n]*/, int32_t* counts /*[P]*/,
                      uint64_t* T /*device*/, void* workspace, void* stream);
int c3dgs_mcmc_apply(int64_t P, int64_t n, const int32_t* dst /*[n] or NULL*/, int64_t dst_base, const int32_t* sources /*[n]*/,
                     const int32_t* counts /*[P]*/, int32_t n_tensors, const c3dgs_rows_tensor* tensors /*host*/,
                     int32_t copy_rows, float min_opacity, void* workspace, void* stream);
int c3dgs_mcmc_noise(int64_t P, float* xyz /*[P,3]*/, const float* rotation /*[P,4]*/, const float* scaling /*[P,3]*/,
                     const float* scaling_factor /*[P] or NULL*/, const float* raw_opacity /*[P]*/, const float* xi /*[P,3]*/,
                     float noise_lr, float xyz_lr, void* stream);

/* ---- per-image colour correction by a bilateral grid (csrc/bilagrid.hip; no reference counterpart: gsplat's lib_bilagrid /
 * fused_bilagrid; a grid of shape (1, 1, 1) is upstream 3DGS's per-image 3x4 `exposure`) ----
 * Added without an ABI version bump: new entry points only. One camera's grid G is fp32 [12, L, Hg, Wg], the 12 rows a row-major
 * 3x4 matrix per lattice vertex; rgb, out, dL_dout, dL_drgb are planar fp32 [3, H, W]. For pixel (x, y) with colour c = (r, g, b):
 *   gx = (x + 0.5) / W (Wg - 1),  gy = (y + 0.5) / H (Hg - 1),  z = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
 *   A = the trilinear interpolation of the 12 rows at (z, gy, gx), hat weights max(0, 1 - |coordinate - index|) per axis, an
 *       axis of size 1 weighing 1;   out = A[:, :3] c + A[:, 3]
 * which is grid_sample(G[None], (2 xs - 1, 2 ys - 1, 2 luma - 1), "bilinear", "border", align_corners=True) followed by the affine.
 * An identity grid of shape (1, 1, 1) returns rgb bit for bit. A NaN luma reads level 0.
 * slice_backward: dL_dgrid (every element written; a vertex no pixel touches receives exactly 0) and, unless dL_drgb is NULL,
 *   dL_drgb = A[:, :3]^T dL_dout + (dL/dz)(L - 1)(0.299, 0.587, 0.114), the second term zero where the luma was clamped and for
 *   L == 1. dL_dgrid is gathered by vertex into `workspace` (c3dgs_bilagrid_workspace_bytes(H, W, L, Hg, Wg) bytes, never 0,
 *   8-byte aligned, every word read is written first) and folded in a fixed order: no float atomics, bitwise
 *   reproducible, and the same bits with and without dL_drgb.
 * tv: out[0] = (1 / C) sum over the lattice axes of size >= 2 of sum((X[i + 1] - X[i])^2 along the axis) / (12 x the lattice
 *   positions of one camera's differences along it), for X = grids [C, 12, L, Hg, Wg]; summed in double in a fixed order.
 *   `workspace`: the same query with H = W = 1 (8 KiB suffice). tv_backward: dL_dgrids = dL_dtv[0] x d tv / dX, every element
 *   written, each from its up to six neighbours; dL_dtv is one fp32 on the device.
 * Every entry returns C3DGS_E_INVALID with a message before any device work for a non-positive size, 12 L Hg Wg (for tv also
 * C 12 L Hg Wg) or 3 H W not below 2^31, a NULL required pointer or workspace, and a gather launch that does not fit
 * (Hg Wg x slabs >= 2^31 or L > 524280); c3dgs_bilagrid_workspace_bytes returns 0 then and leaves the message in
 * c3dgs_last_error. Stage names: "bilagrid_slice"; "bilagrid_slice_backward" (all of its launches; "bilagrid_gather",
 * "bilagrid_fold", "bilagrid_rgb_backward" alone); "bilagrid_tv" (both launches); "bilagrid_tv_backward". */
size_t c3dgs_bilagrid_workspace_bytes(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg);
int c3dgs_bilagrid_slice(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg, const float* grid, const float* rgb,
                         float* out, void* stream);
int c3dgs_bilagrid_slice_backward(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg, const float* grid, const float* rgb,
                                  const float* dL_dout, float* dL_dgrid /*written*/, float* dL_drgb /*| NULL*/, void* workspace,
                                  void* stream);
int c3dgs_bilagrid_tv(int32_t C, int32_t L, int32_t Hg, int32_t Wg, const float* grids, void* workspace, float* out /*[1]*/,
                      void* stream);
int c3dgs_bilagrid_tv_backward(int32_t C, int32_t L, int32_t Hg, int32_t Wg, const float* grids, const float* dL_dtv /*[1], device*/,
                               float* dL_dgrids /*written*/, void* stream);

/* ---- initial densification (GaussianModel.densify_initial, scene/gaussian_model.py:1352-1389): new points one `step` apart
 * on the ray from every point to each of its three nearest neighbours, planned in one pass from the neighbour table of
 * c3dgs_knn_neighbours instead of the reference's loop over levels (DESIGN.md "Initial densification"). With
 *   rel[i,nb] = fl(fl(sqrt(d2[i,nb])) / step)      and r2[nb] the second-largest rel of slot nb, counted with multiplicity,
 * point i receives c = max(0, floor(min(rel, r2)) - 1) rows for slot nb, at levels 1..c (the min with r2 is the reference's
 * `slot.sum() > 1`: levels only the single farthest point reaches insert nothing). Added without an ABI version bump.
 *
 * plan: the source map of the NEW rows in the reference's order: slot-major (nb = 0, 1, 2), then level ascending, then
 * source index ascending. totals (device int32[4]) = {rows of slot 0, slot 1, slot 2, overflow}. Per-point counts saturate
 * at INT32_MAX, sums are formed in 64 bits, and overflow = 1 when P + new rows > INT32_MAX - 255; then the slot totals are
 * clamped and nothing else is written. Two-call protocol, like c3dgs_rows_plan: with src == NULL only the totals are
 * computed (workspace >= c3dgs_ray_fill_plan_workspace_bytes(P, 0)); the caller reads them, allocates and calls again with
 * workspace >= c3dgs_ray_fill_plan_workspace_bytes(P, rows of all three slots). The second call recomputes everything from
 * its inputs, reads the totals back itself (one small synchronising read: they size its launches and the key bits of the
 * level sort), writes rows j < capacity of src, slot (0..2) and level (1..c) and touches nothing beyond. P == 0: totals = 0.
 * P or capacity < 0, P > INT32_MAX - 255, a step that is not a positive finite number, NULL d2, totals or workspace, src
 * without slot and level, and a workspace too small for the rows return C3DGS_E_INVALID; all but the last before any launch. */
size_t c3dgs_ray_fill_plan_workspace_bytes(int32_t P, int64_t rows);
int c3dgs_ray_fill_plan(int32_t P, const float* d2 /*[P,3]*/, float step, int64_t capacity, int32_t* src, uint8_t* slot,
                        int32_t* level, int32_t* totals /*device [4]*/, void* workspace, size_t workspace_bytes, void* stream);
/* positions: out[r] = xyz[i] * (1 - a) + a * xyz[idx[i,nb]], a = fl(float(level[r]) / rel[i,nb]), i = src[r], nb = slot[r];
 * one subtraction, two multiplications and one addition, each rounded to fp32 on its own (:1379, :1385). `out` is the
 * [n_new,3] block behind the P originals of the new xyz tensor. A row whose src, slot or neighbour is out of range gets
 * zeros and reads nothing. */
int c3dgs_ray_fill_xyz(int32_t P, const float* xyz /*[P,3]*/, const int32_t* idx /*[P,3]*/, const float* d2 /*[P,3]*/, float step,
                       int64_t n_new, const int32_t* src, const uint8_t* slot, const int32_t* level, float* out /*[n_new,3]*/,
                       void* stream);

/* ---- ground-truth image of a camera (scene/cameras.py:67-92, Camera.original_image): decoded 8-bit texels -> the planar fp32
 * image the loss reads, at the camera's resolution, in one launch. Added without an ABI version bump: a new entry point only.
 * Every step is ONE separately rounded fp32 operation unless fp64 is stated:
 *   texel    v = fl(float(u) / 255), correctly rounded
 *   alpha    C == 4: a = fl(float(u_a) / 255), v = v * a;  with bg != NULL: v = v * a + bg[c] * (1 - a)
 *   flip     flip != 0: texel (y, x) is read from (Hs-1-y, Ws-1-x), an index remap in front of the resize
 *   resize   OpenCV's documented INTER_LINEAR (half-pixel centres, edge clamp, no antialiasing). Per axis, in fp64:
 *            scale = 1.0 / ((double)dst / (double)src), f = (float)((d + 0.5) * scale - 0.5); then s = floor(f), f -= s;
 *            s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0; second tap at min(s + 1, src - 1).
 *            h = t0 * (1 - fx) + t1 * fx on both rows, then o = h0 * (1 - fy) + h1 * fy. Equal sizes give the texel value.
 *   output   out[c][y][x] = min(max(o, 0), 1)
 * Nothing outside `out` is written; `src` is read through the aligned dwords that hold its bytes and nothing beyond them.
 * No atomics: bit-identical from run to run. A NULL src or out, C not in {3, 4}, bg with C == 3 and a dimension outside
 * [1, 32768] return C3DGS_E_INVALID before any launch. The image path is our own contract (tests/image_ref.py): cv2.resize
 * itself is not pinned. */
int c3dgs_image_from_u8(int32_t Hs, int32_t Ws, int32_t C /*3|4*/, const uint8_t* src /*device [Hs][Ws][C]*/, int32_t flip,
                        const float* bg /*device [3] or NULL*/, int32_t Hd, int32_t Wd, float* out /*device [3][Hd][Wd]*/,
                        void* stream);

/* ---- prune / codebook compaction of an INDEXED model (scene/gaussian_model.py:1101-1158, the index remapping the entry points
 * above do not mirror). A model keeps up to two index spaces: space 0 = colour (idx0 = _feature_indices into the K0 rows of
 * _features_dc / _features_rest), space 1 = geometry (idx1 = _gaussian_indices into the K1 rows of _scaling / _rotation).
 * The plan removes the Gaussians with keep[i] == 0 (keep == NULL: all survive), drops every codebook row no survivor
 * references and renumbers the indices; c3dgs_rows_apply then moves the rows (kind all C3DGS_KIND_ORIGINAL, role copy: one
 * launch per row space, by src, cb_src0 and cb_src1). Added without an ABI version bump: new entry points only.
 *
 * Order contract:
 *   src[j]       source row of surviving Gaussian j, in source order                              j < P_new
 *   cb_srcX[r]   old id of surviving codebook row r: the referenced old ids in ASCENDING order     r < KX_new
 *   new_idxX[j]  rank of idxX[src[j]] among the referenced ids, so  cb_srcX[new_idxX[j]] == idxX[src[j]]
 * which is the reference's result (sorted unique ids, index_map[u] = position of u, :1110-1114) without its Python loop
 * over the ids. An index space whose idx is NULL is skipped: its total is 0 and its outputs are not touched.
 *
 * totals (device int32[4]) = {P_new, K0_new, K1_new, out_of_range}. Two-call protocol, like c3dgs_rows_plan: with
 * src == NULL only the totals are computed (the caller reads them once, allocates and calls again; the second call
 * recomputes flags, scans and totals from the inputs, nothing is carried over in the workspace); otherwise src, and
 * new_idxX and cb_srcX of every index space given, are required, rows j < cap_rows of src / new_idx0 / new_idx1,
 * r < cap_cb0 of cb_src0 and r < cap_cb1 of cb_src1 are written and nothing beyond the capacities is touched.
 *
 * Bad indices: an index outside [0, KX) is never dereferenced. Every one of them is counted in totals[3], over ALL P rows of
 * every index space given (the reference asserts index.max() < n_feats on the whole array, :1106), it references no row,
 * and where its Gaussian survives new_idxX[j] = -1. The caller is expected to treat totals[3] != 0 as an error.
 *
 * Limits: row counts are int32 and at most INT32_MAX - 255, indices int64. P = 0 (totals = 0, nothing else touched), KX = 0 with idxX NULL, and
 * P_new = 0 are valid. P, K0, K1 or a capacity < 0, P, K0 or K1 > INT32_MAX - 255, idxX given with KX <= 0, a NULL totals or workspace, and src given
 * without the outputs of a given index space return C3DGS_E_INVALID before any launch.
 * workspace >= c3dgs_index_plan_workspace_bytes(P, K0, K1); the library clears the flags it keeps there itself. */
size_t c3dgs_index_plan_workspace_bytes(int32_t P, int32_t K0, int32_t K1);
int c3dgs_index_plan(int32_t P, const uint8_t* keep /*[P] or NULL*/, const int64_t* idx0 /*[P] or NULL*/, int32_t K0,
                     const int64_t* idx1 /*[P] or NULL*/, int32_t K1, int64_t cap_rows, int64_t cap_cb0, int64_t cap_cb1,
                     int32_t* src /*[P_new]*/, int64_t* new_idx0 /*[P_new]*/, int64_t* new_idx1 /*[P_new]*/,
                     int32_t* cb_src0 /*[K0_new]*/, int32_t* cb_src1 /*[K1_new]*/, int32_t* totals /*device [4]*/,
                     void* workspace, void* stream);

/* ---- sensitivity pass (compress.py:110-113): acc[i] += |g[i]| for n floats, one launch */
int c3dgs_abs_accumulate(int64_t n, const float* g, float* acc, void* stream);

/* ---- extract_rot_scale(to_full_cov(cov)) (utils/splats.py:7-35; compress_covariance, compression/vq.py:186):
 * cov6[n,6] = upper triangle (xx,xy,xz,yy,yz,zz) -> rot[n,4] unit quaternion (r,x,y,z) of the eigenvector frame with
 * determinant +1, scale[n,3] = sqrt of the ascending eigenvalues of cov + 1e-8 I (NaN -> 1e-6). */
int c3dgs_extract_rot_scale(int32_t n, const float* cov6, float* rot, float* scale, void* stream);

/* ---- QAT getters: activation + fake-quant + visibility gathers in front of every raster call -------------------
 * SURVEY.md 8(f) row N1; reference scene/gaussian_model.py:54-77 (activations), :109-118 (seven
 * torch.ao.quantization.FakeQuantize(dtype=qint8) modules = MovingAverageMinMaxObserver, per-tensor affine,
 * [-128,127], averaging constant 0.01), :213-267 (getters), :851-862 (the [visible] gathers of GaussianModel.render),
 * :1405-1414 (FakeQuantizationHalf). The reference spends ~100 small launches and ~20 host syncs per view here
 * (aminmax + `float(scale)` / `int(zero_point)` per module, nonzero per boolean-mask gather); this path keeps the
 * observer state on the device and never reads it back.
 *
 * Observer/quantiser state of ONE FakeQuantize module, resident in device memory (16 bytes): */
typedef struct c3dgs_fq_state {
    float min_val, max_val;   /* MovingAverageMinMaxObserver running range; +inf / -inf before the first batch */
    float scale;              /* max((max(max_val,0) - min(min_val,0)) / 255, eps_f32)                          */
    int32_t zero_point;       /* clamp(-128 - round(min(min_val,0)/scale), -128, 127)                           */
} c3dgs_fq_state;

enum { C3DGS_FQ_OPACITY = 0, C3DGS_FQ_SCALING = 1, C3DGS_FQ_SCALING_FACTOR = 2, C3DGS_FQ_ROTATION = 3,
       C3DGS_FQ_FEATURES_DC = 4, C3DGS_FQ_FEATURES_REST = 5, C3DGS_FQ_COUNT = 6 };

typedef struct c3dgs_qat_params {
    int32_t P, GS, SHS, M;          /* points, geometry codebook rows, colour codebook rows, SH coefficients (M >= 1) */
    const float* xyz;               /* [P,3]   raw _xyz                                            */
    const float* opacity;           /* [P,1]   raw _opacity (pre-sigmoid)                          */
    const float* scaling_factor;    /* [P,1]   raw _scaling_factor (log)                           */
    const float* scaling;           /* [GS,3]  raw _scaling                                        */
    const float* rotation;          /* [GS,4]  raw _rotation                                       */
    const float* features_dc;       /* [SHS,1,3]                                                   */
    const float* features_rest;     /* [SHS,M-1,3] (may be NULL when M == 1)                       */
    c3dgs_fq_state* state;          /* device, [C3DGS_FQ_COUNT]                                    */
    int32_t observer_enabled[6];    /* torch FakeQuantize.observer_enabled per module              */
    int32_t fake_quant_enabled[6];  /* torch FakeQuantize.fake_quant_enabled per module            */
    int32_t half_xyz;               /* 1: xyz_qa = x.half().float() (:1405-1414); 0: identity      */
    float averaging_constant;       /* 0.01                                                        */
} c3dgs_qat_params;

/* Any input pointer may be NULL: that tensor is skipped in every call below.
 * observe: one pass over the raw tensors -> min/max of the ACTIVATED values (sigmoid(opacity), normalize(relu(scaling)),
 *   the rest raw), moving-average update and qparams of every module whose observer is enabled (FakeQuantize.forward,
 *   first half). `workspace` >= c3dgs_qat_workspace_bytes() bytes of device scratch.
 * codebooks: scales_n[GS,3] = fq(normalize(relu(scaling))); rotations[GS,4] = normalize(fq(rotation));
 *   shs[SHS,M,3] = cat(fq_dc(features_dc), fq_rest(features_rest), dim=1)   (get_scaling_normalized,
 *   _rotation_post_activation, _get_features_raw).
 * visible: visible[p] = in_frustum(xyz_qa(xyz[p])) (rasterizer markVisible on get_xyz), rank = exclusive scan of it
 *   (the row of p in every `[visible]`-gathered tensor), *count (device int32) = number visible. visible == NULL input to
 *   points/points_backward means "all rows, rank = identity" (plain getters).
 * points: rows j = rank[p] of means3D = xyz_qa(xyz), opacities = fq(sigmoid(opacity)), scale_factors =
 *   exp(fq(scaling_factor)), sh_indices / g_indices copies (the five boolean-mask gathers of render()).
 * *_backward: straight-through fake-quant masks x activation derivatives, recomputed from the raw tensors and the
 *   state snapshot `state` (the caller passes a copy taken at forward time); P-sized outputs are fully written
 *   (zeros for invisible rows). */
size_t c3dgs_qat_workspace_bytes(void);
int c3dgs_qat_observe(const c3dgs_qat_params* q, void* workspace, void* stream);
int c3dgs_qat_codebooks(const c3dgs_qat_params* q, float* scales_n, float* rotations, float* shs, void* stream);
int c3dgs_qat_codebooks_backward(const c3dgs_qat_params* q, const float* dL_dscales_n, const float* dL_drotations,
                                 const float* dL_dshs, float* dL_dscaling, float* dL_drotation, float* dL_dfeatures_dc,
                                 float* dL_dfeatures_rest, void* stream);
size_t c3dgs_qat_scan_bytes(int32_t P);
int c3dgs_qat_visible(const c3dgs_qat_params* q, const float* viewmatrix, uint8_t* visible /*[P]*/, int32_t* rank /*[P]*/,
                      int32_t* count /*device [1]*/, void* scan_workspace, void* stream);
int c3dgs_qat_points(const c3dgs_qat_params* q, const uint8_t* visible, const int32_t* rank, const int64_t* sh_indices,
                     const int64_t* g_indices, float* means3D /*[V,3]*/, float* opacities /*[V,1]*/,
                     float* scale_factors /*[V,1]*/, int64_t* sh_indices_out /*[V]*/, int64_t* g_indices_out /*[V]*/,
                     void* stream);
int c3dgs_qat_points_backward(const c3dgs_qat_params* q, const uint8_t* visible, const int32_t* rank,
                              const float* dL_dmeans3D /*[V,3]*/, const float* dL_dmeans2D /*[V,3]*/,
                              const float* dL_dopacities /*[V,1]*/, const float* dL_dscale_factors /*[V,1]*/,
                              float* dL_dxyz /*[P,3]*/, float* dL_dscreenspace /*[P,3]*/, float* dL_dopacity /*[P,1]*/,
                              float* dL_dscaling_factor /*[P,1]*/, void* stream);
/* int8 payload of GaussianModel.save_npz (scene/gaussian_model.py:525-617): per tensor
 * torch.quantize_per_tensor(activation(raw), scale, zero_point, qint8).int_repr() with the module's CURRENT state:
 * opacity <- sigmoid, scaling <- normalize(relu) (or exp when scaling_is_exp), rotation <- normalize, the rest raw.
 * NULL outputs (or NULL inputs in `q`) are skipped. */
int c3dgs_qat_quantize(const c3dgs_qat_params* q, int32_t scaling_is_exp, int8_t* opacity /*[P,1]*/, int8_t* scaling /*[GS,3]*/,
                       int8_t* scaling_factor /*[P,1]*/, int8_t* rotation /*[GS,4]*/, int8_t* features_dc /*[SHS,1,3]*/,
                       int8_t* features_rest /*[SHS,M-1,3]*/, void* stream);
/* One stand-alone FakeQuantize module on an arbitrary tensor (the mirror of calling the torch module): observe (if
 * `observe`), then out = fake_quantize_per_tensor_affine(x) (copy when !enabled); backward: dx = g * mask. */
int c3dgs_fake_quantize(int64_t n, const float* x, c3dgs_fq_state* state, int32_t observe, int32_t enabled,
                        float averaging_constant, float* out, void* workspace, void* stream);
int c3dgs_fake_quantize_backward(int64_t n, const float* x, const c3dgs_fq_state* state, int32_t enabled, const float* g,
                                 float* dx, void* stream);

/* ---- introspection (tests and profiling only) ---- */
typedef struct c3dgs_geom_layout {   /* byte offsets into the geometry buffer for P Gaussians */
    size_t total_bytes;
    size_t splat;          /* float4[3*P]: {x, y, conic_a, conic_b} {conic_c, opacity, r, g} {b, bits(instance offset), bits(rect_lo), bits(rect_hi)} */
    size_t depth_keys;     /* uint32[P] bits of the view-space depth (the float itself for a visible Gaussian), 0xFFFFFFFF for
                            * culled ones; tiles_touched is the area of `rects`; the sort payload is the Gaussian id itself  */
    size_t depth_keys_sorted; /* uint32[P]                                                 */
    size_t depth_order;    /* uint32[P] Gaussian ids in (depth, id) order                  */
    size_t sorted_offsets; /* uint16[4*P] tile rectangles in DEPTH order (k-th nearest Gaussian); their areas scanned with depth_base[k>>8] give the emission offsets */
    size_t inst_offset;    /* uint32[P] inclusive scan of tiles_touched in ID order WITHIN each 256-Gaussian group; + block_base[i>>8] = backward slot end of i */
    size_t rects;          /* uint16[4*P]: xmin, ymin, xmax, ymax (tile units)             */
    size_t clamped;        /* uint8[P] bit c set = channel c was clamped                   */
    size_t scan_temp;      /* depth-sort temporary storage (control words + ping/pong buffers) */
    size_t scan_temp_bytes;
    size_t block_base;     /* uint32[ceil(P/256)+1] instances before each 256-Gaussian group; last = num_rendered */
    size_t depth_base;     /* uint32[ceil(P/256)+1] the same for groups of the DEPTH order (where the pairs are emitted) */
} c3dgs_geom_layout;

typedef struct c3dgs_binning_layout { /* byte offsets into the binning buffer for R instances */
    size_t total_bytes;
    size_t keys_unsorted;   /* uint16[R] tile id, emitted in (depth, id) order of the Gaussians */
    size_t values_unsorted; /* uint32[R] Gaussian id                                       */
    size_t keys_sorted;     /* uint16[R] tile id after the stable tile sort                */
    size_t point_list;      /* uint32[R] Gaussian ids sorted by (tile, depth, id)          */
    size_t sort_temp;
    size_t sort_temp_bytes;
} c3dgs_binning_layout;

typedef struct c3dgs_image_layout {   /* byte offsets into the image buffer                  */
    size_t total_bytes;
    size_t final_T;    /* float[W*H]                                                       */
    size_t n_contrib;  /* uint32[W*H]                                                      */
    size_t ranges;     /* uint32[2*T]                                                      */
    size_t tile_used;  /* uint32[T] max n_contrib over the tile's pixels                   */
    size_t tile_order; /* uint32[T] scratch of the backward: its tile schedule (ABI version 4)  */
} c3dgs_image_layout;

int c3dgs_get_geom_layout(int32_t P, c3dgs_geom_layout* out);
int c3dgs_get_binning_layout(int32_t R, int32_t W, int32_t H, c3dgs_binning_layout* out);
typedef struct c3dgs_backward_layout { /* byte offsets into the backward workspace for P Gaussians and R instances */
    size_t total_bytes;  /* what the backward asks its workspace callback for = c3dgs_backward_workspace_bytes(P, R)       */
    size_t partials;     /* float[9*R] one slot of nine sums per (Gaussian, tile) instance, contiguous per Gaussian, id order */
    size_t touched;      /* uint8[R] 1 = the blend wrote the slot; the only part cleared per call                          */
    size_t live_ids;     /* uint32[n_lists*list_len], n_lists = ceil(max(P,1) / list_len): list k holds, from its front and in
                          * id order, the blended ones of the Gaussians [k*list_len, (k+1)*list_len)                         */
    size_t live_slots;   /* uint32[n_lists*list_len] the slot of `partials` where the listed Gaussian's nine sums are parked   */
    size_t live_count;   /* uint32[n_lists] entries of each list                                                          */
    size_t list_len;     /* Gaussians per list (1024)                                                                     */
} c3dgs_backward_layout;

int c3dgs_get_image_layout(int32_t W, int32_t H, c3dgs_image_layout* out);
int c3dgs_get_backward_layout(int32_t P, int32_t R, c3dgs_backward_layout* out);
size_t c3dgs_backward_workspace_bytes(int32_t P, int32_t R);   /* total_bytes of c3dgs_backward_layout */

/* tests / tools only: where the forward leaves the tiles' COMPACT lists -- of the list entries a tile visits, those that can reach
 * a pixel of it (non-zero quadrant mask), in list order, densely from the start of the tile's own segment [ranges[tile].x, ...).
 * The backward walks these instead of the point list. Not part of the public buffer layouts (the structs above do not change).
 * Valid after a forward with R > 0, until the binning / image buffers are reused. */
typedef struct c3dgs_compact_layout {
    size_t cqm;         /* binning buffer: uint8[R]  quadrant mask (bit qy*2+qx, never 0) of compact entry ranges[tile].x + k  */
    size_t cid;         /* binning buffer: uint32[R] its Gaussian id; the entries k < tile_used_c[tile] are written            */
    size_t tile_used_c; /* image buffer: uint32[T]   max n_contrib_c over the tile's pixels = compact entries the tile uses    */
    size_t n_contrib_c; /* image buffer: uint32[W*H] 1-based compact index of the pixel's last contributor (0: none)           */
} c3dgs_compact_layout;
int c3dgs_get_compact_layout(int32_t R, int32_t W, int32_t H, c3dgs_compact_layout* out);

/* ---- optional per-stage timing (HIP events on the caller's stream; used by bench.py's roofline leg) ----
 * c3dgs_profile_enable(1) makes every stage launch record a start/stop event pair; c3dgs_profile_read()
 * synchronises those events, returns one record per stage seen since the last read (count returned, at
 * most `capacity`) and resets the accumulators. Disabled (the default) it costs nothing. */
typedef struct c3dgs_stage_time {
    char name[32];
    double total_ms;
    int64_t count;
} c3dgs_stage_time;
int c3dgs_profile_enable(int on);
/* Restrict the event pairs to ONE stage (by the name c3dgs_profile_read reports, e.g. "render_backward"); NULL or "" =
 * every stage. Every event pair costs a few microseconds of queue time, so a timed region brackets only the kernel
 * it needs. */
int c3dgs_profile_only(const char* stage_name);
int c3dgs_profile_read(c3dgs_stage_time* out, int capacity);

const char* c3dgs_last_error(void);
int c3dgs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* C3DGS_HIP_H */
