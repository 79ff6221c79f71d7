// render_distortion.hip -- the depth-distortion map of a finished forward (Mip-NeRF 360's regulariser, as 2DGS and gsplat use it),
// for gfx950. Forward-only; the reference's rasterizer has no counterpart.
//
// Per pixel, over the entries k = 1..m the forward blended, with w_k = alpha_k T_k, T_{k+1} = T_k (1 - alpha_k), T_1 = 1,
// z_k = the fp32 view-space depth preprocess stored for the Gaussian (the bits in depth_keys[id]) and s_k = f(z_k):
//     raw mode            f(z) = z
//     ndc(near, far) mode f(z) = far / (far - near) * (1 - near / z)          (2DGS's mapping; increasing in z)
//     distortion = sum_i sum_j w_i w_j |s_i - s_j| = 2 sum_k w_k (s_k A_<k - S_<k),   A_<k = 1 - T_k,  S_<k = sum_{j<k} w_j s_j
//     moment     = sum_k w_k s_k
// The second form holds because a tile's list is in ascending fp32 depth and f is increasing. There is no 1/3 sum w^2 delta term.
//
// A replay of the forward (replay.hpp: the tile walk, the staging and the candidate lists), front to back: render_depth_kernel's
// sibling. The staged record carries s - c0 (common.hpp: DistortionMap) in place of the red, computed once per entry by the thread
// that stages it. Four running values per pixel: T, the pixel's first blended s as a pivot p, and S_< and the distortion on
// s - p. The map does not change when every s of a pixel moves by a constant, and its fp32 round-off then scales with the ray's
// spread and not with s; the moment is put together at the end, M = c0 A + p A + sum w (s - c0 - p) with A = 1 - T, so that it
// is sum w s to within a rounding of its own size -- which is what the backward's own pivot needs of it
// (render_maps_backward.hip). No atomics, no scratch, no list stores: bitwise reproducible.
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

// seven waves per SIMD (at most 72 VGPRs), render_depth_kernel's occupancy and for its reason: 50 VGPRs (one more than that
// kernel), its 20,928 B of LDS (17 granules of 1280 B: seven workgroups per CU), no scratch
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7)))
render_distortion_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                         const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                         const float4* __restrict__ splat, const uint32_t* __restrict__ depth_keys, DistortionMap f,
                         float* __restrict__ out_distortion, float* __restrict__ out_moment, const uint32_t* __restrict__ sort_err)
{
    if (block_has_no_tile(blockIdx.x, T)) return;
    __shared__ ReplayStage st;
    static_assert(sizeof(st) <= 18 * 1280, "render_distortion: more than 18 LDS granules = six workgroups per CU instead of seven");

    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing, every output is NaN
    const bool poisoned = *sort_err != 0u;
    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, poisoned, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;

    float Tr = 1.0f, S = 0.f, dist = 0.f, p = 0.f;              // T_k, S_<k and sum_{j<k} w_j (s_j A_<j - S_<j) about p, the pivot

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u;
    auto gather = [&](int pos) {                                // compact entry `pos` of the tile -> this thread's staging registers
        qm = 0u;
        if (pos < t.used) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            const float z = __uint_as_float(depth_keys[id]);
            rb.z = f.rel(z, f.rz(z));                           // in place of the record's red
        }
    };
    gather(tid);
    for (int r = 0; r < t.rounds; r++) {
        const int buf = r & 1;
        stage_batch(st, buf, tid, ra, rb);
        publish_quadrant_masks(st, buf, wave, lane, qm);
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        const int jend = t.wave_last - r * BATCH;
        if (jend <= 0) continue;
        const int nw = build_candidate_list(st, buf, wave, lane,
                                            [&](unsigned long long m, int c) { return keep_in_front(m, jend - c * 64); });
        const int thr = front_cut(buf, t.last - r * BATCH);
        for (int k = 0; k < nw; k += 8) {
            uint32_t e[8];
            load_row(st, wave, k, e);
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const StagedRecord s = staged_record(st, e[g]);
                float dx, dy, G, alpha;
                const bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                const bool blend = hit && ((int)e[g] < thr);
                const float w = blend ? alpha * Tr : 0.f;
                p = (blend && Tr == 1.0f) ? s.b.z : p;          // T is 1 until the first blend and below 1 behind it
                const float sp = s.b.z - p;
                // w = 0 leaves all three as they are
                dist = fmaf(w, fmaf(sp, 1.0f - Tr, -S), dist);
                S = fmaf(sp, w, S);
                Tr = blend ? Tr * (1.f - alpha) : Tr;
            }
        }
    }
    if (t.inside) {
        const float poison = poisoned ? __uint_as_float(0x7fc00000u) : 0.f;
        out_distortion[t.pix] = 2.0f * dist + poison;
        if (out_moment) out_moment[t.pix] = fmaf(f.c0, 1.0f - Tr, fmaf(p, 1.0f - Tr, S)) + poison;
    }
}

void launch_render_distortion(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const uint32_t* depth_keys,
                              const DistortionMap& f, float* out_distortion, float* out_moment, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_distortion_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm,
                                                            splat, depth_keys, f, out_distortion, out_moment, sort_err);
}

} // namespace c3dgs
