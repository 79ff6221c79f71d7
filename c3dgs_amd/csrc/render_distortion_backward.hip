// render_distortion_backward.hip -- gradients through the depth, accumulated-opacity and distortion maps (render_depth.hip,
// render_distortion.hip) in ONE blend replay, for gfx950. The reference's rasterizer has no counterpart.
//
// render_depth_backward_kernel's sibling: where the loss uses the distortion map this kernel runs INSTEAD of that one, so a
// backward never replays the blend twice for its maps. Per pixel, over the entries k = 1..m the forward blended, with
// w_k = alpha_k T_k, s_k = f(z_k) (common.hpp: DistortionMap), the incoming gradients gD, gA, gL of the depth, alpha and distortion
// maps at the pixel, M = the pixel's moment sum_k w_k s_k (render_distortion's second output) and
//     A_<k = 1 - T_k,   A_>k = T_{k+1} - T_{m+1},   S_>k = sum_{j>k} w_j s_j,   S_<k = M - S_>k - w_k s_k:
//     u_k         = dL/dw_k through the distortion = 2 gL (s_k (A_<k - A_>k) - S_<k + S_>k)
//     c_k         = gD z_k + gA + u_k
//     dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k)            (no background term)
//     dL/dz_k     = w_k (gD + 2 gL (A_<k - A_>k) f'(z_k))
// The loss does not change when every s of a pixel moves by a constant, but fp32 sums of w s do: u_k is a difference of sums of
// the size of s, which cancels where a pixel's mass is concentrated (the ndc mode: s near 1, spreads of 0.01). So the recurrences
// run on s_k - p with the pivot p = M / A, A = 1 - T_{m+1}, and the moment M - p A (what fp32 leaves of zero); every equation
// above holds for any p. s_k - p is formed in one rounding at the size of the difference (DistortionMap::about), and the forward
// hands over an M that is sum w s to within one rounding of its own size (render_distortion.hip sums about a pivot of its own).
// tests/test_distortion_ref_cpu.py restates both kernels in fp32 and holds them to half the GPU bars; the plain recurrences miss
// them there by a factor of up to nine.
// Walked BACK TO FRONT exactly as render_depth_backward_kernel walks (see there for the reduction network, the slots, the flags
// and the dL/dz plane, which depth_backward_fold_kernel folds behind backward_preprocess as it does for that kernel): T starts at
// the forward's final_T = T_{m+1} and is divided by (1 - alpha); the two suffix sums S_> and sum w c grow from 0. The staged
// record carries z in place of the red and 1 / z in its spare word. No float atomics, bitwise reproducible.
// The sort's time-out word set: walks nothing (the fold writes NaN).
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

constexpr int DIST_BWD_TERMS = 7;     // S0, Sx, Sy, Sxx, Sxy, Syy, dz: render_depth_backward_kernel's seven

// render_depth_backward_kernel's footprint: 50,624 B of LDS = three workgroups per CU, i.e. three waves per SIMD (at most 168
// VGPRs; it takes 100, no scratch)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
render_distortion_backward_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges,
                                  const uint32_t* __restrict__ tile_used_c, const uint32_t* __restrict__ n_contrib_c,
                                  const float* __restrict__ final_Ts, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                                  const float4* __restrict__ splat, const uint32_t* __restrict__ depth_keys,
                                  const uint32_t* __restrict__ block_base, const float* __restrict__ dL_ddepth,
                                  const float* __restrict__ dL_dalpha_map, const float* __restrict__ dL_ddistortion,
                                  const float* __restrict__ moment, DistortionMap f, float* __restrict__ partials,
                                  float* __restrict__ dz_plane, uint8_t* __restrict__ touched, const uint32_t* __restrict__ sort_err)
{
    // every product below is rounded on its own, as in render_depth_backward_kernel (explicit fmaf calls are not affected)
#pragma clang fp contract(off)
    if (block_has_no_tile(blockIdx.x, T)) return;
    if (*sort_err != 0u) return;
    __shared__ ReplayStage st;                       // the staged record carries z in place of the red, 1 / z behind it
    __shared__ float s_stat[4][BATCH][DIST_BWD_TERMS];    // [wave][batch entry] the seven sums over the wave's 64 pixels
    __shared__ uint8_t s_hits[4][BATCH];             // ... and whether any of them blended it
    static_assert(sizeof(st) + sizeof(s_stat) + sizeof(s_hits) <= 41 * 1280,
                  "render_distortion_backward: more than 41 LDS granules = two workgroups per CU instead of three");

    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, false, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;
    const float Tfin = t.inside ? final_Ts[t.pix] : 0.f;        // T_{m+1}: transmittance behind the pixel's last blended entry
    float Tr = Tfin;
    const float gD = (t.inside && dL_ddepth) ? dL_ddepth[t.pix] : 0.f;
    const float gA = (t.inside && dL_dalpha_map) ? dL_dalpha_map[t.pix] : 0.f;
    const float gL2 = t.inside ? 2.0f * dL_ddistortion[t.pix] : 0.f;
    // the pivot: every s of the pixel is taken about the pixel's mean s = moment / A, and the moment with it
    const float Apix = 1.0f - Tfin;
    const float Mraw = t.inside ? moment[t.pix] : 0.f;
    const float piv = Apix > 0.f ? Mraw / Apix : 0.f;
    const float M = fmaf(-piv, Apix, Mraw);                     // sum_k w_k (s_k - piv): what fp32 leaves of 0
    const float qs = f.c0 - piv;                                // s_k - piv = DistortionMap::about(z, 1 / z, qs), one rounding
    float Sd = 0.f;                                             // sum_{j behind} w_j c_j
    float Ss = 0.f;                                             // S_>: sum_{j behind} w_j (s_j - piv)

    const int beta = candidate_of_lane(lane);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u, slot_next = 0u;
    auto gather = [&](int back) {                               // `back`-th entry from the end -> this thread's staging registers
        qm = 0u;
        const int pos = t.used - 1 - back;
        if (pos >= 0) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            rb.z = __uint_as_float(depth_keys[id]);             // in place of the record's red
            rb.w = f.rz(rb.z);                                  // the record's spare word
            slot_next = entry_slot(splat[3 * (size_t)id + 2], block_base, id, t.tx, t.ty);
        }
    };
    gather(tid);
    for (int r = 0; r < t.rounds; r++) {
        const int buf = r & 1;
        const uint32_t slot = slot_next;                        // of batch entry `tid`, which this thread stages and later merges
        stage_batch(st, buf, tid, ra, rb);
        publish_quadrant_masks(st, buf, wave, lane, qm);
#pragma unroll
        for (int w = 0; w < 4; w++) {
#pragma unroll
            for (int q = 0; q < DIST_BWD_TERMS; q++) s_stat[w][tid][q] = 0.f;
            s_hits[w][tid] = 0;
        }
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        const int pos0 = t.used - 1 - r * BATCH;                // 0-based compact position of batch entry j is pos0 - j
        const int jmin = pos0 - t.wave_last + 1;
        if (jmin < BATCH) {
            const int nw = build_candidate_list(st, buf, wave, lane,
                                                [&](unsigned long long m, int c) { return drop_behind(m, jmin - c * 64); });
            const int thr = (int)((uint32_t)buf * REPLAY_BUF_BYTES) + min(max(pos0 - t.last, -1), BATCH) * (int)REPLAY_REC_BYTES;
            for (int k = 0; k < nw; k += 8) {
                uint32_t e[8];
                load_row(st, wave, k, e);
                const uint32_t my_off = st.list[wave][k + beta];  // the candidate this lane reports on
                float v0[8], vx[8], vxx[8], vz[8];
                uint32_t my_hit = 0u;
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const StagedRecord s = staged_record(st, e[g]);
                    float dx, dy, G, alpha;
                    bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                    hit = hit && ((int)e[g] > thr);
                    // branch-free: a pixel that does not blend the entry runs the same instructions with alpha = G = 0, which leaves
                    // T and the suffix sums untouched and makes all seven terms exactly 0
                    const float a_eff = hit ? alpha : 0.f, G_eff = hit ? G : 0.f;
                    const float rinv = __builtin_amdgcn_rcpf(1.f - a_eff);   // 1 - alpha is in [0.01, 1]; rcp(1) == 1
                    const float dA = (1.0f - Tr * rinv) - (Tr - Tfin);       // A_<k - A_>k: Tr still is T_{k+1}
                    Tr = Tr * rinv;                              // transmittance in front of this entry
                    const float wgt = a_eff * Tr;                // alpha_k T_k
                    const float sk = f.about(s.b.z, s.b.w, qs);
                    const float ws = wgt * sk;
                    const float Slt = (M - Ss) - ws;             // S_<k
                    const float u = gL2 * fmaf(sk, dA, Ss - Slt);
                    const float cd = (s.b.z * gD + gA) + u;
                    const float dL_dalpha = fmaf(Tr, cd, -(rinv * Sd));
                    Sd = fmaf(wgt, cd, Sd);
                    Ss = Ss + ws;
                    const float w = G_eff * dL_dalpha, wx = w * dx;
                    v0[g] = w; vx[g] = wx; vxx[g] = wx * dx;
                    vz[g] = wgt * fmaf(gL2 * dA, f.ds(s.b.w), gD);
                    const uint32_t h = __ballot(hit) != 0ull ? 1u : 0u;
                    my_hit = (beta == g) ? h : my_hit;
                }
                const float c0 = reduce_columns_of_8(v0, lane, OpAdd()), cx = reduce_columns_of_8(vx, lane, OpAdd());
                const float cxx = reduce_columns_of_8(vxx, lane, OpAdd()), cz = reduce_columns_of_8(vz, lane, OpAdd());
                const float dyb = staged_mean_y(st, my_off) - t.pyf;
                float sum[DIST_BWD_TERMS];
                sum[0] = reduce_rows_of_8(c0, OpAdd());
                sum[1] = reduce_rows_of_8(cx, OpAdd());
                sum[2] = reduce_rows_of_8(dyb * c0, OpAdd());
                sum[3] = reduce_rows_of_8(cxx, OpAdd());
                sum[4] = reduce_rows_of_8(dyb * cx, OpAdd());
                sum[5] = reduce_rows_of_8((dyb * dyb) * c0, OpAdd());
                sum[6] = reduce_rows_of_8(cz, OpAdd());
                // each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane
                const int myj = batch_entry_of(my_off, buf);
                if (lane < 8 && myj < BATCH) {
#pragma unroll
                    for (int q = 0; q < DIST_BWD_TERMS; q++) s_stat[wave][myj][q] = sum[q];
                    s_hits[wave][myj] = (uint8_t)my_hit;
                }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves, (0 + 1) + (2 + 3), and owns the slot
        if (r * BATCH + tid < t.used) {
            const uint32_t h = (uint32_t)s_hits[0][tid] | s_hits[1][tid] | s_hits[2][tid] | s_hits[3][tid];
            const bool was = touched[slot] != 0;
            if (h || was) {
                float t[DIST_BWD_TERMS];
#pragma unroll
                for (int q = 0; q < DIST_BWD_TERMS; q++)
                    t[q] = (s_stat[0][tid][q] + s_stat[1][tid][q]) + (s_stat[2][tid][q] + s_stat[3][tid][q]);
                float* dst = partials + (size_t)slot * PARTIAL_FLOATS;
                if (was) {
                    if (h) {
#pragma unroll
                        for (int q = 0; q < 6; q++) dst[3 + q] += t[q];
                    }
                } else {
                    dst[0] = 0.f; dst[1] = 0.f; dst[2] = 0.f;
#pragma unroll
                    for (int q = 0; q < 6; q++) dst[3 + q] = t[q];
                    touched[slot] = 1;
                }
                dz_plane[slot] = t[6];                           // valid wherever the flag is set behind this kernel
            }
        }
    }
}

void launch_render_distortion_backward(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const BwdPtrs& w,
                                       float* dz_plane, const float* dL_ddepth, const float* dL_dalpha, const float* dL_ddistortion,
                                       const float* moment, const DistortionMap& f, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_distortion_backward_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c,
                                                                     img.final_T, cl.cid, cl.cqm, g.splat, g.depth_keys, g.block_base,
                                                                     dL_ddepth, dL_dalpha, dL_ddistortion, moment, f, w.partials,
                                                                     dz_plane, w.touched, sort_err);
}

} // namespace c3dgs
