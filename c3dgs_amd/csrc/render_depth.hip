// render_depth.hip -- depth, accumulated opacity and median depth of a finished forward, for gfx950. Forward-only; the
// reference's rasterizer has no counterpart.
//
// Per pixel, over the entries k = 1..m the forward blended, with w_k = alpha_k T_k, T_{k+1} = T_k (1 - alpha_k), T_1 = 1 and
// z_k = the fp32 view-space depth preprocess stored for the Gaussian (the bits in depth_keys[id]):
//     depth  = sum_k w_k z_k      accumulated like a colour channel of the forward (fmaf in list order, from 0); not normalised
//     alpha  = 1 - T_{m+1}        from this kernel's own replayed T
//     median = z_k of the first blended entry with T_{k+1} < 0.5, or 0
//
// A replay of the forward (replay.hpp: the tile walk, the staging and the candidate lists), front to back. The staged record
// carries z in place of the red. No atomics, no scratch, no list stores.
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

// seven waves per SIMD (at most 72 VGPRs), the forward's occupancy: left alone, the scheduler hoists the LDS reads of a whole row
// of 8 and takes 90
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7)))
render_depth_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                    const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                    const float4* __restrict__ splat, const uint32_t* __restrict__ depth_keys, float* __restrict__ out_depth,
                    float* __restrict__ out_alpha, float* __restrict__ out_median, const uint32_t* __restrict__ sort_err)
{
    if (block_has_no_tile(blockIdx.x, T)) return;
    __shared__ ReplayStage st;
    static_assert(sizeof(st) <= 18 * 1280, "render_depth: more than 18 LDS granules = six workgroups per CU instead of seven");

    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing, every output is NaN
    const bool poisoned = *sort_err != 0u;
    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, poisoned, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;

    float Tr = 1.0f, D = 0.f, med = 0.f;

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u;
    auto gather = [&](int pos) {                                // compact entry `pos` of the tile -> this thread's staging registers
        qm = 0u;
        if (pos < t.used) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            rb.z = __uint_as_float(depth_keys[id]);             // in place of the record's red
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
                const float test_T = Tr * (1.f - alpha);
                const float w = blend ? alpha * Tr : 0.f;
                D = fmaf(s.b.z, w, D);
                // T only falls: the first entry that takes it below 0.5 is the one that finds it at or above
                med = (blend && test_T < 0.5f && !(Tr < 0.5f)) ? s.b.z : med;
                Tr = blend ? test_T : Tr;
            }
        }
    }
    if (t.inside) {
        const float poison = poisoned ? __uint_as_float(0x7fc00000u) : 0.f;
        if (out_depth) out_depth[t.pix] = D + poison;
        if (out_alpha) out_alpha[t.pix] = (1.0f - Tr) + poison;
        if (out_median) out_median[t.pix] = med + poison;
    }
}

void launch_render_depth(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const uint32_t* depth_keys,
                         float* out_depth, float* out_alpha, float* out_median, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_depth_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm, splat,
                                                       depth_keys, out_depth, out_alpha, out_median, sort_err);
}

} // namespace c3dgs
