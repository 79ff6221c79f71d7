// render_normal.hip -- the blended normal map of a finished forward, for gfx950. Forward-only; the reference's rasterizer has no
// counterpart.
//
// Per pixel, over the entries k = 1..m the forward blended, with w_k = alpha_k T_k, T_{k+1} = T_k (1 - alpha_k), T_1 = 1 and
// n_k = the view-space normal gaussian_normals_kernel (normals.hip) wrote for the Gaussian:
//     normal_c = sum_k w_k n_k,c     accumulated like a colour channel of the forward (fmaf in list order, from 0); not normalised,
//                                    no background term: render_depth's convention for `depth`
//
// A replay of the forward (replay.hpp: the tile walk, the staging and the candidate lists), front to back: render_depth_kernel's
// sibling. The 32-byte staged record has two spare words and a normal has three components: n_x and n_y ride in the record
// (in place of the red and behind it), n_z in a plane of its own, one float per staged entry, double-buffered like the records
// and addressed by the record's byte offset / 8 (a record is 32 bytes, a float 4). No atomics, no scratch, no list stores:
// bitwise reproducible.
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

// seven waves per SIMD (at most 72 VGPRs), render_depth_kernel's occupancy and for its reason. LDS: the 20,928 B of the stage +
// 2,056 B of the n_z plane = 22,984 B = 18 granules of 1280 B, the last count at which seven workgroups fit a CU
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7)))
render_normal_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                     const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                     const float4* __restrict__ splat, const float4* __restrict__ normals, float* __restrict__ out_normal,
                     const uint32_t* __restrict__ sort_err)
{
    if (block_has_no_tile(blockIdx.x, T)) return;
    __shared__ ReplayStage st;
    __shared__ float s_nz[2 * (BATCH + 1)];                     // [buf][batch entry], the sentinels included
    static_assert(sizeof(st) + sizeof(s_nz) <= 18 * 1280, "render_normal: more than 18 LDS granules = six workgroups per CU instead of seven");
    static_assert(REPLAY_REC_BYTES == 32 && REPLAY_BUF_BYTES == (BATCH + 1) * REPLAY_REC_BYTES, "s_nz is addressed by record byte offset / 8: one float per 32-byte record");

    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing, every output is NaN
    const bool poisoned = *sort_err != 0u;
    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, poisoned, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;
    if (tid < 2) s_nz[tid * (BATCH + 1) + BATCH] = 0.f;         // the sentinels blend nothing, but 0 x their n_z must be 0

    float Tr = 1.0f, N0 = 0.f, N1 = 0.f, N2 = 0.f;

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    float nz = 0.f;
    uint32_t qm = 0u;
    auto gather = [&](int pos) {                                // compact entry `pos` of the tile -> this thread's staging registers
        qm = 0u;
        if (pos < t.used) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            const float4 n = normals[id];
            rb.z = n.x; rb.w = n.y; nz = n.z;                   // in place of the record's red, in its spare word, in the plane
        }
    };
    gather(tid);
    for (int r = 0; r < t.rounds; r++) {
        const int buf = r & 1;
        stage_batch(st, buf, tid, ra, rb);
        s_nz[buf * (BATCH + 1) + tid] = nz;
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
                const float sz = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(s_nz) + (e[g] >> 3));
                float dx, dy, G, alpha;
                const bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                const bool blend = hit && ((int)e[g] < thr);
                const float w = blend ? alpha * Tr : 0.f;
                N0 = fmaf(s.b.z, w, N0);
                N1 = fmaf(s.b.w, w, N1);
                N2 = fmaf(sz, w, N2);
                Tr = blend ? Tr * (1.f - alpha) : Tr;
            }
        }
    }
    if (t.inside) {
        const float poison = poisoned ? __uint_as_float(0x7fc00000u) : 0.f;
        const size_t n_pix = (size_t)W * H;
        out_normal[t.pix] = N0 + poison;
        out_normal[n_pix + t.pix] = N1 + poison;
        out_normal[2 * n_pix + t.pix] = N2 + poison;
    }
}

void launch_render_normal(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const float* normals,
                          float* out_normal, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_normal_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm, splat,
                                                        reinterpret_cast<const float4*>(normals), out_normal, sort_err);
}

} // namespace c3dgs
