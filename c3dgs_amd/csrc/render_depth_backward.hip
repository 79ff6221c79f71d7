// render_depth_backward.hip -- gradients through the depth and accumulated-opacity maps of render_depth.hip, for gfx950.
// The reference's rasterizer has no counterpart.
//
// Per pixel, over the entries k = 1..m the forward blended, with w_k = alpha_k T_k, D = sum w_k z_k, A = sum w_k, the incoming
// gradients gD = dL/dD[pix], gA = dL/dA[pix] and c_k = gD z_k + gA:
//     dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k)           (no background term: A telescopes)
//     dL/dz_g     = sum over the pixels of w_k gD
// From dL/dalpha_k the chain to opacity, conic and 2D mean is render_backward_kernel's for a colour channel: the six moments
// {S0, Sx, Sy, Sxx, Sxy, Syy} of G dL/dalpha about the Gaussian's 2D mean, which backward_preprocess.hip turns into the gradients.
//
// Two launches behind render_backward (or behind the flag clear alone, when the loss does not use the image), no float
// atomics, bitwise reproducible:
//   A  render_depth_backward_kernel: a replay of the finished forward (replay.hpp: the tile walk, the staging, the candidate
//      lists and the forward's cuts tile_used_c / n_contrib_c; it decides nothing again), walked BACK TO FRONT with
//      render_backward_kernel's recurrences: T starts at the forward's final_T and is divided by (1 - alpha) on the way to the
//      front, the "what lies behind" sum grows from 0. Per row of 8 candidates the
//      per-pixel terms {w, w dx, w dx^2, alpha T gD} are reduced over a pixel row with the column levels of render_common.hpp's
//      transposing butterfly, the row's dy gives the y-moments, the row levels add the seven sums over the 8 rows (the pairings
//      and roundings of render_backward_kernel's network, so the sums are that kernel's for a colour channel), the four
//      waves meet in LDS, and one thread per entry merges them, (0 + 1) + (2 + 3), and ADDS the six moments into the entry's
//      36-byte slot of the product backward's partial sums (entry_slot(); read-add-store where the slot's flag byte is set, a
//      store that sets the byte otherwise; the colour components stay as they are). A slot belongs to one (Gaussian, tile), i.e.
//      to one workgroup of this grid, and render_backward has finished on the stream: no race. dL/dz goes to a 4-byte plane of
//      its own in the same slot numbering; it is written for every slot whose flag is set afterwards.
//   B  depth_backward_fold_kernel, behind backward_preprocess: one lane per LISTED Gaussian folds the flagged slots of its run of
//      the dL/dz plane with fold_slot_run() and adds dL/dz x the depth row of the view matrix -- the row preprocess forms the
//      stored depth from, xform4x3's z -- into dL_dmeans3D.
// Both honour the sort's time-out word: set -> A walks nothing, B poisons the listed rows with NaN.
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

constexpr int DEPTH_BWD_TERMS = 7;    // S0, Sx, Sy, Sxx, Sxy, Syy, dz

// ---- stage A
// The four per-wave planes of seven floats per batch entry are 28 KB; with the staged records and lists 50,624 B of LDS = three
// workgroups per CU, i.e. three waves per SIMD (at most 168 VGPRs: the 32 values of a row of 8 stay in registers, no scratch).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
render_depth_backward_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                             const uint32_t* __restrict__ n_contrib_c, const float* __restrict__ final_Ts,
                             const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm, const float4* __restrict__ splat,
                             const uint32_t* __restrict__ depth_keys, const uint32_t* __restrict__ block_base,
                             const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha_map,
                             float* __restrict__ partials, float* __restrict__ dz_plane, uint8_t* __restrict__ touched,
                             const uint32_t* __restrict__ sort_err)
{
    // every product below is rounded on its own, as in render_backward_kernel, whose terms feed hand-placed DPP adds: the sums are
    // then that kernel's bits for a colour channel (explicit fmaf calls are not affected)
#pragma clang fp contract(off)
    if (block_has_no_tile(blockIdx.x, T)) return;
    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing (stage B writes NaN)
    if (*sort_err != 0u) return;
    __shared__ ReplayStage st;                       // the staged record carries z in place of the red
    __shared__ float s_stat[4][BATCH][DEPTH_BWD_TERMS];   // [wave][batch entry] the seven sums over the wave's 64 pixels
    __shared__ uint8_t s_hits[4][BATCH];             // ... and whether any of them blended it
    static_assert(sizeof(st) + sizeof(s_stat) + sizeof(s_hits) <= 41 * 1280,
                  "render_depth_backward: more than 41 LDS granules = two workgroups per CU instead of three");

    // t.last is where this pixel's walk starts
    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, false, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;
    float Tr = t.inside ? final_Ts[t.pix] : 0.f;                // transmittance behind the pixel's last blended entry
    const float gD = (t.inside && dL_ddepth) ? dL_ddepth[t.pix] : 0.f;
    const float gA = (t.inside && dL_dalpha_map) ? dL_dalpha_map[t.pix] : 0.f;
    float Sd = 0.f;                                             // sum_{j behind} w_j c_j

    const int beta = candidate_of_lane(lane);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u, slot_next = 0u;
    // batch entry j of round r is compact entry used - 1 - (r * BATCH + j): back to front, as render_backward walks
    auto gather = [&](int back) {                               // `back`-th entry from the end -> this thread's staging registers
        qm = 0u;
        const int pos = t.used - 1 - back;
        if (pos >= 0) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            rb.z = __uint_as_float(depth_keys[id]);             // in place of the record's red
            slot_next = entry_slot(splat[3 * (size_t)id + 2], block_base, id, t.tx, t.ty);
        }
    };
    gather(tid);
    for (int r = 0; r < t.rounds; r++) {
        const int buf = r & 1;
        const uint32_t slot = slot_next;                        // of batch entry `tid`, which this thread stages and later merges
        stage_batch(st, buf, tid, ra, rb);
        publish_quadrant_masks(st, buf, wave, lane, qm);
        // a wave only writes the entries of its own candidate list: the others read as "nothing blended". This thread read
        // its entry's words of the previous batch behind that batch's second barrier, so it may clear them here.
#pragma unroll
        for (int w = 0; w < 4; w++) {
#pragma unroll
            for (int q = 0; q < DEPTH_BWD_TERMS; q++) s_stat[w][tid][q] = 0.f;
            s_hits[w][tid] = 0;
        }
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        const int pos0 = t.used - 1 - r * BATCH;                // 0-based compact position of batch entry j is pos0 - j
        // entries at position >= wave_last (j <= pos0 - wave_last) lie behind every pixel of this wave
        const int jmin = pos0 - t.wave_last + 1;
        if (jmin < BATCH) {
            const int nw = build_candidate_list(st, buf, wave, lane,
                                                [&](unsigned long long m, int c) { return drop_behind(m, jmin - c * 64); });
            // a pixel takes entry j only if pos0 - j < last, i.e. record offset > thr (the sentinel's opacity is 0: never a hit)
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
                    // in front of the pixel's last contributor every hit was blended by the forward (its stop lies behind it)
                    hit = hit && ((int)e[g] > thr);
                    // branch-free, as render_backward: a pixel that does not blend the entry runs the same instructions with
                    // alpha = G = 0, which leaves T and Sd untouched and makes all seven terms exactly 0
                    const float a_eff = hit ? alpha : 0.f, G_eff = hit ? G : 0.f;
                    const float rinv = __builtin_amdgcn_rcpf(1.f - a_eff);   // 1 - alpha is in [0.01, 1]; rcp(1) == 1
                    Tr = Tr * rinv;                              // transmittance in front of this entry
                    const float wgt = a_eff * Tr;                // alpha_k T_k
                    const float cd = s.b.z * gD + gA;            // two roundings: the colour backward's (z, 1, 0) . (gD, gA, 0)
                    const float dL_dalpha = fmaf(Tr, cd, -(rinv * Sd));
                    Sd = fmaf(wgt, cd, Sd);
                    // w = G * dL/dalpha and its first two x-moments about the mean; the y-moments follow from the row sums
                    const float w = G_eff * dL_dalpha, wx = w * dx;
                    v0[g] = w; vx[g] = wx; vxx[g] = wx * dx;
                    vz[g] = wgt * gD;
                    const uint32_t h = __ballot(hit) != 0ull ? 1u : 0u;
                    my_hit = (beta == g) ? h : my_hit;
                }
                // column levels: the sums over this lane's pixel row of candidate beta; then this row's dy to that candidate (the
                // same subtraction gaussian_alpha made for it) gives the row's y-moments, and the row levels add the 8 rows up:
                // render_backward_kernel's pairings and roundings, term for term
                const float c0 = reduce_columns_of_8(v0, lane, OpAdd()), cx = reduce_columns_of_8(vx, lane, OpAdd());
                const float cxx = reduce_columns_of_8(vxx, lane, OpAdd()), cz = reduce_columns_of_8(vz, lane, OpAdd());
                const float dyb = staged_mean_y(st, my_off) - t.pyf;
                float sum[DEPTH_BWD_TERMS];
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
                    for (int q = 0; q < DEPTH_BWD_TERMS; q++) s_stat[wave][myj][q] = sum[q];
                    s_hits[wave][myj] = (uint8_t)my_hit;
                }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves, (0 + 1) + (2 + 3) as render_backward_kernel's flush, and owns the slot
        if (r * BATCH + tid < t.used) {
            const uint32_t h = (uint32_t)s_hits[0][tid] | s_hits[1][tid] | s_hits[2][tid] | s_hits[3][tid];
            const bool was = touched[slot] != 0;
            if (h || was) {
                float t[DEPTH_BWD_TERMS];
#pragma unroll
                for (int q = 0; q < DEPTH_BWD_TERMS; q++)
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

// ---- stage B: one lane per listed Gaussian (sum_partials_kernel's lists: BWD_LIST entries per list, filled from the front, the
// grid and the workgroup -> (list, quarter) map of backward_preprocess_kernel) folds the flagged slots of its run of the dL/dz
// plane (replay.hpp)
__global__ void __launch_bounds__(256)
depth_backward_fold_kernel(int P, const uint32_t* __restrict__ live_count, const uint32_t* __restrict__ live_ids,
                           const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base,
                           const float* __restrict__ dz_plane, const uint8_t* __restrict__ touched,
                           const float* __restrict__ view, float* __restrict__ dL_dmeans3D, const uint32_t* __restrict__ sort_err)
{
    const uint32_t n_lists = gridDim.x / (BWD_LIST / 256);
    const uint32_t list = blockIdx.x % n_lists, quarter = blockIdx.x / n_lists;
    const uint32_t n_live = live_count[list];
    const uint32_t off = quarter * 256u + threadIdx.x;
    if ((off & ~63u) >= n_live) return;                          // whole waves only: the shuffles below need every lane
    const int lane = threadIdx.x & 63;
    const bool live = off < n_live;
    const int i = live ? (int)live_ids[(size_t)list * BWD_LIST + off] : 0;
    float sum = 0.f;
    if (*sort_err != 0u) {
        sum = __uint_as_float(0x7fc00000u);
    } else {
        SlotRun run = { 0u, 0u };
        if (live && i < P) run = slot_run(i, inst_offset, block_base);
        sum = fold_slot_run(run, dz_plane, touched, lane);
    }
    if (!live || i >= P) return;
    // z = view[2] x + view[6] y + view[10] z + view[14] (gsmath.hpp: xform4x3, what preprocess stores as the depth)
    float* dst = dL_dmeans3D + 3 * (size_t)i;
    dst[0] += sum * view[2];
    dst[1] += sum * view[6];
    dst[2] += sum * view[10];
}

void launch_render_depth_backward(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const BwdPtrs& w,
                                  float* dz_plane, const float* dL_ddepth, const float* dL_dalpha, const uint32_t* sort_err,
                                  hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_depth_backward_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, img.final_T,
                                                                cl.cid, cl.cqm, g.splat, g.depth_keys, g.block_base, dL_ddepth,
                                                                dL_dalpha, w.partials, dz_plane, w.touched, sort_err);
}

void launch_depth_backward_fold(int P, const GeomPtrs& g, const BwdPtrs& w, const float* dz_plane, const float* view,
                                float* dL_dmeans3D, const uint32_t* sort_err, hipStream_t s)
{
    if (P <= 0) return;
    const int n_lists = (P + BWD_LIST - 1) / BWD_LIST;
    depth_backward_fold_kernel<<<n_lists * (BWD_LIST / 256), 256, 0, s>>>(P, w.live_count, w.live_ids, g.inst_offset, g.block_base,
                                                                          dz_plane, w.touched, view, dL_dmeans3D, sort_err);
}

} // namespace c3dgs
