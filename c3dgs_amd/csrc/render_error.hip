// render_error.hip -- per-Gaussian error scores of a finished forward, for gfx950. Forward-only; the reference's rasterizer has
// no counterpart.
//
// For every Gaussian g, over the (pixel, entry) pairs the forward BLENDED, with w = alpha * T in fp32 and e = pixel_map[pixel]:
//     err_sum[g] = sum fl(w * e)
// the score of error-based densification ("Revising Densification in Gaussian Splatting": E_g = sum over pixels of w_g e).
//
// Three launches, no float atomics, bitwise reproducible:
//   clear  the `touched` bytes of the workspace (backward_prep_kernel's fill workgroups: launch_backward_prep with no tiles)
//   A'     render_error_kernel: a replay of the forward (replay.hpp: the tile walk, the staging and the candidate lists), front to
//          back. A pixel reads its map value once; per pair the weight is multiplied by it (its own rounding, never fused), ONE
//          add network per row of 8 candidates (render_common.hpp's transposing butterfly), the four waves merged in wave order
//          0..3, one plain 4-byte store + a flag byte per (Gaussian, tile) at entry_slot().
//   B'     error_sum_kernel: fold_slot_run() over each Gaussian's run of floats.
// The walk, the network, the merge order and the fold order are those of the blend statistics (render_contrib.hip), so a map of
// ones gives weight_sum's bits.
// Also here: error_map_l1_kernel (the usual map: mean absolute colour difference per pixel) and error_accumulate_kernel (one
// view's row into model-sized max / sum accumulators).
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

namespace {

// w * e with a rounding of its own: the product must not be contracted into the first add of the reduction network
__device__ __forceinline__ float mul_rounded(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}

} // namespace

// ---- stage A'
// The plane per (wave, entry) is 4 bytes instead of render_contrib's 8: 26,048 B of LDS = 21 granules, six workgroups per CU
// instead of five, i.e. six waves per SIMD (at most 80 VGPRs).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6)))
render_error_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                    const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                    const float4* __restrict__ splat, const uint32_t* __restrict__ block_base,
                    const float* __restrict__ pixel_map, float* __restrict__ slots, uint8_t* __restrict__ touched,
                    const uint32_t* __restrict__ sort_err)
{
    if (block_has_no_tile(blockIdx.x, T)) return;
    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing (stage B' writes NaN rows)
    if (*sort_err != 0u) return;
    __shared__ ReplayStage st;
    __shared__ float s_stat[4][BATCH];               // [wave][batch entry] sum of w e over the wave's 64 pixels
    __shared__ uint8_t s_hits[4][BATCH];             // ... and whether any of them blended it
    static_assert(sizeof(st) + sizeof(s_stat) + sizeof(s_hits) <= 21 * 1280,
                  "render_error: more than 21 LDS granules = five workgroups per CU instead of six");

    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, false, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;
    const float ev = t.inside ? pixel_map[t.pix] : 0.f;         // the pixel's map value, read once

    float Tr = 1.0f;
    const int beta = candidate_of_lane(lane);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u, slot_next = 0u;
    auto gather = [&](int pos) {                                // compact entry `pos` of the tile -> this thread's staging registers
        qm = 0u;
        if (pos < t.used) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
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
        for (int w = 0; w < 4; w++) { s_stat[w][tid] = 0.f; s_hits[w][tid] = 0; }
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        const int jend = t.wave_last - r * BATCH;
        if (jend > 0) {
            const int nw = build_candidate_list(st, buf, wave, lane,
                                                [&](unsigned long long m, int c) { return keep_in_front(m, jend - c * 64); });
            const int thr = front_cut(buf, t.last - r * BATCH);
            for (int k = 0; k < nw; k += 8) {
                uint32_t e[8];
                load_row(st, wave, k, e);
                const uint32_t my_off = st.list[wave][k + beta];  // the candidate this lane reports on
                float we[8];
                uint32_t my_hit = 0u;
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const StagedRecord s = staged_record(st, e[g]);
                    float dx, dy, G, alpha;
                    const bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                    const bool blend = hit && ((int)e[g] < thr);
                    const float w = blend ? alpha * Tr : 0.f;
                    we[g] = mul_rounded(w, ev);
                    Tr = blend ? Tr * (1.f - alpha) : Tr;
                    const uint32_t h = __ballot(blend) != 0ull ? 1u : 0u;
                    my_hit = (beta == g) ? h : my_hit;
                }
                const float sum = reduce_row_of_8(we, lane, OpAdd());
                // each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane
                const int myj = batch_entry_of(my_off, buf);
                if (lane < 8 && myj < BATCH) { s_stat[wave][myj] = sum; s_hits[wave][myj] = (uint8_t)my_hit; }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves in wave order 0..3; a slot is written iff some pixel of the tile
        // blended the entry (the condition of the blend statistics: the two passes touch the same slots)
        if (r * BATCH + tid < t.used) {
            const uint32_t h = (uint32_t)s_hits[0][tid] | s_hits[1][tid] | s_hits[2][tid] | s_hits[3][tid];
            if (h) {
                const float q0 = s_stat[0][tid], q1 = s_stat[1][tid], q2 = s_stat[2][tid], q3 = s_stat[3][tid];
                slots[slot] = ((q0 + q1) + q2) + q3;
                touched[slot] = 1;
            }
        }
    }
}

// ---- stage B': one lane per Gaussian folds the touched slots of its run (replay.hpp), one float per slot
__global__ void __launch_bounds__(256)
error_sum_kernel(int P, const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base,
                 const float* __restrict__ slots, const uint8_t* __restrict__ touched, float* __restrict__ out_sum,
                 const uint32_t* __restrict__ sort_err)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    float sum = 0.f;
    if (*sort_err != 0u) {
        sum = __uint_as_float(0x7fc00000u);
    } else {
        SlotRun run = { 0u, 0u };
        if (i < P) run = slot_run(i, inst_offset, block_base);
        sum = fold_slot_run(run, slots, touched, lane);
    }
    if (i >= P) return;
    out_sum[i] = sum;
}

// ---- a view's row into model-sized accumulators (view_row() says which row)
__global__ void __launch_bounds__(256)
error_accumulate_kernel(int P_model, int P_rows, const uint8_t* __restrict__ visible, const int32_t* __restrict__ rank,
                        const float* __restrict__ err_sum, float* __restrict__ acc_max, float* __restrict__ acc_sum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P_model) return;
    const int row = view_row(i, visible, rank, P_rows);
    if (row < 0) return;
    const float e = err_sum[row];
    acc_max[i] = max_keeping_nan(acc_max[i], e);
    acc_sum[i] += e;
}

// ---- the usual map: out[p] = (|img[0][p] - gt[0][p]| + ... + |img[C-1][p] - gt[C-1][p]|) / (float)C, channels added in
// ascending order, a true division. The planes and the map are contiguous, so a lane takes four consecutive pixels of the
// flattened image: 16-byte loads and one 16-byte store where the four addresses of the group are 16-byte aligned in every plane
// (always, for an aligned base and H W a multiple of 4), scalar access otherwise and at the ragged end. HBM-bound.
__global__ void __launch_bounds__(256)
error_map_l1_kernel(int C, long long N, const float* __restrict__ img, const float* __restrict__ gt, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const long long p = 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (p >= N) return;
    const float fc = (float)C;
    // every plane starts N floats behind the one before: all planes of both images are aligned alike iff N % 4 == 0 (or C == 1)
    const bool vec = p + 4 <= N && (C == 1 || (N & 3) == 0) &&
                     ((((uintptr_t)(img + p)) | ((uintptr_t)(gt + p)) | ((uintptr_t)(out + p))) & 15u) == 0;
    if (vec) {
        float4 acc = make_float4(0, 0, 0, 0);
        for (int c = 0; c < C; c++) {
            const float4 a = *reinterpret_cast<const float4*>(img + (size_t)c * N + p);
            const float4 b = *reinterpret_cast<const float4*>(gt + (size_t)c * N + p);
            const float4 d = make_float4(fabsf(a.x - b.x), fabsf(a.y - b.y), fabsf(a.z - b.z), fabsf(a.w - b.w));
            acc = c == 0 ? d : make_float4(acc.x + d.x, acc.y + d.y, acc.z + d.z, acc.w + d.w);
        }
        *reinterpret_cast<float4*>(out + p) = make_float4(acc.x / fc, acc.y / fc, acc.z / fc, acc.w / fc);
    } else {
        const long long pe = p + 4 < N ? p + 4 : N;
        for (long long q = p; q < pe; q++) {
            float acc = 0.f;
            for (int c = 0; c < C; c++) {
                const float d = fabsf(img[(size_t)c * N + q] - gt[(size_t)c * N + q]);
                acc = c == 0 ? d : acc + d;
            }
            out[q] = acc / fc;
        }
    }
}

void launch_render_error(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const ErrorPtrs& w,
                         const float* pixel_map, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_error_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm,
                                                       g.splat, g.block_base, pixel_map, w.slots, w.touched, sort_err);
}

void launch_error_sum(int P, const GeomPtrs& g, const ErrorPtrs& w, float* out_sum, const uint32_t* sort_err, hipStream_t s)
{
    error_sum_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, g.inst_offset, g.block_base, w.slots, w.touched, out_sum, sort_err);
}

void launch_error_accumulate(int P_model, int P_rows, const uint8_t* visible, const int32_t* rank, const float* err_sum,
                             float* acc_max, float* acc_sum, hipStream_t s)
{
    error_accumulate_kernel<<<(P_model + 255) / 256, 256, 0, s>>>(P_model, P_rows, visible, rank, err_sum, acc_max, acc_sum);
}

void launch_error_map_l1(int C, int H, int W, const float* img, const float* gt, float* out, hipStream_t s)
{
    const long long N = (long long)H * W, groups = (N + 3) / 4;
    error_map_l1_kernel<<<(unsigned)((groups + 255) / 256), 256, 0, s>>>(C, N, img, gt, out);
}

} // namespace c3dgs
