// render_contrib.hip -- per-Gaussian blend statistics of a finished forward, for gfx950. Forward-only; the reference's
// rasterizer has no counterpart.
//
// For every Gaussian g, over the (pixel, entry) pairs the forward BLENDED (a hit that passed the T test; the entry that only
// stopped a pixel is not one), with w = alpha * T in fp32:
//     weight_sum[g] = sum w        weight_max[g] = max w        hits[g] = number of such pairs
//
// Three launches, no float atomics, bitwise reproducible:
//   clear  the `touched` bytes of the workspace (backward_prep_kernel's fill workgroups: launch_backward_prep with no tiles)
//   A      render_contrib_kernel: a replay of the forward (replay.hpp: the tile walk, the staging and the candidate lists), front
//          to back. Per row of 8 candidates a wave reduces the 8 weights over its 64 pixels with the transposing butterfly of
//          render_common.hpp, once for the sum and once for the max (7 + 3 operations each instead of 8 x 6), the four waves'
//          results for a batch entry meet in LDS, and one thread per entry merges them in wave order 0..3 and writes
//          {sum, max, hits} + a flag byte with plain stores to the entry's slot (entry_slot(): the backward's slot numbering).
//   B      contrib_sum_kernel: fold_slot_run() over each Gaussian's run of {sum, max, hits} records.
// and c3dgs_contrib_accumulate's kernel, which folds a view's three rows into model-sized accumulators.
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

// ---- stage A
// five waves per SIMD (at most 102 VGPRs): what the kernel's 31 KB of LDS allow anyway (five workgroups per CU)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5)))
render_contrib_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                      const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                      const float4* __restrict__ splat, const uint32_t* __restrict__ block_base, ContribSlot* __restrict__ slots,
                      uint8_t* __restrict__ touched, const uint32_t* __restrict__ sort_err)
{
    if (block_has_no_tile(blockIdx.x, T)) return;
    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing (stage B writes NaN rows)
    if (*sort_err != 0u) return;
    __shared__ ReplayStage st;
    __shared__ float2 s_stat[4][BATCH];              // [wave][batch entry] {sum, max} over the wave's 64 pixels
    __shared__ uint8_t s_hits[4][BATCH];             // ... and how many of them blended it (<= 64)
    static_assert(sizeof(st) + sizeof(s_stat) + sizeof(s_hits) <= 25 * 1280,
                  "render_contrib: more than 25 LDS granules = four workgroups per CU instead of five");

    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, false, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;

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
        // its entry's four words of the previous batch behind that batch's second barrier, so it may clear them here.
#pragma unroll
        for (int w = 0; w < 4; w++) { s_stat[w][tid] = make_float2(0.f, 0.f); s_hits[w][tid] = 0; }
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
                float ws[8], wm[8];
                uint32_t my_hits = 0u;
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const StagedRecord s = staged_record(st, e[g]);
                    float dx, dy, G, alpha;
                    const bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                    const bool blend = hit && ((int)e[g] < thr);
                    const float w = blend ? alpha * Tr : 0.f;
                    ws[g] = w; wm[g] = w;
                    Tr = blend ? Tr * (1.f - alpha) : Tr;
                    const uint32_t h = (uint32_t)__popcll(__ballot(blend));
                    my_hits = (beta == g) ? h : my_hits;
                }
                const float sum = reduce_row_of_8(ws, lane, OpAdd());
                const float mx = reduce_row_of_8(wm, lane, OpMax());
                // each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane
                const int myj = batch_entry_of(my_off, buf);
                if (lane < 8 && myj < BATCH) { s_stat[wave][myj] = make_float2(sum, mx); s_hits[wave][myj] = (uint8_t)my_hits; }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves in wave order 0..3
        if (r * BATCH + tid < t.used) {
            const uint32_t h = (uint32_t)s_hits[0][tid] + s_hits[1][tid] + s_hits[2][tid] + s_hits[3][tid];
            if (h) {
                const float2 q0 = s_stat[0][tid], q1 = s_stat[1][tid], q2 = s_stat[2][tid], q3 = s_stat[3][tid];
                ContribSlot o;
                o.sum = ((q0.x + q1.x) + q2.x) + q3.x;
                o.max = fmaxf(fmaxf(fmaxf(q0.y, q1.y), q2.y), q3.y);
                o.hits = h;
                slots[slot] = o;
                touched[slot] = 1;
            }
        }
    }
}

// ---- stage B: one lane per Gaussian folds the touched slots of its run (replay.hpp). What a slot holds and how two of them add:
// an unwritten one adds +0, max 0, 0 hits
__device__ __forceinline__ void fold_zero(ContribSlot& v) { v.sum = 0.f; v.max = 0.f; v.hits = 0u; }
__device__ __forceinline__ void fold_add(ContribSlot& acc, const ContribSlot& v)
{
    acc.sum += v.sum;
    acc.max = fmaxf(acc.max, v.max);
    acc.hits += v.hits;
}
__device__ __forceinline__ ContribSlot fold_shfl_xor(const ContribSlot& v, int o)
{
    ContribSlot p;
    p.sum = __shfl_xor(v.sum, o); p.max = __shfl_xor(v.max, o); p.hits = __shfl_xor(v.hits, o);
    return p;
}

__global__ void __launch_bounds__(256)
contrib_sum_kernel(int P, const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base,
                   const ContribSlot* __restrict__ slots, const uint8_t* __restrict__ touched, float* __restrict__ out_sum,
                   float* __restrict__ out_max, uint32_t* __restrict__ out_hits, const uint32_t* __restrict__ sort_err)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    ContribSlot acc;
    fold_zero(acc);
    if (*sort_err != 0u) {
        acc.sum = acc.max = __uint_as_float(0x7fc00000u);
    } else {
        SlotRun run = { 0u, 0u };
        if (i < P) run = slot_run(i, inst_offset, block_base);
        acc = fold_slot_run(run, slots, touched, lane);
    }
    if (i >= P) return;
    if (out_sum) out_sum[i] = acc.sum;
    if (out_max) out_max[i] = acc.max;
    if (out_hits) out_hits[i] = acc.hits;
}

// ---- stage C: a view's rows into model-sized accumulators (view_row() says which row)
__global__ void __launch_bounds__(256)
contrib_accumulate_kernel(int P_model, int P_rows, const uint8_t* __restrict__ visible, const int32_t* __restrict__ rank,
                          const float* __restrict__ weight_sum, const float* __restrict__ weight_max,
                          const uint32_t* __restrict__ hits, float* __restrict__ acc_sum, float* __restrict__ acc_max,
                          long long* __restrict__ acc_hits, uint32_t* __restrict__ acc_views)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P_model) return;
    const int row = view_row(i, visible, rank, P_rows);
    if (row < 0) return;
    const float s = weight_sum[row], m = weight_max[row];
    const uint32_t h = hits[row];
    acc_sum[i] += s;
    acc_max[i] = max_keeping_nan(acc_max[i], m);
    acc_hits[i] += (long long)h;
    acc_views[i] += h > 0u ? 1u : 0u;
}

void launch_render_contrib(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const ContribPtrs& w,
                           const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    render_contrib_kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm,
                                                         g.splat, g.block_base, w.slots, w.touched, sort_err);
}

void launch_contrib_sum(int P, const GeomPtrs& g, const ContribPtrs& w, float* out_sum, float* out_max, uint32_t* out_hits,
                        const uint32_t* sort_err, hipStream_t s)
{
    contrib_sum_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, g.inst_offset, g.block_base, w.slots, w.touched, out_sum, out_max, out_hits,
                                                       sort_err);
}

void launch_contrib_accumulate(int P_model, int P_rows, const uint8_t* visible, const int32_t* rank, const float* weight_sum,
                               const float* weight_max, const uint32_t* hits, float* acc_sum, float* acc_max, int64_t* acc_hits,
                               uint32_t* acc_views, hipStream_t s)
{
    contrib_accumulate_kernel<<<(P_model + 255) / 256, 256, 0, s>>>(P_model, P_rows, visible, rank, weight_sum, weight_max, hits,
                                                                    acc_sum, acc_max, (long long*)acc_hits, acc_views);
}

} // namespace c3dgs
