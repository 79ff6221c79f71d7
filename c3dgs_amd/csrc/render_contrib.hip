// render_contrib.hip -- per-Gaussian blend statistics of a finished forward, for gfx950. Forward-only; the reference's
// rasterizer has no counterpart.
//
// For every Gaussian g, over the (pixel, entry) pairs the forward BLENDED (a hit that passed the T test; the entry that only
// stopped a pixel is not one), with w = alpha * T in fp32 exactly as render_depth_kernel forms it:
//     weight_sum[g] = sum w        weight_max[g] = max w        hits[g] = number of such pairs
//
// Three launches, no float atomics, bitwise reproducible:
//   clear  the `touched` bytes of the workspace (backward_prep_kernel's fill workgroups: launch_backward_prep with no tiles)
//   A      render_contrib_kernel: render_depth_kernel's replay of the blend (same structure, same shared alpha expression, same
//          cuts: it decides nothing again). Per row of 8 candidates a wave reduces the 8 weights over its 64 pixels with a
//          transposing butterfly, once for the sum and once for the max (7 + 3 operations each instead of 8 x 6), the four
//          waves' results for a batch entry meet in LDS, and one thread per entry merges them in wave order 0..3 and writes
//          {sum, max, hits} + a flag byte with plain stores to the entry's slot: the backward's slot layout,
//          block_base[id >> 8] + the record's first slot + the tile's offset inside the Gaussian's rectangle.
//   B      contrib_sum_kernel: one lane per Gaussian folds the touched slots of its run in slot order (the whole wave a long run).
// and c3dgs_contrib_accumulate's kernel, which folds a view's three rows into model-sized accumulators.
#include "common.hpp"
#include "render_common.hpp"

namespace c3dgs {

// ---- stage A
// five waves per SIMD (at most 102 VGPRs): what the kernel's 31 KB of LDS allow anyway (five workgroups per CU)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5)))
render_contrib_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                      const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                      const float4* __restrict__ splat, const uint32_t* __restrict__ block_base, ContribSlot* __restrict__ slots,
                      uint8_t* __restrict__ touched, const uint32_t* __restrict__ sort_err)
{
    const int tile = tile_of_block(blockIdx.x, T);
    if (tile >= T || (blockIdx.x >> 3) >= ((T + 7) >> 3)) return;
    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing (stage B writes NaN rows)
    if (*sort_err != 0u) return;
    __shared__ float4 s_ab[2][BATCH + 1][2];          // entry BATCH of each buffer: sentinel with opacity 0 (blends nothing)
    __shared__ uint32_t s_list[4][BATCH + 8];        // per wave: its candidates of the batch, padded to a multiple of 8
    __shared__ unsigned long long s_mask[2][4][4];   // [buf][quadrant][staging wave]
    __shared__ float2 s_stat[4][BATCH];              // [wave][batch entry] {sum, max} over the wave's 64 pixels
    __shared__ uint8_t s_hits[4][BATCH];             // ... and how many of them blended it (<= 64)
    static_assert(sizeof(s_ab) + sizeof(s_list) + sizeof(s_mask) + sizeof(s_stat) + sizeof(s_hits) <= 25 * 1280,
                  "render_contrib: more than 25 LDS granules = four workgroups per CU instead of five");
    constexpr uint32_t REC_BYTES = 32, BUF_BYTES = (BATCH + 1) * REC_BYTES;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx = tile % gx, ty = tile / gx;
    const int px = tx * TILE + (wave & 1) * 8 + (lane & 7);
    const int py = ty * TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const size_t pix = (size_t)W * py + px;
    if (tid < 2) { s_ab[tid][BATCH][0] = make_float4(0, 0, 0, 0); s_ab[tid][BATCH][1] = make_float4(0, 0, 0, 0); }

    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    const int used = min(n, (int)tile_used_c[tile]);            // compact entries the forward wrote and some pixel blended
    const int rounds = (used + BATCH - 1) / BATCH;

    // 1-based compact index of the pixel's last blended entry = how far this pixel walks; per wave the deepest of its 64
    const int last = inside ? min((int)n_contrib_c[pix], used) : 0;
    int wave_last = last;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wave_last = max(wave_last, __shfl_xor(wave_last, o));
    wave_last = __builtin_amdgcn_readfirstlane(wave_last);

    float Tr = 1.0f;
    const char* rec_base = reinterpret_cast<const char*>(&s_ab[0][0][0]);
    // where this lane's reduced values belong: candidate beta of the row
    const int beta = ((lane >> 2) & 1) * 4 + (lane & 1) * 2 + ((lane >> 1) & 1);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u, slot_next = 0u;
    auto gather = [&](int pos) {                                // compact entry `pos` of the tile -> this thread's staging registers
        qm = 0u;
        if (pos < used) {
            const uint32_t id = cid[range.x + pos];
            qm = cqm[range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            // the entry's slot, as render_backward forms it: first slot of the Gaussian + the tile's place in its rectangle
            const float4 c = splat[3 * (size_t)id + 2];
            const uint32_t off = __float_as_uint(c.y), lo = __float_as_uint(c.z), hi = __float_as_uint(c.w);
            const int x0 = lo & 0xffff, y0 = lo >> 16, x1 = hi & 0xffff;
            slot_next = block_base[id >> 8] + off + (uint32_t)((ty - y0) * (x1 - x0) + (tx - x0));
        }
    };
    gather(tid);
    for (int r = 0; r < rounds; r++) {
        const int buf = r & 1;
        const uint32_t slot = slot_next;                        // of batch entry `tid`, which this thread stages and later merges
        prescale_conic(ra, rb);
        s_ab[buf][tid][0] = ra; s_ab[buf][tid][1] = rb;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned long long bm = __ballot((qm >> q) & 1u);
            if (lane == 0) s_mask[buf][q][wave] = bm;
        }
        // a wave only writes the entries of its own candidate list: the others read as "nothing blended". This thread read
        // its entry's four words of the previous batch behind that batch's second barrier, so it may clear them here.
#pragma unroll
        for (int w = 0; w < 4; w++) { s_stat[w][tid] = make_float2(0.f, 0.f); s_hits[w][tid] = 0; }
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        // entry j of the batch has compact index r * BATCH + j + 1: nothing at or behind j = wave_last - r * BATCH matters to this wave
        const int jend = wave_last - r * BATCH;
        if (jend > 0) {
            int nw = 0;
            const uint32_t buf_off = (uint32_t)buf * BUF_BYTES;
            {
                const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    unsigned long long m = uniform_u64(s_mask[buf][wave][c]);
                    const int jn = jend - c * 64;               // entries of this staging wave in front of the cut
                    if (jn <= 0) m = 0; else if (jn < 64) m &= (1ull << jn) - 1ull;
                    if ((m >> lane) & 1ull) s_list[wave][nw + (int)__popcll(m & lt)] = buf_off + (uint32_t)(c * 64 + lane) * REC_BYTES;
                    nw += (int)__popcll(m);
                }
                if (lane < 8) s_list[wave][nw + lane] = buf_off + (uint32_t)BATCH * REC_BYTES;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            // a pixel takes entry j only if r * BATCH + j + 1 <= last, i.e. record offset < thr (the sentinel's never is)
            const int thr = (int)buf_off + min(max(last - r * BATCH, 0), BATCH) * (int)REC_BYTES;
            for (int k = 0; k < nw; k += 8) {
                const uint4 row0 = *reinterpret_cast<const uint4*>(&s_list[wave][k]);
                const uint4 row1 = *reinterpret_cast<const uint4*>(&s_list[wave][k + 4]);
                const uint32_t e[8] = { row0.x, row0.y, row0.z, row0.w, row1.x, row1.y, row1.z, row1.w };
                const uint32_t my_off = s_list[wave][k + beta];  // the candidate this lane reports on
                float ws[8], wm[8];
                uint32_t my_hits = 0u;
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const float4 a = *reinterpret_cast<const float4*>(rec_base + e[g]);
                    const float4 b = *reinterpret_cast<const float4*>(rec_base + e[g] + 16);
                    float dx, dy, G, alpha;
                    const bool hit = gaussian_alpha(a.x, a.y, a.z, a.w, b.x, b.y, pxf, pyf, dx, dy, G, alpha);
                    // in front of the pixel's last contributor every hit was blended by the forward (its stop lies behind it)
                    const bool blend = hit && ((int)e[g] < thr);
                    const float w = blend ? alpha * Tr : 0.f;
                    ws[g] = w; wm[g] = w;
                    Tr = blend ? Tr * (1.f - alpha) : Tr;
                    const uint32_t h = (uint32_t)__popcll(__ballot(blend));
                    my_hits = (beta == g) ? h : my_hits;
                }
                const float sum = reduce_row_of_8(ws, lane, OpAdd());
                const float mx = reduce_row_of_8(wm, lane, OpMax());
                // lanes 0..7 hold the row's 8 candidates (beta is a permutation of them); the row's padding is the sentinel.
                // Each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane.
                const int myj = (int)((my_off - buf_off) / REC_BYTES);
                if (lane < 8 && myj < BATCH) { s_stat[wave][myj] = make_float2(sum, mx); s_hits[wave][myj] = (uint8_t)my_hits; }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves in wave order 0..3
        if (r * BATCH + tid < used) {
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

// ---- stage B: one lane per Gaussian folds the touched slots of its run [start, end) in slot order. The run's start comes from
// the id-order scan (inst_offset + block_base, as sum_partials_kernel reads it), its length is the rectangle's area.
// A run longer than CONTRIB_LONG_RUN slots (a splat over hundreds of tiles; with one lane on it the whole wave waits for that
// lane: 1.63 ms on the heavy-tailed scene) is folded by the WHOLE wave instead: lane l takes slots start + l, start + l + 64, ...
// in that order and the 64 partial results meet in an xor butterfly (32, 16, ..., 1). Which lane adds what, and the order of
// the butterfly, follow from the run's start and length alone, so the row is the same bits whoever the neighbours are.
constexpr uint32_t CONTRIB_LONG_RUN = 64;
__global__ void __launch_bounds__(256)
contrib_sum_kernel(int P, const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base,
                   const ContribSlot* __restrict__ slots, const uint8_t* __restrict__ touched, float* __restrict__ out_sum,
                   float* __restrict__ out_max, uint32_t* __restrict__ out_hits, const uint32_t* __restrict__ sort_err)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    float sum = 0.f, mx = 0.f;
    uint32_t hits = 0u;
    if (*sort_err != 0u) {
        sum = mx = __uint_as_float(0x7fc00000u);
    } else {
        uint32_t start = 0u, end = 0u;
        if (i < P) {
            end = inst_offset[i] + block_base[i >> 8];
            start = (i == 0) ? 0u : inst_offset[i - 1] + block_base[(i - 1) >> 8];
        }
        const bool long_run = end - start > CONTRIB_LONG_RUN;
        if (!long_run)
            for (uint32_t s = start; s < end; s++) {
                if (!touched[s]) continue;
                const ContribSlot c = slots[s];
                sum += c.sum;
                mx = fmaxf(mx, c.max);
                hits += c.hits;
            }
        for (unsigned long long m = __ballot(long_run); m; m &= m - 1ull) {
            const int src = (int)__ffsll((long long)m) - 1;
            const uint32_t s0 = __shfl(start, src), s1 = __shfl(end, src);
            float ps = 0.f, pm = 0.f;
            uint32_t ph = 0u;
            // four strides per trip: the four flag bytes are requested together, then the records of the written ones (a
            // trip is two memory round trips whatever it finds; one stride per trip left a 8160-tile run at 128 x 2 of them)
            for (uint32_t s = s0 + (uint32_t)lane; s < s1; s += 256) {
                uint8_t f[4];
#pragma unroll
                for (int k = 0; k < 4; k++) f[k] = (s + 64u * k < s1) ? touched[s + 64u * k] : (uint8_t)0;
                ContribSlot c[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    c[k].sum = 0.f; c[k].max = 0.f; c[k].hits = 0u;
                    if (f[k]) c[k] = slots[s + 64u * k];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {           // ascending slots; an unwritten one adds +0, max 0, 0 hits
                    ps += c[k].sum;
                    pm = fmaxf(pm, c[k].max);
                    ph += c[k].hits;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                ps += __shfl_xor(ps, o);
                pm = fmaxf(pm, __shfl_xor(pm, o));
                ph += __shfl_xor(ph, o);
            }
            if (lane == src) { sum = ps; mx = pm; hits = ph; }
        }
    }
    if (i >= P) return;
    if (out_sum) out_sum[i] = sum;
    if (out_max) out_max[i] = mx;
    if (out_hits) out_hits[i] = hits;
}

// ---- stage C: a view's rows into model-sized accumulators. Model row i reads view row rank[i] if visible[i] (the pair
// c3dgs_qat_visible produces), or row i when both are null.
__global__ void __launch_bounds__(256)
contrib_accumulate_kernel(int P_model, int P_rows, const uint8_t* __restrict__ visible, const int32_t* __restrict__ rank,
                          const float* __restrict__ weight_sum, const float* __restrict__ weight_max,
                          const uint32_t* __restrict__ hits, float* __restrict__ acc_sum, float* __restrict__ acc_max,
                          long long* __restrict__ acc_hits, uint32_t* __restrict__ acc_views)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P_model) return;
    int row = i;
    if (visible) row = visible[i] ? rank[i] : -1;
    if (row < 0 || row >= P_rows) return;
    const float s = weight_sum[row], m = weight_max[row];
    const uint32_t h = hits[row];
    acc_sum[i] += s;
    const float a = acc_max[i];
    acc_max[i] = (m != m) ? m : fmaxf(a, m);                    // fmaxf drops a NaN operand: a timed-out view must show
    acc_hits[i] += (long long)h;
    acc_views[i] += h > 0u ? 1u : 0u;
}

void launch_render_contrib(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const ContribPtrs& w,
                           const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    const int grid = ((T + 7) / 8) * 8;
    render_contrib_kernel<<<grid, 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm, g.splat,
                                               g.block_base, w.slots, w.touched, sort_err);
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
