// render_error.hip -- per-Gaussian error scores of a finished forward, for gfx950. Forward-only; the reference's rasterizer has
// no counterpart.
//
// For every Gaussian g, over the (pixel, entry) pairs the forward BLENDED, with w = alpha * T in fp32 exactly as
// render_contrib_kernel forms it and e = pixel_map[pixel]:
//     err_sum[g] = sum fl(w * e)
// the score of error-based densification ("Revising Densification in Gaussian Splatting": E_g = sum over pixels of w_g e).
//
// Three launches, no float atomics, bitwise reproducible:
//   clear  the `touched` bytes of the workspace (backward_prep_kernel's fill workgroups: launch_backward_prep with no tiles)
//   A'     render_error_kernel: render_contrib_kernel's replay with another statistic. Same tiling, banding, batches, candidate
//          lists, cuts, shared alpha expression, slot formation: it decides nothing again. A pixel reads its map value once; per
//          pair the weight is multiplied by it (its own rounding, never fused), ONE add network per row of 8 candidates, the
//          four waves merged in wave order 0..3, one plain 4-byte store + a flag byte per (Gaussian, tile).
//   B'     error_sum_kernel: contrib_sum_kernel's fold of the touched slots of a run in slot order (the whole wave a long run).
// The network (render_common.hpp), the merge order and the fold order are render_contrib.hip's, so a map of ones gives
// weight_sum's bits.
// Also here: error_map_l1_kernel (the usual map: mean absolute colour difference per pixel) and error_accumulate_kernel (one
// view's row into model-sized max / sum accumulators).
#include "common.hpp"
#include "render_common.hpp"

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
    const int tile = tile_of_block(blockIdx.x, T);
    if (tile >= T || (blockIdx.x >> 3) >= ((T + 7) >> 3)) return;
    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing (stage B' writes NaN rows)
    if (*sort_err != 0u) return;
    __shared__ float4 s_ab[2][BATCH + 1][2];          // entry BATCH of each buffer: sentinel with opacity 0 (blends nothing)
    __shared__ uint32_t s_list[4][BATCH + 8];        // per wave: its candidates of the batch, padded to a multiple of 8
    __shared__ unsigned long long s_mask[2][4][4];   // [buf][quadrant][staging wave]
    __shared__ float s_stat[4][BATCH];               // [wave][batch entry] sum of w e over the wave's 64 pixels
    __shared__ uint8_t s_hits[4][BATCH];             // ... and whether any of them blended it
    static_assert(sizeof(s_ab) + sizeof(s_list) + sizeof(s_mask) + sizeof(s_stat) + sizeof(s_hits) <= 21 * 1280,
                  "render_error: more than 21 LDS granules = five workgroups per CU instead of six");
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
    const float ev = inside ? pixel_map[pix] : 0.f;             // the pixel's map value, read once
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
        // its entry's words of the previous batch behind that batch's second barrier, so it may clear them here.
#pragma unroll
        for (int w = 0; w < 4; w++) { s_stat[w][tid] = 0.f; s_hits[w][tid] = 0; }
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
                float we[8];
                uint32_t my_hit = 0u;
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const float4 a = *reinterpret_cast<const float4*>(rec_base + e[g]);
                    const float4 b = *reinterpret_cast<const float4*>(rec_base + e[g] + 16);
                    float dx, dy, G, alpha;
                    const bool hit = gaussian_alpha(a.x, a.y, a.z, a.w, b.x, b.y, pxf, pyf, dx, dy, G, alpha);
                    // in front of the pixel's last contributor every hit was blended by the forward (its stop lies behind it)
                    const bool blend = hit && ((int)e[g] < thr);
                    const float w = blend ? alpha * Tr : 0.f;
                    we[g] = mul_rounded(w, ev);
                    Tr = blend ? Tr * (1.f - alpha) : Tr;
                    const uint32_t h = __ballot(blend) != 0ull ? 1u : 0u;
                    my_hit = (beta == g) ? h : my_hit;
                }
                const float sum = reduce_row_of_8(we, lane, OpAdd());
                // lanes 0..7 hold the row's 8 candidates (beta is a permutation of them); the row's padding is the sentinel.
                // Each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane.
                const int myj = (int)((my_off - buf_off) / REC_BYTES);
                if (lane < 8 && myj < BATCH) { s_stat[wave][myj] = sum; s_hits[wave][myj] = (uint8_t)my_hit; }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves in wave order 0..3; a slot is written iff some pixel of the tile
        // blended the entry (render_contrib's condition: the two passes touch the same slots)
        if (r * BATCH + tid < used) {
            const uint32_t h = (uint32_t)s_hits[0][tid] | s_hits[1][tid] | s_hits[2][tid] | s_hits[3][tid];
            if (h) {
                const float q0 = s_stat[0][tid], q1 = s_stat[1][tid], q2 = s_stat[2][tid], q3 = s_stat[3][tid];
                slots[slot] = ((q0 + q1) + q2) + q3;
                touched[slot] = 1;
            }
        }
    }
}

// ---- stage B': contrib_sum_kernel's fold with one float per slot: the same lane -> slot assignment, four strides per trip and
// xor butterfly order, so that equal slot values give equal bits.
constexpr uint32_t ERROR_LONG_RUN = 64;                         // = CONTRIB_LONG_RUN of render_contrib.hip
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
        uint32_t start = 0u, end = 0u;
        if (i < P) {
            end = inst_offset[i] + block_base[i >> 8];
            start = (i == 0) ? 0u : inst_offset[i - 1] + block_base[(i - 1) >> 8];
        }
        const bool long_run = end - start > ERROR_LONG_RUN;
        if (!long_run)
            for (uint32_t s = start; s < end; s++) {
                if (!touched[s]) continue;
                sum += slots[s];
            }
        for (unsigned long long m = __ballot(long_run); m; m &= m - 1ull) {
            const int src = (int)__ffsll((long long)m) - 1;
            const uint32_t s0 = __shfl(start, src), s1 = __shfl(end, src);
            float ps = 0.f;
            // four strides per trip: the four flag bytes are requested together, then the values of the written ones
            for (uint32_t s = s0 + (uint32_t)lane; s < s1; s += 256) {
                uint8_t f[4];
#pragma unroll
                for (int k = 0; k < 4; k++) f[k] = (s + 64u * k < s1) ? touched[s + 64u * k] : (uint8_t)0;
                float c[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    c[k] = 0.f;
                    if (f[k]) c[k] = slots[s + 64u * k];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) ps += c[k];         // ascending slots; an unwritten one adds +0
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o);
            if (lane == src) sum = ps;
        }
    }
    if (i >= P) return;
    out_sum[i] = sum;
}

// ---- a view's row into model-sized accumulators. Model row i reads view row rank[i] if visible[i] (the pair
// c3dgs_qat_visible produces), or row i when both are null.
__global__ void __launch_bounds__(256)
error_accumulate_kernel(int P_model, int P_rows, const uint8_t* __restrict__ visible, const int32_t* __restrict__ rank,
                        const float* __restrict__ err_sum, float* __restrict__ acc_max, float* __restrict__ acc_sum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P_model) return;
    int row = i;
    if (visible) row = visible[i] ? rank[i] : -1;
    if (row < 0 || row >= P_rows) return;
    const float e = err_sum[row];
    const float a = acc_max[i];
    acc_max[i] = (e != e) ? e : fmaxf(a, e);                    // fmaxf drops a NaN operand: a timed-out view must show
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
    const int grid = ((T + 7) / 8) * 8;
    render_error_kernel<<<grid, 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm, g.splat,
                                             g.block_base, pixel_map, w.slots, w.touched, sort_err);
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
