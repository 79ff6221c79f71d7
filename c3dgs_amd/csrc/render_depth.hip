// render_depth.hip -- depth, accumulated opacity and median depth of a finished forward, for gfx950. Forward-only; the
// reference's rasterizer has no counterpart.
//
// Per pixel, over the entries k = 1..m the forward blended, with w_k = alpha_k T_k, T_{k+1} = T_k (1 - alpha_k), T_1 = 1 and
// z_k = the fp32 view-space depth preprocess stored for the Gaussian (the bits in depth_keys[id]):
//     depth  = sum_k w_k z_k      accumulated like a colour channel of the forward (fmaf in list order, from 0); not normalised
//     alpha  = 1 - T_{m+1}        from this kernel's own replayed T
//     median = z_k of the first blended entry with T_{k+1} < 0.5, or 0
//
// The kernel REPLAYS the forward, it decides nothing again: it walks the tile's compact list (cid / cqm: the entries that can
// reach the tile, in list order) up to tile_used_c[tile], and a pixel only takes entries whose compact index is <=
// n_contrib_c[pix] -- the forward's own early stop. Inside that prefix the hit test is the forward's gaussian_alpha() on the
// same pre-scaled conic, so the same bits give the same decisions, the same T and the same weights. Positions past
// tile_used_c are never read (the compact list is only written that far).
//
// Structure = render_forward_kernel's: one 16x16 tile per 256-thread workgroup, one 8x8 quadrant per wave, batches of 256
// entries staged into double-buffered LDS (one barrier per batch, the next batch's gather in flight behind the blend),
// per-wave candidate lists of LDS byte offsets from the cqm ballots. The staged record is 32 bytes
// {x, y, ka, kb | kc, opacity, z, -}: two ds_read_b128 per pair. No atomics, no scratch, no list stores.
#include "common.hpp"
#include "render_common.hpp"

namespace c3dgs {

// seven waves per SIMD (at most 72 VGPRs), the forward's occupancy: left alone, the scheduler hoists the LDS reads of a whole row
// of 8 and takes 90
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7)))
render_depth_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_used_c,
                    const uint32_t* __restrict__ n_contrib_c, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                    const float4* __restrict__ splat, const uint32_t* __restrict__ depth_keys, float* __restrict__ out_depth,
                    float* __restrict__ out_alpha, float* __restrict__ out_median, const uint32_t* __restrict__ sort_err)
{
    const int tile = tile_of_block(blockIdx.x, T);
    if (tile >= T || (blockIdx.x >> 3) >= ((T + 7) >> 3)) return;
    __shared__ float4 s_ab[2][BATCH + 1][2];          // entry BATCH of each buffer: sentinel with opacity 0 (blends nothing)
    __shared__ uint32_t s_list[4][BATCH + 8];        // per wave: its candidates of the batch, padded to a multiple of 8
    __shared__ unsigned long long s_mask[2][4][4];   // [buf][quadrant][staging wave]
    static_assert(sizeof(s_ab) + sizeof(s_list) + sizeof(s_mask) <= 18 * 1280,
                  "render_depth: more than 18 LDS granules = six workgroups per CU instead of seven");
    constexpr uint32_t REC_BYTES = 32, BUF_BYTES = (BATCH + 1) * REC_BYTES;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx = tile % gx, ty = tile / gx;
    const int px = tx * TILE + (wave & 1) * 8 + (lane & 7);
    const int py = ty * TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const size_t pix = (size_t)W * py + px;
    if (tid < 2) { s_ab[tid][BATCH][0] = make_float4(0, 0, 0, 0); s_ab[tid][BATCH][1] = make_float4(0, 0, 0, 0); }

    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing, every output is NaN
    const bool poisoned = *sort_err != 0u;
    const uint2 range = poisoned ? make_uint2(0u, 0u) : ranges[tile];
    const int n = (int)(range.y - range.x);
    const int used = poisoned ? 0 : min(n, (int)tile_used_c[tile]);       // compact entries the forward wrote and some pixel blended
    const int rounds = (used + BATCH - 1) / BATCH;

    // 1-based compact index of the pixel's last blended entry = how far this pixel walks; per wave the deepest of its 64
    const int last = (inside && !poisoned) ? min((int)n_contrib_c[pix], used) : 0;
    int wave_last = last;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wave_last = max(wave_last, __shfl_xor(wave_last, o));
    wave_last = __builtin_amdgcn_readfirstlane(wave_last);

    float Tr = 1.0f, D = 0.f, med = 0.f;
    const char* rec_base = reinterpret_cast<const char*>(&s_ab[0][0][0]);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    uint32_t qm = 0u;
    auto gather = [&](int pos) {                                // compact entry `pos` of the tile -> this thread's staging registers
        qm = 0u;
        if (pos < used) {
            const uint32_t id = cid[range.x + pos];
            qm = cqm[range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            rb.z = __uint_as_float(depth_keys[id]);             // in place of the record's red
        }
    };
    gather(tid);
    for (int r = 0; r < rounds; r++) {
        const int buf = r & 1;
        prescale_conic(ra, rb);
        s_ab[buf][tid][0] = ra; s_ab[buf][tid][1] = rb;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned long long bm = __ballot((qm >> q) & 1u);
            if (lane == 0) s_mask[buf][q][wave] = bm;
        }
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        // entry j of the batch has compact index r * BATCH + j + 1: nothing at or behind j = wave_last - r * BATCH matters to this wave
        const int jend = wave_last - r * BATCH;
        if (jend <= 0) continue;
        int nw = 0;
        {
            const unsigned long long lt = (1ull << lane) - 1ull;
            const uint32_t buf_off = (uint32_t)buf * BUF_BYTES;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                unsigned long long m = uniform_u64(s_mask[buf][wave][c]);
                const int jn = jend - c * 64;                   // entries of this staging wave in front of the cut
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
        const int thr = (int)((uint32_t)buf * BUF_BYTES) + min(max(last - r * BATCH, 0), BATCH) * (int)REC_BYTES;
        for (int k = 0; k < nw; k += 8) {
            const uint4 row0 = *reinterpret_cast<const uint4*>(&s_list[wave][k]);
            const uint4 row1 = *reinterpret_cast<const uint4*>(&s_list[wave][k + 4]);
            const uint32_t e[8] = { row0.x, row0.y, row0.z, row0.w, row1.x, row1.y, row1.z, row1.w };
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const float4 a = *reinterpret_cast<const float4*>(rec_base + e[g]);
                const float4 b = *reinterpret_cast<const float4*>(rec_base + e[g] + 16);
                float dx, dy, G, alpha;
                const bool hit = gaussian_alpha(a.x, a.y, a.z, a.w, b.x, b.y, pxf, pyf, dx, dy, G, alpha);
                // in front of the pixel's last contributor every hit was blended by the forward (its stop lies behind it)
                const bool blend = hit && ((int)e[g] < thr);
                const float test_T = Tr * (1.f - alpha);
                const float w = blend ? alpha * Tr : 0.f;
                D = fmaf(b.z, w, D);
                // T only falls: the first entry that takes it below 0.5 is the one that finds it at or above
                med = (blend && test_T < 0.5f && !(Tr < 0.5f)) ? b.z : med;
                Tr = blend ? test_T : Tr;
            }
        }
    }
    if (inside) {
        const float poison = poisoned ? __uint_as_float(0x7fc00000u) : 0.f;
        if (out_depth) out_depth[pix] = D + poison;
        if (out_alpha) out_alpha[pix] = (1.0f - Tr) + poison;
        if (out_median) out_median[pix] = med + poison;
    }
}

void launch_render_depth(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const uint32_t* depth_keys,
                         float* out_depth, float* out_alpha, float* out_median, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    const int grid = ((T + 7) / 8) * 8;
    render_depth_kernel<<<grid, 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, cl.cid, cl.cqm, splat,
                                             depth_keys, out_depth, out_alpha, out_median, sort_err);
}

} // namespace c3dgs
