// render_maps_backward.hip -- gradients through the depth, accumulated-opacity, distortion and normal maps (render_depth.hip,
// render_distortion.hip, render_normal.hip) in ONE blend replay per backward, for gfx950. The reference's rasterizer has no
// counterpart.
//
// Two launches, no float atomics, bitwise reproducible; both honour the sort's time-out word (set: A walks nothing, B writes NaN):
//   A  render_maps_backward_kernel<DIST, NORMAL>, behind render_backward (or behind the flag clear alone, when the loss does not
//      use the image): one recurrence, four instances, picked by which of dL_ddistortion / dL_dnormal the call has. An instance
//      without a map does not carry that map's terms; with contraction off the terms of a map whose gradient is all zero are
//      exact zeros, so the instances agree wherever they can be compared.
//   B  depth_backward_fold_kernel, behind backward_preprocess: one lane per LISTED Gaussian (replay.hpp: listed_gaussian) folds
//      the flagged slots of its run of the dL/dz plane with fold_slot_run() and adds dL/dz x the depth row of the view matrix --
//      the row preprocess forms the stored depth from, xform4x3's z -- into dL_dmeans3D. (The dn plane's fold is normals.hip's.)
//
// The recurrence. Per pixel, over the entries k = 1..m the forward blended, with w_k = alpha_k T_k, the maps D = sum w_k z_k,
// A = sum w_k, N = sum w_k n_k (n_k: the Gaussian's normal) and the distortion sum_{j<k} w_j w_k |s_j - s_k|, s_k = f(z_k)
// (common.hpp: DistortionMap), the incoming gradients gD, gA, gN, gL at the pixel, M = the pixel's moment sum_k w_k s_k
// (render_distortion's second output) and
//     A_<k = 1 - T_k,   A_>k = T_{k+1} - T_{m+1},   S_>k = sum_{j>k} w_j s_j,   S_<k = M - S_>k - w_k s_k:
//     u_k         = dL/dw_k through the distortion = 2 gL (s_k (A_<k - A_>k) - S_<k + S_>k)                            (DIST)
//     c_k         = gD z_k + gA  [+ u_k]  [+ gN . n_k]             the normal map is one more "colour"
//     dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k)  (no background term: A telescopes)
//     dL/dz_k     = w_k (gD  [+ 2 gL (A_<k - A_>k) f'(z_k)])
//     dL/dn_k     = w_k gN                                                                                            (NORMAL)
// From dL/dalpha_k the chain to opacity, conic and 2D mean is render_backward_kernel's for a colour channel: the six moments
// {S0, Sx, Sy, Sxx, Sxy, Syy} of G dL/dalpha about the Gaussian's 2D mean, which backward_preprocess.hip turns into the gradients.
//
// The pivot (DIST). The loss does not change when every s of a pixel moves by a constant, but fp32 sums of w s do: u_k is a
// difference of sums of the size of s, which cancels where a pixel's mass is concentrated (the ndc mode: s near 1, spreads of
// 0.01). So the recurrences run on s_k - p with the pivot p = M / A, A = 1 - T_{m+1}, and the moment M - p A (what fp32 leaves of
// zero); every equation above holds for any p. s_k - p is formed in one rounding at the size of the difference
// (DistortionMap::about), and the forward hands over an M that is sum w s to within one rounding of its own size
// (render_distortion.hip sums about a pivot of its own). tests/test_distortion_ref_cpu.py restates both kernels in fp32 and holds
// them to half the GPU bars; the plain recurrences miss them there by a factor of up to nine.
//
// The walk is a replay of the finished forward (replay.hpp: the tile walk, the staging, the candidate lists and the forward's
// cuts tile_used_c / n_contrib_c; it decides nothing again), BACK TO FRONT with render_backward_kernel's recurrences: T starts at
// the forward's final_T = T_{m+1} and is divided by (1 - alpha) on the way to the front, the suffix sums S_> and sum w c grow from
// 0. The staged record carries z in place of the red and (DIST) 1 / z in its spare word. Per row of 8 candidates the per-pixel
// terms {w, w dx, w dx^2, dz [, dn]} are reduced over a pixel row with the column levels of render_common.hpp's transposing
// butterfly, the row's dy gives the y-moments, the row levels add the sums over the 8 rows (the pairings and roundings of
// render_backward_kernel's network, so the sums are that kernel's for a colour channel), the four waves meet in LDS, and one
// thread per entry merges them, (0 + 1) + (2 + 3), and ADDS the six moments into the entry's 36-byte slot of the product
// backward's partial sums (entry_slot(); read-add-store where the slot's flag byte is set, a store that sets the byte otherwise;
// the colour components stay as they are). A slot belongs to one (Gaussian, tile), i.e. to one workgroup of this grid, and
// render_backward has finished on the stream: no race. dL/dz goes to a 4-byte plane of its own in the same slot numbering, dL/dn
// (NORMAL) to a plane of three floats per slot behind it; both are written for every slot whose flag is set afterwards.
//
// LDS. The stage (replay.hpp) is 20,928 B. Without the normal map seven per-wave sums per batch entry are 28,672 B and the hit
// flags 1,024 B: 50,624 B, inside 41 granules of 1280 B = three workgroups per CU, three waves per SIMD. With it ten sums are
// 40,960 B and three workgroups are out of reach whatever else is trimmed: TWO per CU, inside the 64 KB a workgroup may declare,
// so nothing about the launch is special: with the normals of the staged entries, 3,084 B, and hit flags of 64 B, 65,036 B.
// Those normals need no second buffer (the walk has two barriers per batch and nobody reads a batch's normals behind the second).
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

// "Some pixel of the tile blended batch entry j": cleared by thread j in front of a batch's first barrier, set by the lanes that
// report on an entry between the barriers, read by thread j behind the second. Two forms of the same OR, so no result depends on
// which is used. Without the normal map a byte per (wave, entry) and plain stores: the bits below cost the distortion instance
// 0.7 % on the bench scene (profiles/maps_backward/README.md). With it the bytes do not fit the 64 KB: one BIT per entry that the
// waves OR together (an integer LDS atomic: exact and order-free), double-buffered, because a word is shared by the 32 threads
// that read it in the merge -- the bits of round r - 2 were last read behind that round's second barrier, and every thread has
// passed the first barrier of round r - 1 since.
template <bool NORMAL> struct HitFlags;
template <> struct HitFlags<false> {
    uint8_t bytes[4][BATCH];
    __device__ __forceinline__ void clear(int, int tid)
    {
#pragma unroll
        for (int w = 0; w < 4; w++) bytes[w][tid] = 0;
    }
    __device__ __forceinline__ void set(int, int wave, int j, uint32_t hit) { bytes[wave][j] = (uint8_t)hit; }
    __device__ __forceinline__ uint32_t read(int, int tid) const
    {
        return (uint32_t)bytes[0][tid] | bytes[1][tid] | bytes[2][tid] | bytes[3][tid];
    }
};
template <> struct HitFlags<true> {
    uint32_t bits[2][BATCH / 32];
    __device__ __forceinline__ void clear(int buf, int tid) { if (tid < BATCH / 32) bits[buf][tid] = 0u; }
    __device__ __forceinline__ void set(int buf, int, int j, uint32_t hit)
    {
        if (hit) atomicOr(&bits[buf][j >> 5], 1u << (j & 31));
    }
    __device__ __forceinline__ uint32_t read(int buf, int tid) const { return (bits[buf][tid >> 5] >> (tid & 31)) & 1u; }
};

template <bool DIST, bool NORMAL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NORMAL ? 2 : 3, NORMAL ? 2 : 3)))
render_maps_backward_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges,
                            const uint32_t* __restrict__ tile_used_c, const uint32_t* __restrict__ n_contrib_c,
                            const float* __restrict__ final_Ts, const uint32_t* __restrict__ cid, const uint8_t* __restrict__ cqm,
                            const float4* __restrict__ splat, const uint32_t* __restrict__ depth_keys,
                            const uint32_t* __restrict__ block_base, const float4* __restrict__ normals,
                            const float* __restrict__ dL_ddepth, const float* __restrict__ dL_dalpha_map,
                            const float* __restrict__ dL_dnormal, const float* __restrict__ dL_ddistortion,
                            const float* __restrict__ moment, DistortionMap f, float* __restrict__ partials,
                            float* __restrict__ dz_plane, NormalSlot* __restrict__ dn_plane, uint8_t* __restrict__ touched,
                            const uint32_t* __restrict__ sort_err)
{
    // every product below is rounded on its own, as in render_backward_kernel, whose terms feed hand-placed DPP adds: the sums are
    // then that kernel's bits for a colour channel (explicit fmaf calls are not affected)
#pragma clang fp contract(off)
    constexpr int TERMS = 7 + 3 * NORMAL;            // S0, Sx, Sy, Sxx, Sxy, Syy, dz [, dn_x, dn_y, dn_z]
    if (block_has_no_tile(blockIdx.x, T)) return;
    // the sort's time-out word, as in the forward: set -> the lists are not to be trusted, walk nothing (the folds write NaN)
    if (*sort_err != 0u) return;
    __shared__ ReplayStage st;                       // the staged record carries z in place of the red, 1 / z behind it (DIST)
    __shared__ float s_stat[4][BATCH][TERMS];        // [wave][batch entry] the sums over the wave's 64 pixels
    __shared__ HitFlags<NORMAL> s_hit;               // ... and whether any of them blended it
    // NORMAL: the staged entries' normals by component; entry BATCH: the sentinel's zeros (an instance without takes no LDS for it)
    __shared__ float s_n[3][BATCH + 1];
    static_assert(sizeof(st) + sizeof(s_stat) + sizeof(s_hit) + (NORMAL ? sizeof(s_n) : 0) <= (NORMAL ? 65536 : 41 * 1280),
                  "render_maps_backward: more than 64 KB of LDS in one workgroup, or, without the normal map, more than 41 LDS "
                  "granules = two workgroups per CU instead of three");

    // t.last is where this pixel's walk starts
    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, false, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;
    if constexpr (NORMAL) {
        if (tid < 3) s_n[tid][BATCH] = 0.f;
    }
    const float Tfin = t.inside ? final_Ts[t.pix] : 0.f;        // T_{m+1}: transmittance behind the pixel's last blended entry
    float Tr = Tfin;
    const float gD = (t.inside && dL_ddepth) ? dL_ddepth[t.pix] : 0.f;
    const float gA = (t.inside && dL_dalpha_map) ? dL_dalpha_map[t.pix] : 0.f;
    const size_t n_pix = (size_t)W * H;
    const float gN0 = (NORMAL && t.inside) ? dL_dnormal[t.pix] : 0.f;
    const float gN1 = (NORMAL && t.inside) ? dL_dnormal[n_pix + t.pix] : 0.f;
    const float gN2 = (NORMAL && t.inside) ? dL_dnormal[2 * n_pix + t.pix] : 0.f;
    // DIST, the pivot: every s of the pixel is taken about the pixel's mean s = moment / A, and the moment with it
    const float gL2 = (DIST && t.inside) ? 2.0f * dL_ddistortion[t.pix] : 0.f;
    const float Apix = 1.0f - Tfin;
    const float Mraw = (DIST && t.inside) ? moment[t.pix] : 0.f;
    const float piv = Apix > 0.f ? Mraw / Apix : 0.f;
    const float M = fmaf(-piv, Apix, Mraw);                     // sum_k w_k (s_k - piv): what fp32 leaves of 0
    const float qs = f.c0 - piv;                                // s_k - piv = DistortionMap::about(z, 1 / z, qs), one rounding
    float Sd = 0.f;                                             // sum_{j behind} w_j c_j
    float Ss = 0.f;                                             // DIST: S_>, sum_{j behind} w_j (s_j - piv)

    const int beta = candidate_of_lane(lane);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    float4 nr = ra;
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
            if (DIST) rb.w = f.rz(rb.z);                        // the record's spare word
            if (NORMAL) nr = normals[id];
            slot_next = entry_slot(splat[3 * (size_t)id + 2], block_base, id, t.tx, t.ty);
        }
    };
    gather(tid);
    for (int r = 0; r < t.rounds; r++) {
        const int buf = r & 1;
        const uint32_t slot = slot_next;                        // of batch entry `tid`, which this thread stages and later merges
        stage_batch(st, buf, tid, ra, rb);
        if constexpr (NORMAL) { s_n[0][tid] = nr.x; s_n[1][tid] = nr.y; s_n[2][tid] = nr.z; }
        publish_quadrant_masks(st, buf, wave, lane, qm);
        // a wave only writes the entries of its own candidate list: the others read as "nothing blended". This thread read
        // its entry's words of the previous batch behind that batch's second barrier, so it may clear them here.
#pragma unroll
        for (int w = 0; w < 4; w++) {
#pragma unroll
            for (int q = 0; q < TERMS; q++) s_stat[w][tid][q] = 0.f;
        }
        s_hit.clear(buf, tid);
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        const int pos0 = t.used - 1 - r * BATCH;                // 0-based compact position of batch entry j is pos0 - j
        // entries at position >= wave_last (j <= pos0 - wave_last) lie behind every pixel of this wave
        const int jmin = pos0 - t.wave_last + 1;
        if (jmin < BATCH) {
            const int nw = build_candidate_list(st, buf, wave, lane,
                                                [&](unsigned long long m, int c) { return drop_behind(m, jmin - c * 64); });
            // a pixel takes entry j only if pos0 - j < last, i.e. record offset > thr (the sentinel's opacity is 0: never a hit)
            const uint32_t buf_off = (uint32_t)buf * REPLAY_BUF_BYTES;
            const int thr = (int)buf_off + min(max(pos0 - t.last, -1), BATCH) * (int)REPLAY_REC_BYTES;
            for (int k = 0; k < nw; k += 8) {
                uint32_t e[8];
                load_row(st, wave, k, e);
                const uint32_t my_off = st.list[wave][k + beta];  // the candidate this lane reports on
                float v0[8], vx[8], vxx[8], vz[8], vn0[8], vn1[8], vn2[8];
                uint32_t my_hit = 0u;
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const StagedRecord s = staged_record(st, e[g]);
                    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
                    if constexpr (NORMAL) {
                        const int j = (int)((e[g] - buf_off) / REPLAY_REC_BYTES);
                        n0 = s_n[0][j]; n1 = s_n[1][j]; n2 = s_n[2][j];
                    }
                    float dx, dy, G, alpha;
                    bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                    // in front of the pixel's last contributor every hit was blended by the forward (its stop lies behind it)
                    hit = hit && ((int)e[g] > thr);
                    // branch-free, as render_backward: a pixel that does not blend the entry runs the same instructions with
                    // alpha = G = 0, which leaves T and the suffix sums untouched and makes every term exactly 0
                    const float a_eff = hit ? alpha : 0.f, G_eff = hit ? G : 0.f;
                    const float rinv = __builtin_amdgcn_rcpf(1.f - a_eff);   // 1 - alpha is in [0.01, 1]; rcp(1) == 1
                    const float dA = (1.0f - Tr * rinv) - (Tr - Tfin);       // DIST: A_<k - A_>k: Tr still is T_{k+1}
                    Tr = Tr * rinv;                              // transmittance in front of this entry
                    const float wgt = a_eff * Tr;                // alpha_k T_k
                    const float gn = (n0 * gN0 + n1 * gN1) + n2 * gN2;       // NORMAL
                    float cd = s.b.z * gD + gA;               // two roundings: the colour backward's (z, 1, 0) . (gD, gA, 0)
                    if constexpr (DIST) {
                        const float sk = f.about(s.b.z, s.b.w, qs);
                        const float ws = wgt * sk;
                        const float Slt = (M - Ss) - ws;         // S_<k
                        const float u = gL2 * fmaf(sk, dA, Ss - Slt);
                        cd = cd + u;
                        Ss = Ss + ws;
                        vz[g] = wgt * fmaf(gL2 * dA, f.ds(s.b.w), gD);
                    } else {
                        vz[g] = wgt * gD;
                    }
                    if constexpr (NORMAL) cd = cd + gn;
                    const float dL_dalpha = fmaf(Tr, cd, -(rinv * Sd));
                    Sd = fmaf(wgt, cd, Sd);
                    // w = G * dL/dalpha and its first two x-moments about the mean; the y-moments follow from the row sums
                    const float w = G_eff * dL_dalpha, wx = w * dx;
                    v0[g] = w; vx[g] = wx; vxx[g] = wx * dx;
                    if constexpr (NORMAL) { vn0[g] = wgt * gN0; vn1[g] = wgt * gN1; vn2[g] = wgt * gN2; }
                    const uint32_t h = __ballot(hit) != 0ull ? 1u : 0u;
                    my_hit = (beta == g) ? h : my_hit;
                }
                // column levels: the sums over this lane's pixel row of candidate beta; then this row's dy to that candidate (the
                // same subtraction gaussian_alpha made for it) gives the row's y-moments, and the row levels add the 8 rows up:
                // render_backward_kernel's pairings and roundings, term for term
                const float c0 = reduce_columns_of_8(v0, lane, OpAdd()), cx = reduce_columns_of_8(vx, lane, OpAdd());
                const float cxx = reduce_columns_of_8(vxx, lane, OpAdd()), cz = reduce_columns_of_8(vz, lane, OpAdd());
                float cn0 = 0.f, cn1 = 0.f, cn2 = 0.f;
                if constexpr (NORMAL) {
                    cn0 = reduce_columns_of_8(vn0, lane, OpAdd()); cn1 = reduce_columns_of_8(vn1, lane, OpAdd());
                    cn2 = reduce_columns_of_8(vn2, lane, OpAdd());
                }
                const float dyb = staged_mean_y(st, my_off) - t.pyf;
                float sum[TERMS];
                sum[0] = reduce_rows_of_8(c0, OpAdd());
                sum[1] = reduce_rows_of_8(cx, OpAdd());
                sum[2] = reduce_rows_of_8(dyb * c0, OpAdd());
                sum[3] = reduce_rows_of_8(cxx, OpAdd());
                sum[4] = reduce_rows_of_8(dyb * cx, OpAdd());
                sum[5] = reduce_rows_of_8((dyb * dyb) * c0, OpAdd());
                sum[6] = reduce_rows_of_8(cz, OpAdd());
                if constexpr (NORMAL) {
                    sum[7] = reduce_rows_of_8(cn0, OpAdd());
                    sum[8] = reduce_rows_of_8(cn1, OpAdd());
                    sum[9] = reduce_rows_of_8(cn2, OpAdd());
                }
                // each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane
                const int myj = batch_entry_of(my_off, buf);
                if (lane < 8 && myj < BATCH) {
#pragma unroll
                    for (int q = 0; q < TERMS; q++) s_stat[wave][myj][q] = sum[q];
                    s_hit.set(buf, wave, myj, my_hit);
                }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves, (0 + 1) + (2 + 3) as render_backward_kernel's flush, and owns the slot
        if (r * BATCH + tid < t.used) {
            const uint32_t h = s_hit.read(buf, tid);
            const bool was = touched[slot] != 0;
            if (h || was) {
                float t[TERMS];
#pragma unroll
                for (int q = 0; q < TERMS; q++)
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
                if constexpr (NORMAL) {
                    const NormalSlot dn = { t[7], t[8], t[9] };
                    dn_plane[slot] = dn;                         // likewise
                }
            }
        }
    }
}

// ---- stage B
__global__ void __launch_bounds__(256)
depth_backward_fold_kernel(int P, const uint32_t* __restrict__ live_count, const uint32_t* __restrict__ live_ids,
                           const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base,
                           const float* __restrict__ dz_plane, const uint8_t* __restrict__ touched,
                           const float* __restrict__ view, float* __restrict__ dL_dmeans3D, const uint32_t* __restrict__ sort_err)
{
    const ListedGaussian lg = listed_gaussian(live_count, live_ids);
    if (!lg.wave_has_work) return;
    const bool live = lg.live;
    const int i = lg.i, lane = threadIdx.x & 63;
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

void launch_render_maps_backward(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const BwdPtrs& w,
                                 float* dz_plane, NormalSlot* dn_plane, const float* normals, const float* dL_ddepth,
                                 const float* dL_dalpha, const float* dL_dnormal, const float* dL_ddistortion, const float* moment,
                                 const DistortionMap& f, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    const bool dist = dL_ddistortion != nullptr;
    const auto kernel = dL_dnormal ? (dist ? render_maps_backward_kernel<true, true> : render_maps_backward_kernel<false, true>)
                                   : (dist ? render_maps_backward_kernel<true, false> : render_maps_backward_kernel<false, false>);
    kernel<<<banded_grid(T), 256, 0, s>>>(W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, img.final_T, cl.cid, cl.cqm,
                                          g.splat, g.depth_keys, g.block_base, reinterpret_cast<const float4*>(normals), dL_ddepth,
                                          dL_dalpha, dL_dnormal, dL_ddistortion, moment, f, w.partials, dz_plane, dn_plane, w.touched,
                                          sort_err);
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
