// render_normal_backward.hip -- gradients through the depth, accumulated-opacity, NORMAL and (optionally) distortion maps
// (render_depth.hip, render_normal.hip, render_distortion.hip) in ONE blend replay, for gfx950. The reference's rasterizer has no
// counterpart.
//
// Where the loss uses the normal map this kernel runs INSTEAD of render_depth_backward_kernel / render_distortion_backward_kernel,
// never beside them, so a backward replays the blend once for all of its maps. Per pixel, over the entries k = 1..m the forward
// blended, with w_k = alpha_k T_k, n_k the Gaussian's normal and gN the incoming gradient of the normal map at the pixel, it is
// those kernels' recurrence (see there; DIST = false: render_depth_backward's expressions, DIST = true: the pivoted ones of
// render_distortion_backward, term for term) with
//     c_k        += gN . n_k                                   the normal map is one more "colour": N = sum_k w_k n_k
//     dL/dn_g     = sum over the pixels of w_k gN              three floats per (Gaussian, tile) slot in a plane of their own, in
//                                                              the slot numbering of the partials and the dL/dz plane, under the
//                                                              same `touched` flags; normal_backward_fold_kernel (normals.hip)
//                                                              folds it behind backward_preprocess.
// The walk, the reduction network, the slots, the flags and the dL/dz plane are render_depth_backward_kernel's.
//
// LDS. Ten per-wave sums per batch entry (that kernel's seven and the three of dn) are 40 KB where seven are 28 KB, and 41
// granules = three workgroups per CU are out of reach whatever else is trimmed. The choice made here: TWO workgroups per CU (two
// waves per SIMD), but inside the 64 KB a workgroup may declare, so nothing about the launch is special:
//     the stage 20,928 B + the sums 40,960 B + the normals 3,084 B + the hit bits 64 B = 65,036 B.
// What was trimmed to get there: the normals of the staged entries need no second buffer (this walk has two barriers per batch
// and nobody reads a batch's normals behind the second), and "some pixel of wave w blended entry j" is one BIT per entry that
// the waves OR together (an integer LDS atomic: exact and order-free) in place of a byte per (wave, entry); the bits are
// double-buffered, because a word is shared by the 32 threads that read it in the merge.
// No float atomics, bitwise reproducible. The sort's time-out word set: walks nothing (the folds write NaN).
#include "common.hpp"
#include "render_common.hpp"
#include "replay.hpp"

namespace c3dgs {

constexpr int NORMAL_BWD_TERMS = 10;  // S0, Sx, Sy, Sxx, Sxy, Syy, dz, dn_x, dn_y, dn_z

template <bool DIST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
render_normal_backward_kernel(int W, int H, int gx, int T, const uint2* __restrict__ ranges,
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
    // every product below is rounded on its own, as in the two kernels this one stands in for (explicit fmaf calls are not affected)
#pragma clang fp contract(off)
    if (block_has_no_tile(blockIdx.x, T)) return;
    if (*sort_err != 0u) return;
    __shared__ ReplayStage st;                       // the staged record carries z in place of the red, 1 / z behind it (DIST)
    __shared__ float s_stat[4][BATCH][NORMAL_BWD_TERMS];  // [wave][batch entry] the ten sums over the wave's 64 pixels
    __shared__ float s_n[3][BATCH + 1];              // the staged entries' normals by component; entry BATCH: the sentinel's zeros
    __shared__ uint32_t s_hit[2][BATCH / 32];        // [round & 1] bit j: some pixel of the tile blended batch entry j
    static_assert(sizeof(st) + sizeof(s_stat) + sizeof(s_n) + sizeof(s_hit) <= 65536,
                  "render_normal_backward: more than 64 KB of LDS in one workgroup");

    const ReplayTile t = replay_tile(blockIdx.x, W, H, gx, T, ranges, tile_used_c, n_contrib_c, false, st);
    const int tid = t.tid, wave = t.wave, lane = t.lane;
    if (tid < 3) s_n[tid][BATCH] = 0.f;
    const float Tfin = t.inside ? final_Ts[t.pix] : 0.f;        // T_{m+1}: transmittance behind the pixel's last blended entry
    float Tr = Tfin;
    const float gD = (t.inside && dL_ddepth) ? dL_ddepth[t.pix] : 0.f;
    const float gA = (t.inside && dL_dalpha_map) ? dL_dalpha_map[t.pix] : 0.f;
    const size_t n_pix = (size_t)W * H;
    const float gN0 = t.inside ? dL_dnormal[t.pix] : 0.f;
    const float gN1 = t.inside ? dL_dnormal[n_pix + t.pix] : 0.f;
    const float gN2 = t.inside ? dL_dnormal[2 * n_pix + t.pix] : 0.f;
    // DIST: render_distortion_backward_kernel's pivot, see there
    const float gL2 = (DIST && t.inside) ? 2.0f * dL_ddistortion[t.pix] : 0.f;
    const float Apix = 1.0f - Tfin;
    const float Mraw = (DIST && t.inside) ? moment[t.pix] : 0.f;
    const float piv = Apix > 0.f ? Mraw / Apix : 0.f;
    const float M = fmaf(-piv, Apix, Mraw);
    const float qs = f.c0 - piv;
    float Sd = 0.f;                                             // sum_{j behind} w_j c_j
    float Ss = 0.f;                                             // DIST: S_>, sum_{j behind} w_j (s_j - piv)

    const int beta = candidate_of_lane(lane);

    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    float4 nr = ra;
    uint32_t qm = 0u, slot_next = 0u;
    auto gather = [&](int back) {                               // `back`-th entry from the end -> this thread's staging registers
        qm = 0u;
        const int pos = t.used - 1 - back;
        if (pos >= 0) {
            const uint32_t id = cid[t.range.x + pos];
            qm = cqm[t.range.x + pos];
            ra = splat[3 * (size_t)id]; rb = splat[3 * (size_t)id + 1];
            rb.z = __uint_as_float(depth_keys[id]);             // in place of the record's red
            if (DIST) rb.w = f.rz(rb.z);                        // the record's spare word
            nr = normals[id];
            slot_next = entry_slot(splat[3 * (size_t)id + 2], block_base, id, t.tx, t.ty);
        }
    };
    gather(tid);
    for (int r = 0; r < t.rounds; r++) {
        const int buf = r & 1;
        const uint32_t slot = slot_next;                        // of batch entry `tid`, which this thread stages and later merges
        stage_batch(st, buf, tid, ra, rb);
        s_n[0][tid] = nr.x; s_n[1][tid] = nr.y; s_n[2][tid] = nr.z;
        publish_quadrant_masks(st, buf, wave, lane, qm);
#pragma unroll
        for (int w = 0; w < 4; w++) {
#pragma unroll
            for (int q = 0; q < NORMAL_BWD_TERMS; q++) s_stat[w][tid][q] = 0.f;
        }
        // the bits of round r - 2 were last read behind that round's second barrier, and every thread has passed the first
        // barrier of round r - 1 since
        if (tid < BATCH / 32) s_hit[buf][tid] = 0u;
        __syncthreads();
        gather((r + 1) * BATCH + tid);                          // the next batch, behind this batch's blending
        const int pos0 = t.used - 1 - r * BATCH;                // 0-based compact position of batch entry j is pos0 - j
        const int jmin = pos0 - t.wave_last + 1;
        if (jmin < BATCH) {
            const int nw = build_candidate_list(st, buf, wave, lane,
                                                [&](unsigned long long m, int c) { return drop_behind(m, jmin - c * 64); });
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
                    const int j = (int)((e[g] - buf_off) / REPLAY_REC_BYTES);
                    const float n0 = s_n[0][j], n1 = s_n[1][j], n2 = s_n[2][j];
                    float dx, dy, G, alpha;
                    bool hit = gaussian_alpha(s.a.x, s.a.y, s.a.z, s.a.w, s.b.x, s.b.y, t.pxf, t.pyf, dx, dy, G, alpha);
                    hit = hit && ((int)e[g] > thr);
                    // branch-free: a pixel that does not blend the entry runs the same instructions with alpha = G = 0, which leaves
                    // T and the suffix sums untouched and makes all ten terms exactly 0
                    const float a_eff = hit ? alpha : 0.f, G_eff = hit ? G : 0.f;
                    const float rinv = __builtin_amdgcn_rcpf(1.f - a_eff);   // 1 - alpha is in [0.01, 1]; rcp(1) == 1
                    const float dA = (1.0f - Tr * rinv) - (Tr - Tfin);       // DIST: A_<k - A_>k: Tr still is T_{k+1}
                    Tr = Tr * rinv;                              // transmittance in front of this entry
                    const float wgt = a_eff * Tr;                // alpha_k T_k
                    const float gn = (n0 * gN0 + n1 * gN1) + n2 * gN2;
                    float cd = s.b.z * gD + gA;
                    if (DIST) {
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
                    cd = cd + gn;
                    const float dL_dalpha = fmaf(Tr, cd, -(rinv * Sd));
                    Sd = fmaf(wgt, cd, Sd);
                    const float w = G_eff * dL_dalpha, wx = w * dx;
                    v0[g] = w; vx[g] = wx; vxx[g] = wx * dx;
                    vn0[g] = wgt * gN0; vn1[g] = wgt * gN1; vn2[g] = wgt * gN2;
                    const uint32_t h = __ballot(hit) != 0ull ? 1u : 0u;
                    my_hit = (beta == g) ? h : my_hit;
                }
                const float c0 = reduce_columns_of_8(v0, lane, OpAdd()), cx = reduce_columns_of_8(vx, lane, OpAdd());
                const float cxx = reduce_columns_of_8(vxx, lane, OpAdd()), cz = reduce_columns_of_8(vz, lane, OpAdd());
                const float cn0 = reduce_columns_of_8(vn0, lane, OpAdd()), cn1 = reduce_columns_of_8(vn1, lane, OpAdd());
                const float cn2 = reduce_columns_of_8(vn2, lane, OpAdd());
                const float dyb = staged_mean_y(st, my_off) - t.pyf;
                float sum[NORMAL_BWD_TERMS];
                sum[0] = reduce_rows_of_8(c0, OpAdd());
                sum[1] = reduce_rows_of_8(cx, OpAdd());
                sum[2] = reduce_rows_of_8(dyb * c0, OpAdd());
                sum[3] = reduce_rows_of_8(cxx, OpAdd());
                sum[4] = reduce_rows_of_8(dyb * cx, OpAdd());
                sum[5] = reduce_rows_of_8((dyb * dyb) * c0, OpAdd());
                sum[6] = reduce_rows_of_8(cz, OpAdd());
                sum[7] = reduce_rows_of_8(cn0, OpAdd());
                sum[8] = reduce_rows_of_8(cn1, OpAdd());
                sum[9] = reduce_rows_of_8(cn2, OpAdd());
                // each (wave, entry) pair occurs once: plain LDS stores into the wave's own plane
                const int myj = batch_entry_of(my_off, buf);
                if (lane < 8 && myj < BATCH) {
#pragma unroll
                    for (int q = 0; q < NORMAL_BWD_TERMS; q++) s_stat[wave][myj][q] = sum[q];
                    if (my_hit) atomicOr(&s_hit[buf][myj >> 5], 1u << (myj & 31));
                }
            }
        }
        __syncthreads();
        // one thread per batch entry merges the four waves, (0 + 1) + (2 + 3), and owns the slot
        if (r * BATCH + tid < t.used) {
            const uint32_t h = (s_hit[buf][tid >> 5] >> (tid & 31)) & 1u;
            const bool was = touched[slot] != 0;
            if (h || was) {
                float t[NORMAL_BWD_TERMS];
#pragma unroll
                for (int q = 0; q < NORMAL_BWD_TERMS; q++)
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
                dz_plane[slot] = t[6];                           // both valid wherever the flag is set behind this kernel
                const NormalSlot dn = { t[7], t[8], t[9] };
                dn_plane[slot] = dn;
            }
        }
    }
}

void launch_render_normal_backward(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const BwdPtrs& w,
                                   float* dz_plane, NormalSlot* dn_plane, const float* normals, const float* dL_ddepth,
                                   const float* dL_dalpha, const float* dL_dnormal, const float* dL_ddistortion, const float* moment,
                                   const DistortionMap& f, const uint32_t* sort_err, hipStream_t s)
{
    const int gx = tiles_x(W), T = gx * tiles_y(H);
    const float4* nrm = reinterpret_cast<const float4*>(normals);
    if (dL_ddistortion)
        render_normal_backward_kernel<true><<<banded_grid(T), 256, 0, s>>>(
            W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, img.final_T, cl.cid, cl.cqm, g.splat, g.depth_keys, g.block_base,
            nrm, dL_ddepth, dL_dalpha, dL_dnormal, dL_ddistortion, moment, f, w.partials, dz_plane, dn_plane, w.touched, sort_err);
    else
        render_normal_backward_kernel<false><<<banded_grid(T), 256, 0, s>>>(
            W, H, gx, T, img.ranges, img.tile_used_c, img.n_contrib_c, img.final_T, cl.cid, cl.cqm, g.splat, g.depth_keys, g.block_base,
            nrm, dL_ddepth, dL_dalpha, dL_dnormal, nullptr, nullptr, f, w.partials, dz_plane, dn_plane, w.touched, sort_err);
}

} // namespace c3dgs
