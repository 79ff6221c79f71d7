// replay.hpp -- the skeleton of the passes that REPLAY a finished forward (render_depth.hip, render_contrib.hip, render_error.hip,
// render_maps_backward.hip), the fold of a Gaussian's slot run behind three of them, and the lane -> listed Gaussian map of the
// kernels that walk sum_partials_kernel's lists. One owner per piece, so that the passes walk the same entries, take the same cuts,
// number the same slots and add in the same order: a map of ones gives weight_sum's bits, render_depth's w is render_contrib's,
// the map backward touches the slots the product backward numbers. Device code only.
//
// A replay decides nothing again: it walks the tile's compact list (cid / cqm: the entries that can reach the tile, in list order)
// up to tile_used_c[tile], and a pixel only takes entries whose compact index is <= n_contrib_c[pix] -- the forward's own early
// stop. Inside that prefix the hit test is the forward's gaussian_alpha() on the same pre-scaled conic, so the same bits give the
// same decisions, the same T and the same weights. Positions past tile_used_c are never read (the compact list is only written
// that far).
//
// Structure = render_forward_kernel's: one 16x16 tile per 256-thread workgroup, one 8x8 quadrant per wave, batches of 256 entries
// staged into double-buffered LDS (one barrier per batch, the next batch's gather in flight behind the blend), per-wave candidate
// lists of LDS byte offsets from the cqm ballots. What a pass does with a pair -- its statistic, the LDS planes for it, the merge
// of the four waves and the slot write -- is the pass's own and stays in its file.
#pragma once
#include "common.hpp"
#include "render_common.hpp"

namespace c3dgs {

// ---------------------------------------------------------------- the tile walk
// The staged record is 32 bytes {x, y, ka, kb | kc, opacity, z or red, -}: two ds_read_b128 per pair. The candidate lists hold the
// records' BYTE OFFSETS inside `ab`, so a list word read back from LDS is the address operand of those reads as it is.
constexpr uint32_t REPLAY_REC_BYTES = 32, REPLAY_BUF_BYTES = (BATCH + 1) * REPLAY_REC_BYTES;

struct ReplayStage {                                  // LDS of a replay kernel, next to the planes of its statistic
    float4 ab[2][BATCH + 1][2];                       // entry BATCH of each buffer: sentinel with opacity 0 (blends nothing)
    uint32_t list[4][BATCH + 8];                      // per wave: its candidates of the batch, padded to a multiple of 8
    unsigned long long mask[2][4][4];                 // [buf][quadrant][staging wave]
};

struct ReplayTile {
    int tid, wave, lane;
    int tile, tx, ty, px, py;
    bool inside;
    float pxf, pyf;
    size_t pix;
    uint2 range;                                      // the tile's span of the compact list
    int used, rounds;                                 // compact entries the forward wrote and some pixel blended; batches of them
    int last, wave_last;                              // 1-based compact index of the pixel's last blended entry; the wave's deepest
};

// Workgroup b's tile and this thread's pixel in it, and how far the tile, the pixel and the wave walk. Also writes the two sentinel
// records of `st`. `poisoned`: the sort's time-out word is set and the caller goes on regardless -> the lists are not to be
// trusted, nothing is walked. (What a pass does about a time-out is its own business: it may as well return before it gets here.)
__device__ __forceinline__ ReplayTile replay_tile(int b, int W, int H, int gx, int T, const uint2* __restrict__ ranges,
                                                  const uint32_t* __restrict__ tile_used_c, const uint32_t* __restrict__ n_contrib_c,
                                                  bool poisoned, ReplayStage& st)
{
    ReplayTile c;
    c.tile = tile_of_block(b, T);
    c.tid = threadIdx.x; c.wave = c.tid >> 6; c.lane = c.tid & 63;
    c.tx = c.tile % gx; c.ty = c.tile / gx;
    c.px = c.tx * TILE + (c.wave & 1) * 8 + (c.lane & 7);
    c.py = c.ty * TILE + (c.wave >> 1) * 8 + (c.lane >> 3);
    c.inside = c.px < W && c.py < H;
    c.pxf = (float)c.px; c.pyf = (float)c.py;
    c.pix = (size_t)W * c.py + c.px;
    if (c.tid < 2) { st.ab[c.tid][BATCH][0] = make_float4(0, 0, 0, 0); st.ab[c.tid][BATCH][1] = make_float4(0, 0, 0, 0); }

    c.range = poisoned ? make_uint2(0u, 0u) : ranges[c.tile];
    const int n = (int)(c.range.y - c.range.x);
    c.used = poisoned ? 0 : min(n, (int)tile_used_c[c.tile]);
    c.rounds = (c.used + BATCH - 1) / BATCH;

    c.last = (c.inside && !poisoned) ? min((int)n_contrib_c[c.pix], c.used) : 0;
    c.wave_last = c.last;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c.wave_last = max(c.wave_last, __shfl_xor(c.wave_last, o));
    c.wave_last = __builtin_amdgcn_readfirstlane(c.wave_last);      // tell the compiler it is wave-uniform (scalar loop control)
    return c;
}

// this thread's gathered entry -> record `tid` of buffer `buf`, its conic pre-scaled (render_common.hpp says why)
__device__ __forceinline__ void stage_batch(ReplayStage& st, int buf, int tid, float4& ra, float4& rb)
{
    prescale_conic(ra, rb);
    st.ab[buf][tid][0] = ra; st.ab[buf][tid][1] = rb;
}

// qm = the quadrant mask of this thread's entry (0 for none): which of the staging wave's 64 entries reach each quadrant
__device__ __forceinline__ void publish_quadrant_masks(ReplayStage& st, int buf, int wave, int lane, uint32_t qm)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const unsigned long long bm = __ballot((qm >> q) & 1u);
        if (lane == 0) st.mask[buf][q][wave] = bm;
    }
}

// The two cuts of a staging wave's 64-entry mask at the wave's deepest pixel.
// Front to back: entry j of batch r has compact index r * BATCH + j + 1, so nothing at or behind j = wave_last - r * BATCH matters
// to the wave; of staging wave c's entries only the first jn = that - 64 c lie in front of the cut.
__device__ __forceinline__ unsigned long long keep_in_front(unsigned long long m, int jn)
{
    if (jn <= 0) m = 0; else if (jn < 64) m &= (1ull << jn) - 1ull;
    return m;
}
// Back to front: batch entry j is compact position pos0 - j, and positions >= wave_last lie behind every pixel of the wave; of
// staging wave c's entries the first jmin = pos0 - wave_last + 1 - 64 c do.
__device__ __forceinline__ unsigned long long drop_behind(unsigned long long m, int jmin)
{
    if (jmin >= 64) m = 0; else if (jmin > 0) m &= ~0ull << jmin;
    return m;
}

// This wave's candidates of the batch -> its list of record offsets, in batch order, padded with a row of the sentinel's. Returns
// their number. trim(m, c) = the part of staging wave c's 64-entry mask m that the caller's cut leaves (one of the two above, at
// the caller's cut). Wave-private: a wave fence, no workgroup barrier.
template <class Trim>
__device__ __forceinline__ int build_candidate_list(ReplayStage& st, int buf, int wave, int lane, Trim trim)
{
    int nw = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t buf_off = (uint32_t)buf * REPLAY_BUF_BYTES;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const unsigned long long m = trim(uniform_u64(st.mask[buf][wave][c]), c);
        if ((m >> lane) & 1ull) st.list[wave][nw + (int)__popcll(m & lt)] = buf_off + (uint32_t)(c * 64 + lane) * REPLAY_REC_BYTES;
        nw += (int)__popcll(m);
    }
    if (lane < 8) st.list[wave][nw + lane] = buf_off + (uint32_t)BATCH * REPLAY_REC_BYTES;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return nw;
}

// Front to back a pixel takes entry j of batch r only if r * BATCH + j + 1 <= last, i.e. with jn = last - r * BATCH only list
// words (record offsets) below this value (the sentinel's never is). In front of the pixel's last contributor every hit was
// blended by the forward (its stop lies behind it), so hit && word < cut is "the forward blended this pair".
__device__ __forceinline__ int front_cut(int buf, int jn)
{
    return (int)((uint32_t)buf * REPLAY_BUF_BYTES) + min(max(jn, 0), BATCH) * (int)REPLAY_REC_BYTES;
}

// candidates k .. k + 7 of the wave's list: two 16-byte reads
__device__ __forceinline__ void load_row(const ReplayStage& st, int wave, int k, uint32_t (&e)[8])
{
    const uint4 row0 = *reinterpret_cast<const uint4*>(&st.list[wave][k]);
    const uint4 row1 = *reinterpret_cast<const uint4*>(&st.list[wave][k + 4]);
    e[0] = row0.x; e[1] = row0.y; e[2] = row0.z; e[3] = row0.w;
    e[4] = row1.x; e[5] = row1.y; e[6] = row1.z; e[7] = row1.w;
}

// the staged record at list word `off`
struct StagedRecord { float4 a, b; };
__device__ __forceinline__ StagedRecord staged_record(const ReplayStage& st, uint32_t off)
{
    const char* rec_base = reinterpret_cast<const char*>(&st.ab[0][0][0]);
    StagedRecord r;
    r.a = *reinterpret_cast<const float4*>(rec_base + off);
    r.b = *reinterpret_cast<const float4*>(rec_base + off + 16);
    return r;
}
__device__ __forceinline__ float staged_mean_y(const ReplayStage& st, uint32_t off)
{
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(&st.ab[0][0][0]) + off + 4);
}

// list word -> batch entry (BATCH for the sentinel that pads a row). Behind a row's reduction lanes 0..7 hold the row's 8
// candidates (candidate_of_lane is a permutation of them) and report on entry batch_entry_of(list[k + candidate_of_lane(lane)]).
__device__ __forceinline__ int batch_entry_of(uint32_t off, int buf)
{
    return (int)((off - (uint32_t)buf * REPLAY_BUF_BYTES) / REPLAY_REC_BYTES);
}

// ---------------------------------------------------------------- the fold of a Gaussian's slot run
// One lane per Gaussian folds the written slots of its run in slot order. A run longer than LONG_RUN slots (a splat over hundreds
// of tiles; with one lane on it the whole wave waits for that lane: 1.63 ms on the heavy-tailed scene) is folded by the WHOLE wave
// instead: lane l takes slots start + l, start + l + 64, ... in that order and the 64 partial results meet in an xor butterfly
// (32, 16, ..., 1). Which lane adds what, and the order of the butterfly, follow from the run's start and length alone, so the
// result is the same bits whoever the neighbours are.
//
// V is what a slot holds. It comes with fold_zero(V&), the identity an unwritten slot contributes; fold_add(V& acc, const V&);
// and fold_shfl_xor(const V&, int), the partner lane's copy.
constexpr uint32_t LONG_RUN = 64;

__device__ __forceinline__ void fold_zero(float& v) { v = 0.f; }
__device__ __forceinline__ void fold_add(float& acc, const float& v) { acc += v; }
__device__ __forceinline__ float fold_shfl_xor(const float& v, int o) { return __shfl_xor(v, o); }

// Every lane of the wave calls this (the shuffles need them all); a lane without a Gaussian passes an empty run.
template <class V>
__device__ __forceinline__ V fold_slot_run(SlotRun run, const V* __restrict__ slots, const uint8_t* __restrict__ touched, int lane)
{
    V acc;
    fold_zero(acc);
    const bool long_run = run.end - run.start > LONG_RUN;
    if (!long_run)
        for (uint32_t s = run.start; s < run.end; s++) {
            if (!touched[s]) continue;
            fold_add(acc, slots[s]);
        }
    for (unsigned long long m = __ballot(long_run); m; m &= m - 1ull) {
        const int src = (int)__ffsll((long long)m) - 1;
        const uint32_t s0 = __shfl(run.start, src), s1 = __shfl(run.end, src);
        V part;
        fold_zero(part);
        // four strides per trip: the four flag bytes are requested together, then the records of the written ones (a
        // trip is two memory round trips whatever it finds; one stride per trip left a 8160-tile run at 128 x 2 of them)
        for (uint32_t s = s0 + (uint32_t)lane; s < s1; s += 256) {
            uint8_t f[4];
#pragma unroll
            for (int k = 0; k < 4; k++) f[k] = (s + 64u * k < s1) ? touched[s + 64u * k] : (uint8_t)0;
            V c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                fold_zero(c[k]);
                if (f[k]) c[k] = slots[s + 64u * k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) fold_add(part, c[k]);   // ascending slots; an unwritten one adds the identity
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fold_add(part, fold_shfl_xor(part, o));
        if (lane == src) acc = part;
    }
    return acc;
}

// ---------------------------------------------------------------- one lane per listed Gaussian
// sum_partials_kernel's lists of blended Gaussians (BWD_LIST entries per list, filled from the front) are walked by grids of
// n_lists * (BWD_LIST / 256) workgroups of 256: backward_preprocess_kernel and the folds behind it. Workgroup -> (list, quarter of
// the list): all FIRST quarters come first in the grid, then all second ones, ... Lists fill from the front, so the populated
// quarters are spread evenly over the XCDs (consecutive workgroups go to consecutive XCDs; quarter = blockIdx % 4 would send every
// full quarter to the same two of the eight) and the mostly empty ones come last.
struct ListedGaussian {
    bool wave_has_work;                               // false: the wave lies past the list's end, return (whole waves only: the
                                                      // shuffles of a fold need every lane, and no workgroup barrier may follow)
    bool live;                                        // this lane has an entry
    size_t pos;                                       // ... at this index of live_ids (and of what else is kept per entry)
    int i;                                            // ... which is this Gaussian (0 for a lane without)
};
__device__ __forceinline__ ListedGaussian listed_gaussian(const uint32_t* __restrict__ live_count, const uint32_t* __restrict__ live_ids)
{
    const uint32_t n_lists = gridDim.x / (BWD_LIST / 256);
    const uint32_t list = blockIdx.x % n_lists, quarter = blockIdx.x / n_lists;
    const uint32_t n_live = live_count[list];
    const uint32_t off = quarter * 256u + threadIdx.x;
    ListedGaussian c = { (off & ~63u) < n_live, off < n_live, (size_t)list * BWD_LIST + off, 0 };
    if (c.live) c.i = (int)live_ids[c.pos];
    return c;
}

// ---------------------------------------------------------------- a view's rows into model-sized accumulators
// Model row i reads view row rank[i] if visible[i] (the pair c3dgs_qat_visible produces), or row i when both are null.
// -1: the view has no row for it.
__device__ __forceinline__ int view_row(int i, const uint8_t* __restrict__ visible, const int32_t* __restrict__ rank, int P_rows)
{
    int row = i;
    if (visible) row = visible[i] ? rank[i] : -1;
    return (row < 0 || row >= P_rows) ? -1 : row;
}

// fmaxf drops a NaN operand: a timed-out view must show
__device__ __forceinline__ float max_keeping_nan(float acc, float v)
{
    return (v != v) ? v : fmaxf(acc, v);
}

} // namespace c3dgs
