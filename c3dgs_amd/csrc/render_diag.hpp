// render_diag.hpp -- the two instruments of the blend kernels (render.hip, which is the only file that includes this).
//
// The kernels call LaneCount and PhaseClock unconditionally. In the product build every method is an empty inline body, so
// the calls (and the ballots that are their arguments) compile to nothing. A diag variant of the library (c3dgs_amd/build.py
// DIAG_VARIANTS: -DC3DGS_DIAG plus one mode flag) makes one of them real:
//   "lanes"   -DC3DGS_COUNT_LANES   LaneCount counts how many pixel lanes use each (wave, Gaussian) pair   tools/lane_efficiency.py
//   "bwdtime" -DC3DGS_BWD_TIMING    PhaseClock sums render_backward's shader-clock ticks per phase          tools/bwd_phases.py
// Both add into g_lane_counters[16]; c3dgs_debug_lane_counters() (diag.hip) reads and clears them. With -fno-gpu-rdc a device
// symbol cannot cross translation units, so the array and its reader live here, in render.hip's translation unit.
#pragma once

namespace c3dgs {

#if (defined(C3DGS_COUNT_LANES) || defined(C3DGS_BWD_TIMING)) && !defined(C3DGS_DIAG)
#error "C3DGS_COUNT_LANES / C3DGS_BWD_TIMING are modes of a -DC3DGS_DIAG build"
#endif

#ifdef C3DGS_DIAG
// "lanes":   [fwd = 0 | bwd = 8] + { 0: (wave, Gaussian) pairs the blend loop ran (real list entries), 1: slots incl. the sentinel
//            padding, 2: lanes whose pixel used the pair (forward: blended it; backward: hit), 3: pairs with at least one such lane,
//            4: sum over (wave, list) of max(pairs touching pixel rows 0-3, pairs touching rows 4-7) = iterations of a half-wave
//               (8x4-pixel) scheduling unit, 5: the same for four 4x4-pixel blocks, 6: lists walked,
//            7: lanes hit (forward, incl. finished pixels) }
// "bwdtime": [PhaseClock::Phase] = ticks of that phase summed over all waves that had work, [9] = their lifetimes, [10] = their number
// All zero in a diag variant that collects neither.
__device__ unsigned long long g_lane_counters[16];

int read_lane_counters(unsigned long long* out16, hipStream_t s)
{
    static const unsigned long long zeros[16] = { 0 };
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_lane_counters), sizeof(zeros)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lane_counters), zeros, sizeof(zeros)) != hipSuccess;
}
#endif

#ifdef C3DGS_COUNT_LANES
struct LaneCount {
    unsigned long long pairs = 0, slots = 0, lanes = 0, live = 0, half = 0, blk = 0, lists = 0, aux = 0;
    int nA = 0, nB = 0, nb[4] = { 0, 0, 0, 0 };
    __device__ void pair(bool real, unsigned long long used, unsigned long long aux_mask)
    {
        slots++;
        if (!real) return;
        pairs++;
        lanes += __popcll(used);
        aux += __popcll(aux_mask);
        live += used != 0;
        nA += (used & 0x00000000ffffffffull) != 0;
        nB += (used & 0xffffffff00000000ull) != 0;
        nb[0] += (used & 0x000000000f0f0f0full) != 0;
        nb[1] += (used & 0x00000000f0f0f0f0ull) != 0;
        nb[2] += (used & 0x0f0f0f0f00000000ull) != 0;
        nb[3] += (used & 0xf0f0f0f000000000ull) != 0;
    }
    __device__ void end_list()
    {
        lists++;
        half += max(nA, nB);
        blk += max(max(nb[0], nb[1]), max(nb[2], nb[3]));
        nA = nB = nb[0] = nb[1] = nb[2] = nb[3] = 0;
    }
    __device__ void flush(int base, int lane)
    {
        if (lane != 0) return;
        const unsigned long long v[8] = { pairs, slots, lanes, live, half, blk, lists, aux };
        for (int q = 0; q < 8; q++) atomicAdd(&g_lane_counters[base + q], v[q]);
    }
};
#else
struct LaneCount {
    __device__ __forceinline__ void pair(bool, unsigned long long, unsigned long long) {}
    __device__ __forceinline__ void end_list() {}
    __device__ __forceinline__ void flush(int, int) {}
};
#endif

// mark(phase): the ticks since the previous mark (or since construction) belong to `phase`
struct PhaseClock {
    enum Phase { PROLOGUE, TOP_BARRIER, GATHER, CLEAR, CLOSE_BARRIER, COMPACT, GROUPS, FLUSH_BARRIER, FLUSH_STORES, NPHASE };
#ifdef C3DGS_BWD_TIMING
    unsigned long long born = __builtin_readcyclecounter(), last = born, sum[NPHASE] = {};
    __device__ void mark(Phase p)
    {
        const unsigned long long now = __builtin_readcyclecounter();
        sum[p] += now - last;
        last = now;
    }
    __device__ void flush(int lane)
    {
        if (lane != 0) return;
        for (int p = 0; p < NPHASE; p++) atomicAdd(&g_lane_counters[p], sum[p]);
        atomicAdd(&g_lane_counters[9], (unsigned long long)__builtin_readcyclecounter() - born);
        atomicAdd(&g_lane_counters[10], 1ull);
    }
#else
    __device__ __forceinline__ void mark(Phase) {}
    __device__ __forceinline__ void flush(int) {}
#endif
};

} // namespace c3dgs
