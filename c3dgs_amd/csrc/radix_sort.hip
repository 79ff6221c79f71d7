// radix_sort.hip -- stable LSD radix sort of (key, u32 value) pairs for the two sorts of the binning stage (gfx950).
//
// Replaces rocPRIM's radix_sort_pairs in run_depth_sort / run_tile_sort (binning.hip keeps the rocPRIM path, selectable
// with C3DGS_SORT_ROCPRIM=1). One read and one write of the data per digit, no global scan pass, written for this workload:
//   * 8192-item tiles of 1024 threads for the u16 tile keys, 12288-item tiles of 512 threads for the u32 depth keys: measured 0.228 ms against 0.267 ms for the 16.4 M (u16, u32) tile-key pairs;
//   * digit widths chosen per sort (13 tile bits = 7 + 6), keys of the native width;
//   * where a tile's digit offsets come from depends on the key width:
//       u16 keys (tile sort up to 65,536 tiles)  TABLE-DRIVEN, every pass: os_tile_hist_kernel counts the pass's digit per tile,
//           os_table_scan_kernel turns the counts into exclusive prefixes over the tiles, os_pass_kernel<.., PRE = true> reads them.
//           No ticket, no look-back (`ticket` is null and `status` is the table in these launches), no control words to clear,
//           no time-out;
//       u32 keys (depth sort; tile sort above 65,536 tiles)  onesweep: os_hist_kernel builds all digit histograms in one read,
//           os_pass_kernel<.., PRE = false> finds the offsets by a chained look-back over the earlier tiles' status words. ONE
//           clear per sort (digit histograms + look-back words + tickets are one contiguous block, normally cleared by the kernel
//           in front of the sort) instead of the two 5-microsecond fill launches rocPRIM issues in front of every digit pass.
//       The forward's depth sort takes its digits from a biased key and runs three 9-bit passes of this kind instead of four 8-bit
//           ones (os_hist3_scan_kernel, onesweep_depth3_head / _tail; the plan is common.hpp's depth_sort_plan).
// Structure of one digit pass (os_pass_kernel), per tile:
//   ticket      (look-back passes only) blocks take their tile index from an atomic counter, so every predecessor of a block is
//               already running (forward progress of the look-back does not depend on the dispatch order); table-driven passes
//               use blockIdx.x;
//   rank        wave w owns a contiguous chunk of the tile and walks it 64 items at a time; lanes with the same digit find
//               each other with BITS ballots, rank = wave counter + popcount(peers below me), the first peer bumps the
//               counter -> ranks are in input order (stable);
//   offsets     table-driven: thread d reads the tile's exclusive prefix of digit d from the table. Look-back: thread d publishes
//               the tile's count of digit d (aggregate), adds up the predecessors' words until it meets an inclusive prefix,
//               publishes its own inclusive prefix (one 32-bit word: 2 flag bits + 30 count bits, relaxed agent-scope atomics);
//   scatter     items are reordered through LDS into tile-sorted order, then written with consecutive threads on
//               consecutive positions of each digit run.
#include "common.hpp"
#include "scan_blocks.hpp"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace c3dgs {

constexpr int OS_RADIX = 256;
// tile shape per key width (measured): u16 keys 8192-item tiles, 1024 threads x 8 items; u32 keys C3DGS_OS_TILE32 items with
// C3DGS_OS_BLOCK32 threads (82 KB of LDS would allow only one 1024-thread workgroup per CU); only the u32 shape is a build knob
#ifndef C3DGS_OS_TILE32
#define C3DGS_OS_TILE32 12288   // round 2 (tools/ablate_sort2.sh, 3M keys): 8192 x 512 0.205 ms, 12288 x 512 0.191, 16384 x 512 0.209, 16384 x 1024 0.194
#endif
#ifndef C3DGS_OS_BLOCK32
#define C3DGS_OS_BLOCK32 512
#endif
// u16 keys: fixed shape. os_tile_hist_kernel (in front of every table-driven pass) counts the SAME tiles with one 16-byte load of
// 8 keys per thread, so tile = 8 x 1024 is not a build knob (measured alternatives before that pre-pass existed, 16.4 M
// (u16, u32) pairs: 8192 x 1024 0.215 ms, 12288 x 1024 0.243, 16384 x 1024 0.225)
constexpr int OS_TILE16 = 8192, OS_BLOCK16 = 1024;
template <class K> struct OsShape {
    static constexpr int TILE = sizeof(K) == 2 ? OS_TILE16 : C3DGS_OS_TILE32;
    static constexpr int BLOCK = sizeof(K) == 2 ? OS_BLOCK16 : C3DGS_OS_BLOCK32;
    static constexpr int IPT = TILE / BLOCK;
};
constexpr uint32_t OS_FLAG_AGG = 1u << 30, OS_FLAG_PRE = 2u << 30, OS_CNT_MASK = (1u << 30) - 1;
constexpr int OS_MAX_PASSES = 4;
// Every look-back spin is bounded (a predecessor's word normally arrives within microseconds; tickets guarantee it is
// running). On time-out the pass finishes with wrong offsets and raises the device's STICKY error word g_os_error, which
//   * render_forward reads: a forward whose sorts timed out returns a NaN image instead of a plausible wrong one;
//   * every forward copies to the host together with num_rendered (the one natural device->host read): the call fails
//     with C3DGS_E_HIP and clears the word (c_abi.hip);
//   * debug mode reads back synchronously after each sort.
// C3DGS_OS_SPIN_LIMIT is a build parameter only so that a test build can force the time-out (tests/test_sort_gpu.py).
#ifndef C3DGS_OS_SPIN_LIMIT
#define C3DGS_OS_SPIN_LIMIT (1u << 22)
#endif
constexpr uint32_t OS_SPIN_LIMIT = C3DGS_OS_SPIN_LIMIT;
__device__ uint32_t g_os_error;           // zero-initialised at module load; bit 0 = tile-key sort, bit 1 = depth-key sort
// Phase stamps of os_pass_kernel (diag variant "ostime": -DC3DGS_DIAG -DC3DGS_OS_TIMING, tools/sort_phases.py): every fourth of the
// first 256 tiles stamps the shader clock at eight phase boundaries. OS_T_LOADS_DONE / OS_T_DRAIN make the memory operations in front
// of a stamp complete before it (the first through a store that never happens but needs the loaded values). All empty in the product.
#ifdef C3DGS_DIAG
__device__ unsigned long long g_os_times[64 * 8];   // stays zero in a diag variant without C3DGS_OS_TIMING
#endif
#ifdef C3DGS_OS_TIMING
#define OS_T(slot) if (tid == 0 && (bid & 3) == 0 && (bid >> 2) < 64) g_os_times[(bid >> 2) * 8 + (slot)] = __builtin_readcyclecounter();
#define OS_T_DRAIN() asm volatile("s_waitcnt vmcnt(0)");
#define OS_T_LOADS_DONE()                                                                                    \
    if (key[0] == (K)0x12345678 && val[OS_IPT - 1] == 0x87654321u) kout[0] = key[OS_IPT - 1];                \
    OS_T_DRAIN()
#else
#define OS_T(slot)
#define OS_T_DRAIN()
#define OS_T_LOADS_DONE()
#endif

struct OsPlan { int passes; int bits[OS_MAX_PASSES]; };

// The depth sort on biased keys (common.hpp: depth_sort_plan / depth_key_biased). A depth key that passed preprocess's near-plane
// test is at least DEPTH_KEY_BIAS, so key - bias has 27 live bits for every depth below 512: three 9-bit digit passes order what
// four 8-bit passes order on the raw pattern. The culled sentinel 0xFFFFFFFF keeps its value, so its three low digits are the top
// of the digit range and it sorts last. A visible key at or above DEPTH_KEY_LIMIT3 needs a fourth pass on the 5 bits above the 27:
// the histogram launch reduces the largest visible key, the host reads it with num_rendered and queues the last pass or two.
constexpr int OS_RADIX3 = 512, OS_BITS3 = 9, OS_BITS3_TOP = 32 - 3 * OS_BITS3;
static_assert(OS_RADIX3 == C3DGS_OS_BLOCK32, "one thread per digit in the biased depth sort's passes");
static_assert(OS_RADIX3 == (1 << DEPTH_SORT3_BITS) && 3 * OS_BITS3 == 27 && DEPTH_KEY_LIMIT3 == DEPTH_KEY_BIAS + (1u << 27) - 1u, "common.hpp's plan");
template <bool XF> __device__ __forceinline__ uint32_t os_digit_src(uint32_t k) { return XF ? depth_key_biased(k) : k; }

// Measured for the two table-driven passes of the 13-bit tile sort (16.4 M pairs, whole sort): 7 + 6 153.6 us, 6 + 7 154.4 us,
// 8 + 5 158.9 us -- an 8-bit pass costs 8 us more than a 7-bit one (scatter runs half as long), a 5-bit pass saves 5 us on a 6-bit one
static OsPlan os_plan(int total_bits)
{
    OsPlan p;
    p.passes = (total_bits + 7) / 8;
    if (p.passes < 1) p.passes = 1;
    int left = total_bits < 1 ? 1 : total_bits;
    for (int i = 0; i < p.passes; i++) {                    // spread the bits evenly: 13 -> 7 + 6
        const int b = (left + (p.passes - i) - 1) / (p.passes - i);
        p.bits[i] = b;
        left -= b;
    }
    return p;
}

template <class K> static size_t os_blocks(size_t n) { return (n + OsShape<K>::TILE - 1) / OsShape<K>::TILE; }
// The tile-key sort (u16 keys, at most two passes) runs EVERY pass without the chained look-back: in front of the pass a histogram
// kernel counts the pass's digit tile by tile over the pass's input and leaves the counts in a table, one small kernel turns the
// table's columns into exclusive prefixes over the tiles (and their totals into the pass's global histogram), and the pass reads
// its offsets from there. Measured on the 16.4 M pairs of the bench view: the look-back costs ~30 us per pass at 2002 tiles
// (tools/time_sort.py knock-out), the histogram + scan of one digit about half of that.
// Control block: u16 keys  [global histograms: passes x 256 | table: 256 columns x tiles, reused by the second pass];
//                u32 keys  [global histograms: passes x 256 | look-back words: passes x tiles x 256 | 64 tickets].
template <class K> constexpr bool os_table_driven() { return sizeof(K) == 2; }
template <class K> static size_t os_table_words(size_t n) { return os_table_driven<K>() ? os_blocks<K>(n) * OS_RADIX : 0; }
template <class K> static size_t os_lookback_words(size_t n, int passes)
{
    return os_table_driven<K>() ? 0 : (size_t)passes * os_blocks<K>(n) * OS_RADIX + 64;
}
template <class K> static size_t os_ctrl_bytes(size_t n, int passes)
{
    return align_up(((size_t)passes * OS_RADIX + os_lookback_words<K>(n, passes) + os_table_words<K>(n)) * sizeof(uint32_t));
}

// all digit histograms in one read of the keys: 1024-thread workgroups (at most 512 of them, so the final flush stays a
// few hundred atomics per global bin), four independent 16-byte loads in flight per thread. `block` of `nblocks` workgroups.
constexpr int OS_HIST_BLOCK = 1024;
template <class K>
__device__ __forceinline__ void os_hist_body(const K* __restrict__ keys, size_t n, const OsPlan& plan, uint32_t* __restrict__ hist,
                                             unsigned block, unsigned nblocks)
{
    __shared__ uint32_t s_h[OS_MAX_PASSES][OS_RADIX];
    for (int q = threadIdx.x; q < OS_MAX_PASSES * OS_RADIX; q += OS_HIST_BLOCK) (&s_h[0][0])[q] = 0;
    __syncthreads();
    constexpr int VEC = 16 / sizeof(K);                     // keys per 16-byte load
    const size_t nvec = n / VEC;
    const uint4* k4 = reinterpret_cast<const uint4*>(keys);
    auto add = [&](uint32_t k) {
        int shift = 0;
        for (int p = 0; p < plan.passes; p++) {
            atomicAdd(&s_h[p][(k >> shift) & ((1u << plan.bits[p]) - 1u)], 1u);
            shift += plan.bits[p];
        }
    };
    auto add4 = [&](const uint4 v) {
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (sizeof(K) == 4) add(w[e]);
            else { add(w[e] & 0xffffu); add(w[e] >> 16); }
        }
    };
    const size_t stride = (size_t)nblocks * OS_HIST_BLOCK;
    size_t i = (size_t)block * OS_HIST_BLOCK + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const uint4 v0 = k4[i], v1 = k4[i + stride], v2 = k4[i + 2 * stride], v3 = k4[i + 3 * stride];
        add4(v0); add4(v1); add4(v2); add4(v3);
    }
    for (; i < nvec; i += stride) add4(k4[i]);
    for (size_t j = nvec * VEC + (size_t)block * OS_HIST_BLOCK + threadIdx.x; j < n; j += stride) add((uint32_t)keys[j]);
    __syncthreads();
    for (int q = threadIdx.x; q < plan.passes * OS_RADIX; q += OS_HIST_BLOCK) {
        const uint32_t v = (&s_h[0][0])[q];
        if (v) atomicAdd(&hist[q], v);
    }
}

template <class K>
__global__ void __launch_bounds__(OS_HIST_BLOCK) os_hist_kernel(const K* __restrict__ keys, size_t n, OsPlan plan, uint32_t* __restrict__ hist)
{
    os_hist_body<K>(keys, n, plan, hist, blockIdx.x, gridDim.x);
}

// The depth sort's histograms and the id-order scan of the instance totals (scan_blocks.hpp) in ONE launch: both read only what
// preprocess wrote and neither reads the other's output, but alone each is a launch-latency-bound kernel that holds the whole
// chip. Workgroup 0 runs the scan (and its mapped-host-memory store of num_rendered, unchanged and as early as before), workgroups
// 1 .. gridDim.x - 1 the histogram. No hand-off: the two bodies sit side by side, each with its own LDS (4 KB + 128 B).
static_assert(SCAN_BLOCKS_THREADS == OS_HIST_BLOCK, "one workgroup shape for both bodies");
__global__ void __launch_bounds__(OS_HIST_BLOCK)
os_hist_scan_kernel(const uint32_t* __restrict__ keys, size_t n, OsPlan plan, uint32_t* __restrict__ hist, int nb, uint32_t* __restrict__ base,
                    const uint32_t* __restrict__ sort_err, uint32_t* __restrict__ host_out, uint32_t host_seq)
{
    if (blockIdx.x == 0) scan_blocks_body(nb, base, sort_err, host_out, host_seq);
    else os_hist_body<uint32_t>(keys, n, plan, hist, blockIdx.x - 1, gridDim.x - 1);
}

// The biased depth sort's histogram: three 9-bit digits of the transformed key and the largest visible key, one read of the keys.
// Control words behind the look-back words (os3_layout): `maxw` takes every workgroup's largest visible key, `done` counts the
// workgroups that have added theirs; the one that counts last stores the result to the mapped host words {max key, host_seq}
// (`host_max`, optional). Nobody waits for anybody: the last arrival is whoever it is.
__device__ __forceinline__ void os_hist3_body(const uint32_t* __restrict__ keys, size_t n, uint32_t* __restrict__ hist, uint32_t* __restrict__ maxw,
                                              uint32_t* __restrict__ done, uint32_t* __restrict__ host_max, uint32_t host_seq,
                                              unsigned block, unsigned nblocks)
{
    __shared__ uint32_t s_h[3][OS_RADIX3];
    __shared__ uint32_t s_max;
    for (int q = threadIdx.x; q < 3 * OS_RADIX3; q += OS_HIST_BLOCK) (&s_h[0][0])[q] = 0;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    uint32_t mx = 0;
    auto add = [&](uint32_t k) {
        const uint32_t t = depth_key_biased(k);
        atomicAdd(&s_h[0][t & (OS_RADIX3 - 1)], 1u);
        atomicAdd(&s_h[1][(t >> OS_BITS3) & (OS_RADIX3 - 1)], 1u);
        atomicAdd(&s_h[2][(t >> (2 * OS_BITS3)) & (OS_RADIX3 - 1)], 1u);
        if (k != DEPTH_KEY_CULLED) mx = max(mx, k);
    };
    auto add4 = [&](const uint4 v) { add(v.x); add(v.y); add(v.z); add(v.w); };
    const size_t nvec = n / 4;
    const uint4* k4 = reinterpret_cast<const uint4*>(keys);
    const size_t stride = (size_t)nblocks * OS_HIST_BLOCK;
    size_t i = (size_t)block * OS_HIST_BLOCK + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const uint4 v0 = k4[i], v1 = k4[i + stride], v2 = k4[i + 2 * stride], v3 = k4[i + 3 * stride];
        add4(v0); add4(v1); add4(v2); add4(v3);
    }
    for (; i < nvec; i += stride) add4(k4[i]);
    for (size_t j = nvec * 4 + (size_t)block * OS_HIST_BLOCK + threadIdx.x; j < n; j += stride) add(keys[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&s_max, mx);
    __syncthreads();
    for (int q = threadIdx.x; q < 3 * OS_RADIX3; q += OS_HIST_BLOCK) {
        const uint32_t v = (&s_h[0][0])[q];
        if (v) atomicAdd(&hist[q], v);
    }
    if (threadIdx.x == 0) {
        if (s_max) __hip_atomic_fetch_max(maxw, s_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t before = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before == nblocks - 1 && host_max) {
            const uint32_t m = __hip_atomic_load(maxw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(host_max, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_max + 1, host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // publishes the word above
        }
    }
}

// as os_hist_scan_kernel, for the biased depth sort: workgroup 0 the id-order scan and its num_rendered store, the others the histogram
__global__ void __launch_bounds__(OS_HIST_BLOCK)
os_hist3_scan_kernel(const uint32_t* __restrict__ keys, size_t n, uint32_t* __restrict__ hist, uint32_t* __restrict__ maxw, uint32_t* __restrict__ done,
                     uint32_t* __restrict__ host_max, int nb, uint32_t* __restrict__ base, const uint32_t* __restrict__ sort_err,
                     uint32_t* __restrict__ host_out, uint32_t host_seq)
{
    if (blockIdx.x == 0) scan_blocks_body(nb, base, sort_err, host_out, host_seq);
    else os_hist3_body(keys, n, hist, maxw, done, host_max, host_seq, blockIdx.x - 1, gridDim.x - 1);
}

// the fourth pass's histogram (the 5 bits above the 27), launched only where the largest visible key asks for that pass: most keys
// share a digit, so a wave counts its lanes per distinct digit with a ballot and adds once
__global__ void __launch_bounds__(OS_HIST_BLOCK) os_hist3_top_kernel(const uint32_t* __restrict__ keys, size_t n, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_h[1 << OS_BITS3_TOP];
    if (threadIdx.x < (1 << OS_BITS3_TOP)) s_h[threadIdx.x] = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * OS_HIST_BLOCK;
    const size_t rounds = (n + stride - 1) / stride;                 // uniform trip count: every lane takes part in the ballots
    for (size_t r = 0; r < rounds; r++) {
        const size_t i = r * stride + (size_t)blockIdx.x * OS_HIST_BLOCK + threadIdx.x;
        const bool ok = i < n;
        const uint32_t d = ok ? depth_key_biased(keys[i]) >> (3 * OS_BITS3) : 0u;
        unsigned long long left = __ballot(ok);
        while (left) {
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t dl = (uint32_t)__shfl((int)d, leader);
            const unsigned long long same = __ballot(ok && d == dl) & left;
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&s_h[dl], (uint32_t)__popcll(same));
            left &= ~same;
        }
    }
    __syncthreads();
    if (threadIdx.x < (1 << OS_BITS3_TOP) && s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// tile-by-tile histogram of ONE digit of the u16 sort: workgroup b counts the digit (bits [shift, shift + bits)) over tile b of
// `keys` (the tile b of the pass kernel that reads the same keys) and stores the counts as row b of the table -- plain stores, no
// global atomics (the closing atomics of os_hist_kernel are what makes it slower with more workgroups)
__global__ void __launch_bounds__(1024) os_tile_hist_kernel(const uint16_t* __restrict__ keys, uint32_t n, int shift, int bits, uint32_t* __restrict__ table)
{
    constexpr int TILE = OsShape<uint16_t>::TILE;
    static_assert(TILE == 8 * 1024, "one 16-byte load of 8 keys per thread");
    __shared__ uint32_t s_h[OS_RADIX];
    if (threadIdx.x < OS_RADIX) s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)TILE + threadIdx.x * 8u;
    const uint32_t mask = (1u << bits) - 1u;
    auto add = [&](uint32_t k) { atomicAdd(&s_h[(k >> shift) & mask], 1u); };
    if (base + 8 <= n && (reinterpret_cast<uintptr_t>(keys) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(keys + base);
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int e = 0; e < 4; e++) { add(w[e] & 0xffffu); add(w[e] >> 16); }
    } else {
        for (uint32_t i = base; i < min(base + 8u, n); i++) add((uint32_t)keys[i]);
    }
    __syncthreads();
    // column-major table (a column = one digit over all tiles, contiguous for the scan); unused digit columns stay unwritten
    const int t = threadIdx.x;
    if (t < (1 << bits)) table[(size_t)t * gridDim.x + blockIdx.x] = s_h[t];
}

// one workgroup per USED table column (digit) of the pass: the column is replaced by its exclusive prefixes over the tiles (what
// the look-back would have produced) and its total goes to `hist`, the global histogram of that pass (256 words, all written:
// the unused digits get zero, so the sort needs no cleared control words). A thread owns OS_SCAN_V consecutive tiles, so a sweep
// covers 2048 tiles (16.8 M items) with one memory round trip and two barriers: the kernel is latency, not bytes.
constexpr int OS_SCAN_V = 8;
__global__ void __launch_bounds__(256) os_table_scan_kernel(uint32_t* __restrict__ table, uint32_t blocks, uint32_t* __restrict__ hist)
{
    static_assert(OS_RADIX == 256, "one thread per histogram word");
    __shared__ uint32_t s_w[4];
    const int digit = (int)blockIdx.x;                              // gridDim.x = digits in use
    uint32_t* column = table + (size_t)digit * blocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (digit == 0 && threadIdx.x >= gridDim.x) hist[threadIdx.x] = 0u;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < blocks; b0 += 256 * OS_SCAN_V) {
        const uint32_t b = b0 + threadIdx.x * OS_SCAN_V;
        uint32_t c[OS_SCAN_V], mine = 0;
#pragma unroll
        for (int q = 0; q < OS_SCAN_V; q++) { c[q] = b + q < blocks ? column[b + q] : 0u; mine += c[q]; }
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        __syncthreads();                                            // previous sweep's s_w has been read
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t run = carry + incl - mine;
        for (int w = 0; w < wave; w++) run += s_w[w];
#pragma unroll
        for (int q = 0; q < OS_SCAN_V; q++) { if (b + q < blocks) column[b + q] = run; run += c[q]; }
        carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
    if (threadIdx.x == 0) hist[digit] = carry;
}

__device__ __forceinline__ uint32_t os_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void os_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// PRE: the tile's exclusive digit prefixes come from the table os_table_scan_kernel prepared for this pass (`status` = the table,
// no ticket, no look-back); otherwise they are found by the chained look-back over the earlier tiles' status words.
// PAY2 (depth sort): a SECOND 32-bit payload travels with every item -- the Gaussian's tile rectangle packed to four bytes
// (os_pack_rect: grids up to 255 x 255 tiles). The first pass reads the rectangles coalesced, in id order, from `gather_src`
// (p2in == null); the passes hand the packed word on through p2in / p2out; the last pass (p2out == null) unpacks it into
// gather_dst in sorted order. Without it the last pass GATHERS gather_src[id]: 3M random 8-byte reads = 3M x 128-byte lines,
// 42 us at the fabric's line rate for P = 3M (tools/step_timeline.py) against ~4 us more per pass for the extra payload.
__device__ __forceinline__ uint32_t os_pack_rect(uint2 r)
{
    return (r.x & 0xffu) | ((r.x >> 16) << 8) | ((r.y & 0xffu) << 16) | ((r.y >> 16) << 24);
}
__device__ __forceinline__ uint2 os_unpack_rect(uint32_t w)
{
    return make_uint2((w & 0xffu) | (((w >> 8) & 0xffu) << 16), ((w >> 16) & 0xffu) | ((w >> 24) << 16));
}

// RADIX / XF (depth sort on biased keys, see os_depth_xf): RADIX = 512 gives every one of the 512 threads a digit; its per-wave
// counters are 16 bits wide (a wave owns TILE / waves = 1536 items, a tile 12288: both below 65,536), which is what keeps the PAY2
// instantiation inside the LDS. XF: the digit is taken from the transformed key; the keys that travel and are stored stay as they are.
template <class K, int BITS, bool PRE, bool PAY2 = false, int RADIX = OS_RADIX, bool XF = false>
__global__ void __launch_bounds__(OsShape<K>::BLOCK)
os_pass_kernel(const K* __restrict__ kin, K* __restrict__ kout, const uint32_t* __restrict__ vin, uint32_t* __restrict__ vout,
               uint32_t n, int shift, const uint32_t* __restrict__ hist, uint32_t* __restrict__ status, uint32_t* __restrict__ ticket,
               const uint2* __restrict__ gather_src, uint2* __restrict__ gather_dst, const uint32_t* __restrict__ p2in = nullptr,
               uint32_t* __restrict__ p2out = nullptr)
{
    constexpr uint32_t ERR_BIT = sizeof(K) == 2 ? 1u : 2u;
    constexpr uint32_t MASK = (1u << BITS) - 1;
    constexpr int OS_BLOCK = OsShape<K>::BLOCK, OS_IPT = OsShape<K>::IPT, OS_WAVES = OS_BLOCK / 64;
    constexpr int OS_TILE = OsShape<K>::TILE;
    using CNT = typename std::conditional<(RADIX > 256), uint16_t, uint32_t>::type;
    static_assert(RADIX % 64 == 0 && RADIX <= OS_BLOCK && BITS <= 9 && (1 << BITS) <= RADIX, "one thread per digit");
    static_assert(!XF || sizeof(K) == 4, "the transform is the depth keys'");
    static_assert(sizeof(CNT) == 4 || OS_TILE < 65536, "a 16-bit counter holds up to a tile's items");
    static_assert(sizeof(CNT) * OS_WAVES * RADIX + 8 * RADIX + 4 * (RADIX / 64) + 4 + sizeof(K) * OS_TILE + 4 * OS_TILE * (PAY2 ? 2 : 1) + (PAY2 ? 0 : 4)
                      <= 160 * 1024, "LDS of one workgroup (160 KB per CU)");
    __shared__ CNT s_cnt[OS_WAVES][RADIX];        // per-wave digit counters, later exclusive prefixes across the waves
    __shared__ uint32_t s_start[RADIX];           // start of every digit in the tile-sorted order
    __shared__ int32_t s_gbase[RADIX];            // global position = s_gbase[digit] + tile-sorted position
    __shared__ uint32_t s_wtot[RADIX / 64];
    __shared__ uint32_t s_bid;
    __shared__ K s_keys[OS_TILE];
    __shared__ uint32_t s_vals[OS_TILE];
    __shared__ uint32_t s_vals2[PAY2 ? OS_TILE : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_bid = PRE ? blockIdx.x : atomicAdd(ticket, 1u);
    for (int q = tid; q < OS_WAVES * RADIX; q += OS_BLOCK) (&s_cnt[0][0])[q] = 0;
    __syncthreads();
    const uint32_t bid = s_bid;
    OS_T(0)
    const uint32_t block_start = bid * (uint32_t)OS_TILE;
    const uint32_t valid = min((uint32_t)OS_TILE, n - block_start);

    K key[OS_IPT];
    uint32_t val[OS_IPT], rank[OS_IPT];
    uint32_t val2[PAY2 ? OS_IPT : 1];
    const uint32_t wbase = block_start + (uint32_t)wave * 64u * OS_IPT;
#pragma unroll
    for (int k = 0; k < OS_IPT; k++) {
        const uint32_t idx = wbase + (uint32_t)k * 64u + lane;
        const bool ok = idx < n;
        key[k] = ok ? kin[idx] : (K)0;
        val[k] = ok ? (vin ? vin[idx] : idx) : 0u;             // no payload array: the payload is the item's index
        if (PAY2) val2[k] = ok ? (p2in ? p2in[idx] : os_pack_rect(gather_src[idx])) : 0u;
    }
    // ranking: lanes with the same digit find each other with BITS ballots. Written on 32-bit halves with the digit bit as a
    // 0 / -1 mask so that a bit costs six vector instructions (v_bfe_i32, v_cmp, 2 x v_xnor, 2 x v_and); the obvious
    // `peers &= bit ? bal : ~bal` compiled to 16 (two compares per bit, a 64-bit select built from v_cndmask + v_lshl_add_u64).
    // The per-wave digit counters are read and bumped through plain LDS instructions (wavefront-scope relaxed atomics): a
    // `volatile` pointer made them FLAT loads / stores with system-scope cache bits and a full vmcnt(0) wait each -- two memory
    // round trips per item, which was most of this loop's time (tools/sort_phases.py: rank loop 47 % of a depth-key pass).
    const uint32_t lt_lo = lane < 32 ? (1u << lane) - 1u : 0xffffffffu, lt_hi = lane < 32 ? 0u : (1u << (lane - 32)) - 1u;
    OS_T_LOADS_DONE()
    OS_T(1)
    CNT* wc = s_cnt[wave];                       // other lanes of the wave update these between iterations
#pragma unroll
    for (int k = 0; k < OS_IPT; k++) {
        const uint32_t idx = wbase + (uint32_t)k * 64u + lane;
        const bool ok = idx < n;
        const uint32_t d = (os_digit_src<XF>((uint32_t)key[k]) >> shift) & MASK;
        const unsigned long long okb = __ballot(ok);  // padding lanes of the last tile take no part
        uint32_t plo = (uint32_t)okb, phi = (uint32_t)(okb >> 32);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            const int sgn = __builtin_amdgcn_sbfe((int)d, b, 1);                      // 0 or -1
            const unsigned long long bal = __ballot(sgn != 0);
            plo &= ~((uint32_t)bal ^ (uint32_t)sgn);                                   // bit set: keep bal; clear: keep ~bal
            phi &= ~((uint32_t)(bal >> 32) ^ (uint32_t)sgn);
        }
        rank[k] = 0;
        if (ok) {
            const uint32_t before = __hip_atomic_load(&wc[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            const uint32_t below = (uint32_t)__popc(plo & lt_lo) + (uint32_t)__popc(phi & lt_hi);
            rank[k] = before + below;
            if (below == 0) __hip_atomic_store(&wc[d], (CNT)(before + (uint32_t)__popc(plo) + (uint32_t)__popc(phi)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    OS_T(2)
    __syncthreads();
    OS_T(3)
    // thread d (< RADIX): the tile's count of digit d, exclusive prefixes across the waves, then across the digits
    uint32_t tot = 0;
    if (tid < RADIX) {
#pragma unroll
        for (int w = 0; w < OS_WAVES; w++) { const uint32_t c = s_cnt[w][tid]; s_cnt[w][tid] = (CNT)tot; tot += c; }
    }
    uint32_t incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (tid < RADIX && lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    uint32_t start = 0, pre = 0;
    if (tid < RADIX) {
        uint32_t off = 0;
        for (int w = 0; w < wave; w++) off += s_wtot[w];
        start = off + incl - tot;
        s_start[tid] = start;
        // decoupled look-back over the earlier tiles for digit `tid`
        uint32_t* my = status + (size_t)bid * RADIX + tid;
        if (PRE) pre = tid < (1 << BITS) ? status[(size_t)tid * gridDim.x + bid] : 0u;   // column-major table of this pass's digit
        else if (bid == 0) os_store(my, OS_FLAG_PRE | tot);
        else {
            os_store(my, OS_FLAG_AGG | tot);
            for (int64_t b = (int64_t)bid - 1;; b--) {
                uint32_t s, spins = 0;
                do { s = os_load(status + (size_t)b * RADIX + tid); } while ((s >> 30) == 0 && ++spins < OS_SPIN_LIMIT);
                if ((s >> 30) == 0) { atomicOr(&g_os_error, ERR_BIT); break; }   // never hang the device: give up, flag it
                pre += s & OS_CNT_MASK;
                if (s & OS_FLAG_PRE) break;
            }
            os_store(my, OS_FLAG_PRE | (pre + tot));
        }
    }
    OS_T(4)
    // exclusive scan of the global digit histogram by the same RADIX threads
    const uint32_t h = tid < RADIX ? hist[tid] : 0u;
    uint32_t hincl = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(hincl, o); if (lane >= o) hincl += t; }
    __syncthreads();
    if (tid < RADIX && lane == 63) s_wtot[wave] = hincl;
    __syncthreads();
    if (tid < RADIX) {
        uint32_t off = 0;
        for (int w = 0; w < wave; w++) off += s_wtot[w];
        s_gbase[tid] = (int32_t)(off + hincl - h + pre) - (int32_t)start;
    }
    OS_T(5)
    // stable reorder of the tile through LDS
#pragma unroll
    for (int k = 0; k < OS_IPT; k++) {
        const uint32_t idx = wbase + (uint32_t)k * 64u + lane;
        if (idx < n) {
            const uint32_t d = (os_digit_src<XF>((uint32_t)key[k]) >> shift) & MASK;
            const uint32_t p = s_start[d] + s_cnt[wave][d] + rank[k];
            s_keys[p] = key[k];
            s_vals[p] = val[k];
            if (PAY2) s_vals2[p] = val2[k];
        }
    }
    __syncthreads();
    OS_T(6)
#pragma unroll
    for (int m = 0; m < OS_IPT; m++) {
        const uint32_t p = (uint32_t)tid + (uint32_t)m * OS_BLOCK;
        if (p < valid) {
            const K kk = s_keys[p];
            const uint32_t d = (os_digit_src<XF>((uint32_t)kk) >> shift) & MASK;
            const uint32_t g = (uint32_t)(s_gbase[d] + (int32_t)p);
            kout[g] = kk;
            const uint32_t vv = s_vals[p];
            vout[g] = vv;
            if (PAY2) {
                if (p2out) p2out[g] = s_vals2[p];
                else gather_dst[g] = os_unpack_rect(s_vals2[p]);   // last pass: the rectangles arrive with their items
            } else if (gather_src) gather_dst[g] = gather_src[vv]; // last pass of the depth sort: per-Gaussian data in sorted order
        }
    }
    OS_T_DRAIN()
    OS_T(7)
}

template <class K, bool PRE>
static void os_launch_pass(int bits, unsigned blocks, hipStream_t s, const K* ki, K* ko, const uint32_t* vi, uint32_t* vo, uint32_t n,
                           int shift, const uint32_t* hist, uint32_t* status, uint32_t* ticket, const uint2* gsrc, uint2* gdst)
{
#define C3DGS_OS_CASE(B) case B: os_pass_kernel<K, B, PRE><<<blocks, OsShape<K>::BLOCK, 0, s>>>(ki, ko, vi, vo, n, shift, hist, status, ticket, gsrc, gdst); break
    switch (bits) {
        C3DGS_OS_CASE(1); C3DGS_OS_CASE(2); C3DGS_OS_CASE(3); C3DGS_OS_CASE(4);
        C3DGS_OS_CASE(5); C3DGS_OS_CASE(6); C3DGS_OS_CASE(7);
        default: os_pass_kernel<K, 8, PRE><<<blocks, OsShape<K>::BLOCK, 0, s>>>(ki, ko, vi, vo, n, shift, hist, status, ticket, gsrc, gdst); break;
    }
#undef C3DGS_OS_CASE
}

// 4 x 16 bytes per thread, at most 512 workgroups: measured optimum on both sorts (fewer workgroups: LDS-atomic bound;
// more: the closing global atomics, one per workgroup and non-empty bin on the same few hundred words, take over)
template <class K> static unsigned os_hist_blocks(size_t n)
{
    const size_t nvec16 = n * sizeof(K) / 16 + 1;
    return (unsigned)std::min<size_t>((nvec16 + OS_HIST_BLOCK * 4 - 1) / (OS_HIST_BLOCK * 4), 512);
}

// temp = [control block | ping buffer (keys, values) | pong buffer]; the input arrays are never written
template <class K>
static size_t os_temp_bytes(size_t n, int total_bits, bool pay2 = false)
{
    const OsPlan plan = os_plan(total_bits);
    size_t b = os_ctrl_bytes<K>(n, plan.passes);
    const int bufs = plan.passes >= 3 ? 2 : (plan.passes == 2 ? 1 : 0);
    b += (size_t)bufs * (align_up(n * sizeof(K)) + align_up(n * sizeof(uint32_t)));
    if (pay2) b += 2 * align_up(n * sizeof(uint32_t));       // ping-pong of the second payload, behind everything else
    return b;
}

// the control words at the front of `temp` that must be ZERO when the sort starts (digit histograms the histogram kernel adds
// into, look-back status words, tickets). os_sort clears them itself unless the caller says a kernel it ran just before on the
// same stream already did (`ctrl_cleared`: the rasterizer folds the two clears of a forward into preprocess / duplicate_with_keys,
// whose thousands of workgroups do it for free -- a separate fill launch costs ~5 us of an otherwise idle GPU each).
// The table-driven sort has none: its histograms and its table are written in full with plain stores before they are read.
template <class K>
static size_t os_clear_bytes(size_t n, int total_bits)
{
    if (os_table_driven<K>()) return 0;
    return os_ctrl_bytes<K>(n, os_plan(total_bits).passes);
}

template <class K>
static hipError_t os_sort(void* temp, size_t temp_bytes, const K* kin, K* kout, const uint32_t* vin, uint32_t* vout, size_t n,
                          int total_bits, hipStream_t s, const uint2* gather_src = nullptr, uint2* gather_dst = nullptr,
                          bool ctrl_cleared = false, bool pay2 = false, bool hist_done = false)
{
    if (n == 0) return hipSuccess;
    // second payload (see os_pass_kernel): u32 keys in four 8-bit passes with a rectangle table only, and only if the caller's
    // scratch has room for its two buffers
    if (pay2 && (sizeof(K) != 4 || total_bits != 32 || !gather_src || !gather_dst || vin || os_temp_bytes<K>(n, total_bits, true) > temp_bytes))
        pay2 = false;
    if (n >= ((size_t)1 << 30) || total_bits > 8 * (int)sizeof(K) || os_temp_bytes<K>(n, total_bits) > temp_bytes) return hipErrorInvalidValue;
    const OsPlan plan = os_plan(total_bits);
    const size_t blocks = os_blocks<K>(n);
    char* base = (char*)temp;
    const size_t ctrl = os_ctrl_bytes<K>(n, plan.passes);
    uint32_t* hist = (uint32_t*)base;                               // [passes][OS_RADIX]
    uint32_t* behind_hist = hist + (size_t)plan.passes * OS_RADIX;
    K* tk[2]; uint32_t* tv[2];
    char* q = base + ctrl;
    for (int i = 0; i < 2; i++) { tk[i] = (K*)q; q += align_up(n * sizeof(K)); tv[i] = (uint32_t*)q; q += align_up(n * sizeof(uint32_t)); }
    if constexpr (os_table_driven<K>()) {
        // per pass: count the pass's digit per tile of the pass's input, scan the table's columns, scatter from the table. The one
        // table is reused: the stream orders a pass behind its scan and the next histogram behind the pass.
        uint32_t* table = behind_hist;                              // [digit columns][blocks]
        int shift = 0;
        for (int p = 0; p < plan.passes; p++) {
            const bool last = p == plan.passes - 1;
            const K* ki = p == 0 ? kin : tk[(p - 1) & 1];
            const uint32_t* vi = p == 0 ? vin : tv[(p - 1) & 1];
            uint32_t* h = hist + (size_t)p * OS_RADIX;
            os_tile_hist_kernel<<<(unsigned)blocks, 1024, 0, s>>>((const uint16_t*)ki, (uint32_t)n, shift, plan.bits[p], table);
            os_table_scan_kernel<<<1u << plan.bits[p], 256, 0, s>>>(table, (uint32_t)blocks, h);
            os_launch_pass<K, true>(plan.bits[p], (unsigned)blocks, s, ki, last ? kout : tk[p & 1], vi, last ? vout : tv[p & 1], (uint32_t)n,
                                    shift, h, table, nullptr, last ? gather_src : nullptr, last ? gather_dst : nullptr);
            shift += plan.bits[p];
        }
        return hipGetLastError();
    } else {
        uint32_t* status = behind_hist;                             // [passes][blocks][OS_RADIX]
        uint32_t* ticket = status + (size_t)plan.passes * blocks * OS_RADIX;
        uint32_t* t2[2] = { nullptr, nullptr };
        if (pay2) {
            q = base + os_temp_bytes<K>(n, total_bits);
            for (int i = 0; i < 2; i++) { t2[i] = (uint32_t*)q; q += align_up(n * sizeof(uint32_t)); }
        }
        if (!ctrl_cleared) {
            const hipError_t e = hipMemsetAsync(base, 0, os_clear_bytes<K>(n, total_bits), s);
            if (e != hipSuccess) return e;
        }
        // hist_done: the caller has run the histogram on cleared control words already (onesweep_depth_hist_scan)
        if (!hist_done) os_hist_kernel<K><<<os_hist_blocks<K>(n), OS_HIST_BLOCK, 0, s>>>(kin, n, plan, hist);
        int shift = 0;
        for (int p = 0; p < plan.passes; p++) {
            const K* ki = p == 0 ? kin : tk[(p - 1) & 1];
            const uint32_t* vi = p == 0 ? vin : tv[(p - 1) & 1];
            K* ko = p == plan.passes - 1 ? kout : tk[p & 1];
            uint32_t* vo = p == plan.passes - 1 ? vout : tv[p & 1];
            const bool last = p == plan.passes - 1;
            // ticket + p is this pass's counter
            if (pay2)
                os_pass_kernel<K, 8, false, true><<<(unsigned)blocks, OsShape<K>::BLOCK, 0, s>>>(
                    ki, ko, vi, vo, (uint32_t)n, shift, hist + (size_t)p * OS_RADIX, status + (size_t)p * blocks * OS_RADIX, ticket + p,
                    gather_src, gather_dst, p == 0 ? nullptr : t2[(p - 1) & 1], last ? nullptr : t2[p & 1]);
            else
                os_launch_pass<K, false>(plan.bits[p], (unsigned)blocks, s, ki, ko, vi, vo, (uint32_t)n, shift, hist + (size_t)p * OS_RADIX,
                                         status + (size_t)p * blocks * OS_RADIX, ticket + p, last ? gather_src : nullptr, last ? gather_dst : nullptr);
            shift += plan.bits[p];
        }
        return hipGetLastError();
    }
}

// ---- the depth sort on biased keys: scratch layout and the two halves of the sort around the forward's host read
// control block (all cleared by the caller's earlier kernel, onesweep_depth_clear_bytes):
//   [histograms: 3 x 512 | 256 | look-back words: 3 x tiles x 512 | tiles x 256 | 64 words: tickets 0..3, 8 = max visible key, 9 = done]
// then the two (key, id) buffers and the two second-payload buffers, as os_sort lays them out.
struct Os3Layout {
    size_t blocks, ctrl_bytes, total_bytes;
    uint32_t *hist[4], *status[4], *ticket, *maxw, *done;
    uint32_t *tk[2], *tv[2], *t2[2];
};
static Os3Layout os3_layout(void* temp, size_t n)
{
    Os3Layout L;
    L.blocks = os_blocks<uint32_t>(n);
    const size_t hist_words = 3 * OS_RADIX3 + OS_RADIX, status_words = L.blocks * hist_words;
    L.ctrl_bytes = align_up((hist_words + status_words + 64) * sizeof(uint32_t));
    uint32_t* w = (uint32_t*)temp;
    for (int p = 0; p < 4; p++) {
        L.hist[p] = w + (size_t)p * OS_RADIX3;
        L.status[p] = w + hist_words + (size_t)p * L.blocks * OS_RADIX3;
    }
    L.ticket = w + hist_words + status_words;
    L.maxw = L.ticket + 8;
    L.done = L.ticket + 9;
    char* q = (char*)temp + L.ctrl_bytes;
    const size_t a = align_up(n * sizeof(uint32_t));
    for (int i = 0; i < 2; i++) { L.tk[i] = (uint32_t*)q; q += a; L.tv[i] = (uint32_t*)q; q += a; }
    for (int i = 0; i < 2; i++) { L.t2[i] = (uint32_t*)q; q += a; }
    L.total_bytes = (size_t)(q - (char*)temp);
    return L;
}
static bool os3_args_ok(size_t temp_bytes, int P)
{
    return P > 0 && (size_t)P < ((size_t)1 << 30) && os3_layout(nullptr, (size_t)P).total_bytes <= temp_bytes;
}

hipError_t onesweep_depth3_hist_scan(void* temp, size_t temp_bytes, const uint32_t* keys, int P, int nb, uint32_t* base,
                                     const uint32_t* sort_err, uint32_t* host_out, uint32_t host_seq, uint32_t* host_max, hipStream_t s)
{
    if (!os3_args_ok(temp_bytes, P)) return hipErrorInvalidValue;
    const Os3Layout L = os3_layout(temp, (size_t)P);
    os_hist3_scan_kernel<<<1u + os_hist_blocks<uint32_t>((size_t)P), OS_HIST_BLOCK, 0, s>>>(keys, (size_t)P, L.hist[0], L.maxw, L.done, host_max, nb,
                                                                                            base, sort_err, host_out, host_seq);
    return hipGetLastError();
}
const uint32_t* onesweep_depth3_max_word(void* temp, int P) { return os3_layout(temp, (size_t)(P > 0 ? P : 1)).maxw; }

// passes 1 and 2 (of the low 18 bits): they do not depend on how many passes follow
hipError_t onesweep_depth3_head(void* temp, size_t temp_bytes, const uint32_t* kin, int P, const uint2* rects, hipStream_t s)
{
    if (!os3_args_ok(temp_bytes, P) || !rects) return hipErrorInvalidValue;
    const Os3Layout L = os3_layout(temp, (size_t)P);
    const unsigned blocks = (unsigned)L.blocks;
    os_pass_kernel<uint32_t, OS_BITS3, false, true, OS_RADIX3, true><<<blocks, C3DGS_OS_BLOCK32, 0, s>>>(
        kin, L.tk[0], nullptr, L.tv[0], (uint32_t)P, 0, L.hist[0], L.status[0], L.ticket + 0, rects, nullptr, nullptr, L.t2[0]);
    os_pass_kernel<uint32_t, OS_BITS3, false, true, OS_RADIX3, true><<<blocks, C3DGS_OS_BLOCK32, 0, s>>>(
        L.tk[0], L.tk[1], L.tv[0], L.tv[1], (uint32_t)P, OS_BITS3, L.hist[1], L.status[1], L.ticket + 1, rects, nullptr, L.t2[0], L.t2[1]);
    return hipGetLastError();
}
// pass 3, the last one where every visible key is below DEPTH_KEY_LIMIT3; otherwise pass 3 into the free buffer, the histogram of
// the 5 bits above and pass 4 on them. Either way the results land in kout / vout / rects_sorted as the four 8-bit passes leave them.
hipError_t onesweep_depth3_tail(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, uint32_t* vout, int P,
                                const uint2* rects, uint2* rects_sorted, uint32_t max_visible_key, hipStream_t s)
{
    if (!os3_args_ok(temp_bytes, P) || !rects || !rects_sorted) return hipErrorInvalidValue;
    const Os3Layout L = os3_layout(temp, (size_t)P);
    const unsigned blocks = (unsigned)L.blocks;
    const bool four = depth_sort_plan(true, max_visible_key).passes == 4;
    os_pass_kernel<uint32_t, OS_BITS3, false, true, OS_RADIX3, true><<<blocks, C3DGS_OS_BLOCK32, 0, s>>>(
        L.tk[1], four ? L.tk[0] : kout, L.tv[1], four ? L.tv[0] : vout, (uint32_t)P, 2 * OS_BITS3, L.hist[2], L.status[2], L.ticket + 2, rects,
        rects_sorted, L.t2[1], four ? L.t2[0] : nullptr);
    if (four) {
        os_hist3_top_kernel<<<os_hist_blocks<uint32_t>((size_t)P), OS_HIST_BLOCK, 0, s>>>(kin, (size_t)P, L.hist[3]);
        os_pass_kernel<uint32_t, OS_BITS3_TOP, false, true, OS_RADIX, true><<<blocks, C3DGS_OS_BLOCK32, 0, s>>>(
            L.tk[0], kout, L.tv[0], vout, (uint32_t)P, 3 * OS_BITS3, L.hist[3], L.status[3], L.ticket + 3, rects, rects_sorted, L.t2[0], nullptr);
    }
    return hipGetLastError();
}

#ifdef C3DGS_DIAG
int os_read_times(unsigned long long* out512)
{
    return hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_os_times), sizeof(unsigned long long) * 512) != hipSuccess;
}
#endif

// address of the current device's sticky error word (cached per device; one process per GPU is the normal case)
uint32_t* onesweep_error_word()
{
    static uint32_t* cache[64] = { nullptr };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!cache[dev]) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_os_error)) != hipSuccess) return nullptr;
        cache[dev] = (uint32_t*)p;
    }
    return cache[dev];
}

// debug helper: did any look-back so far time out on this device? (synchronises the stream; clears the word)
int onesweep_timed_out(hipStream_t s)
{
    if (!onesweep_enabled()) return 0;
    uint32_t* e = onesweep_error_word();
    uint32_t w = 1;
    if (!e || hipMemcpyAsync(&w, e, sizeof(w), hipMemcpyDeviceToHost, s) != hipSuccess) return 1;
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (w) (void)hipMemsetAsync(e, 0, sizeof(w), s);
    return w != 0;
}

bool onesweep_enabled()
{
    static const bool on = []() { const char* e = std::getenv("C3DGS_SORT_ROCPRIM"); return !(e && e[0] == '1'); }();
    return on;
}
// room for the second payload, in the four-pass and in the biased layout
size_t onesweep_depth_temp_bytes(int P)
{
    const size_t n = (size_t)(P > 0 ? P : 1);
    return std::max(os_temp_bytes<uint32_t>(n, 32, true), os3_layout(nullptr, n).total_bytes);
}
size_t onesweep_tile_temp_bytes(int R, int end_bit, int key_bytes)
{
    return key_bytes == 4 ? os_temp_bytes<uint32_t>((size_t)(R > 0 ? R : 1), end_bit) : os_temp_bytes<uint16_t>((size_t)(R > 0 ? R : 1), end_bit);
}
size_t onesweep_depth_clear_bytes(int P)      // covers the control words of both layouts (both start at the front of the scratch)
{
    const size_t n = (size_t)(P > 0 ? P : 1);
    return std::max(os_clear_bytes<uint32_t>(n, 32), os3_layout(nullptr, n).ctrl_bytes);
}
size_t onesweep_tile_clear_bytes(int R, int end_bit, int key_bytes)
{
    return key_bytes == 4 ? os_clear_bytes<uint32_t>((size_t)(R > 0 ? R : 1), end_bit) : os_clear_bytes<uint16_t>((size_t)(R > 0 ? R : 1), end_bit);
}
hipError_t onesweep_tile_sort32(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout,
                                int R, int end_bit, hipStream_t s, bool ctrl_cleared)
{
    return os_sort<uint32_t>(temp, temp_bytes, kin, kout, vin, vout, (size_t)R, end_bit, s, nullptr, nullptr, ctrl_cleared);
}
// the depth sort's histogram launch with the id-order scan of `nb` workgroup totals in its workgroup 0 (os_hist_scan_kernel).
// `temp`: the depth sort's scratch, its first onesweep_depth_clear_bytes(P) bytes cleared by an earlier kernel on the stream; the
// sort that follows is told `hist_done`.
hipError_t onesweep_depth_hist_scan(void* temp, size_t temp_bytes, const uint32_t* keys, int P, int nb, uint32_t* base,
                                    const uint32_t* sort_err, uint32_t* host_out, uint32_t host_seq, hipStream_t s)
{
    const size_t n = (size_t)P;
    if (P <= 0 || n >= ((size_t)1 << 30) || os_temp_bytes<uint32_t>(n, 32) > temp_bytes) return hipErrorInvalidValue;
    os_hist_scan_kernel<<<1u + os_hist_blocks<uint32_t>(n), OS_HIST_BLOCK, 0, s>>>(keys, n, os_plan(32), (uint32_t*)temp, nb, base,
                                                                                  sort_err, host_out, host_seq);
    return hipGetLastError();
}
hipError_t onesweep_depth_sort(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout,
                               int P, const uint2* gather_src, uint2* gather_dst, hipStream_t s, bool ctrl_cleared, bool rects_fit_bytes,
                               bool hist_done)
{
    // rects_fit_bytes: every coordinate of the tile rectangles is below 256 (grid of at most 255 x 255 tiles), so they can
    // travel with the items as a packed 32-bit second payload instead of being gathered behind the last pass
    static const bool no_pay2 = []() { const char* e = std::getenv("C3DGS_DEPTH_SORT_GATHER"); return e && e[0] == '1'; }();
    return os_sort<uint32_t>(temp, temp_bytes, kin, kout, vin, vout, (size_t)P, 32, s, gather_src, gather_dst, ctrl_cleared,
                             rects_fit_bytes && !no_pay2, hist_done && ctrl_cleared);
}
hipError_t onesweep_tile_sort(void* temp, size_t temp_bytes, const uint16_t* kin, uint16_t* kout, const uint32_t* vin, uint32_t* vout,
                              int R, int end_bit, hipStream_t s, bool ctrl_cleared)
{
    return os_sort<uint16_t>(temp, temp_bytes, kin, kout, vin, vout, (size_t)R, end_bit, s, nullptr, nullptr, ctrl_cleared);
}

} // namespace c3dgs
