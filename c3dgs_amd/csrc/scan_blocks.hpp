// scan_blocks.hpp -- the single-workgroup exclusive scan of the per-workgroup instance totals (gfx950). A device function, not a
// kernel: preprocess.hip launches it alone (scan_blocks_kernel), radix_sort.hip runs it in workgroup 0 of the launch that also
// builds the depth sort's digit histograms (os_hist_scan_kernel), so that the two small jobs behind preprocess share one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace c3dgs {

constexpr int SCAN_BLOCKS_THREADS = 1024;

// exclusive scan of the workgroup totals, in place: base[b] = instances of all Gaussians before workgroup b;
// base[nb] = num_rendered. One workgroup of SCAN_BLOCKS_THREADS threads (all of them must call); nb = P/256 is a few thousand to a few ten-thousand.
// `sort_err` (optional): the device's sticky sort time-out word, copied behind the total so that the forward's single
// device->host read of num_rendered brings it along (radix_sort.hip).
// `host_out` (optional): three words of MAPPED, coherent host memory {total, sort error word, host_seq}: the forward's one
// device->host read without a copy command -- the host polls the third word for `host_seq` (c_abi.hip). A copy command behind
// this kernel cost a 4 us launch of its own plus a ~6 us bubble on the stream.
__device__ __forceinline__ void scan_blocks_body(int nb, uint32_t* __restrict__ base, const uint32_t* __restrict__ sort_err,
                                                 uint32_t* __restrict__ host_out, uint32_t host_seq)
{
    // One workgroup; a thread owns 16 CONSECUTIVE totals (four independent 16-byte loads), so 16384 totals cost one
    // memory round trip and one barrier. (One total per thread and a round trip + barrier per 1024 totals took 12 us for the
    // 11.7k totals of P = 3M: pure latency.) `base` is 256-byte aligned with room up to the next multiple of 16 entries + 2.
    __shared__ uint32_t s_w[2][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t carry = 0;                                   // every thread tracks the running total itself
    int buf = 0;
    for (int c0 = 0; c0 < nb; c0 += 16384, buf ^= 1) {
        const int i0 = c0 + t * 16;
        uint32_t v[16];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (i0 + 4 * q + 3 < nb) x = reinterpret_cast<const uint4*>(base + i0)[q];
            else {
                if (i0 + 4 * q < nb) x.x = base[i0 + 4 * q];
                if (i0 + 4 * q + 1 < nb) x.y = base[i0 + 4 * q + 1];
                if (i0 + 4 * q + 2 < nb) x.z = base[i0 + 4 * q + 2];
            }
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
        uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) mine += v[q];
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        if (lane == 63) s_w[buf][wave] = incl;
        __syncthreads();                                  // s_w is double-buffered: one barrier per sweep
        uint32_t off = carry, all = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { const uint32_t x = s_w[buf][w]; if (w < wave) off += x; all += x; }
        uint32_t run = off + incl - mine;                 // exclusive base of this thread's first total
#pragma unroll
        for (int q = 0; q < 16; q++) { const uint32_t x = v[q]; v[q] = run; run += x; }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (i0 + 4 * q + 3 < nb) reinterpret_cast<uint4*>(base + i0)[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            else {
                if (i0 + 4 * q < nb) base[i0 + 4 * q] = v[4 * q];
                if (i0 + 4 * q + 1 < nb) base[i0 + 4 * q + 1] = v[4 * q + 1];
                if (i0 + 4 * q + 2 < nb) base[i0 + 4 * q + 2] = v[4 * q + 2];
            }
        }
        carry += all;
    }
    __syncthreads();                                      // the last sweep's stores precede the two words behind them
    if (t == 0) {
        base[nb] = carry;
        const uint32_t err = sort_err ? *sort_err : 0u;
        if (sort_err) base[nb + 1] = err;
        if (host_out) {
            __hip_atomic_store(host_out, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_out + 1, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_out + 2, host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // publishes the two words above
        }
    }
}

} // namespace c3dgs
