// mcmc.hpp -- workspace layout and launchers of mcmc.hip (MCMC density control), shared with c_abi.hip.
#pragma once
#include "common.hpp"

namespace c3dgs {

constexpr int MCMC_BLOCK_ROWS = 256;      // rows per weights workgroup = the unit of the first search level
constexpr int MCMC_SCAN_THREADS = 1024;   // the one workgroup of the 64-bit block-base scan
constexpr int MCMC_SCAN_PER_THREAD = 4;   // block totals per thread and sweep: 4096 blocks (2^20 rows) per sweep
constexpr int MCMC_MAX_N = 51;            // relocation: N = min(count + 1, 51), the size of the binomial table

// Caller-owned workspace: local u32[P], the inclusive prefix of q inside each block of MCMC_BLOCK_ROWS rows (< 2^28) | total
// u32[nb], q summed per block | base u64[nb + 1], the exclusive prefix of `total`, base[nb] = T | new_opacity f32[P] and
// new_scale f32[3 P], the relocation values of the rows with count > 0, staged by the apply so that no launch reads a row it
// writes. Every region 256-byte aligned.
struct McmcLayout { size_t local, total, base, new_opacity, new_scale, total_bytes; };
inline McmcLayout mcmc_layout(int64_t P)
{
    const size_t p = (size_t)(P > 0 ? P : 1), nb = (p + MCMC_BLOCK_ROWS - 1) / MCMC_BLOCK_ROWS;
    McmcLayout L;
    size_t o = 0;
    L.local = o;       o = align_up(o + p * 4);
    L.total = o;       o = align_up(o + (nb + MCMC_SCAN_PER_THREAD) * 4);
    L.base = o;        o = align_up(o + (nb + 1) * 8);
    L.new_opacity = o; o = align_up(o + p * 4);
    L.new_scale = o;   o = align_up(o + p * 12);
    L.total_bytes = o;
    return L;
}

// weights + block scan (skipped with reuse_weights: the workspace still holds them), then n draws -> sources, counts. 0 < P < 2^31.
void launch_mcmc_weights(int64_t P, const float* raw_opacity, const uint8_t* dead, int derive, float min_opacity, uint8_t* dead_out,
                         uint32_t* q, int32_t* counts, unsigned long long* T, void* workspace, hipStream_t s);
void launch_mcmc_search(int64_t P, int64_t n, const double* draws, int32_t* sources, int32_t* counts, const void* workspace,
                        hipStream_t s);
// relocation values of the rows with count > 0 into the workspace, then the in-place row step
void launch_mcmc_values(int64_t P, const int32_t* counts, const float* raw_opacity, const float* raw_scale, int scale_floats,
                        float min_opacity, void* workspace, hipStream_t s);
void launch_mcmc_apply(int64_t P, int64_t n, const int32_t* dst, int64_t dst_base, const int32_t* sources, int n_tensors,
                       const c3dgs_rows_tensor* tensors, int copy_rows, const void* workspace, hipStream_t s);
void launch_mcmc_noise(int64_t P, float* xyz, const float* rotation, const float* scaling, const float* scaling_factor,
                       const float* raw_opacity, const float* xi, float noise_lr, float xyz_lr, hipStream_t s);

} // namespace c3dgs
