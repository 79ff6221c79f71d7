// sparse_adam.hip -- the Adam step over the Gaussians one view saw (gfx950, wave64). The rasterizer writes zero gradient rows
// for every Gaussian a view did not blend; the dense step (adam.hip) still moves 28 bytes per element of those rows, to decay
// their moments and drag the parameter along old momentum. Here a per-Gaussian mask (radii > 0, upstream 3DGS's
// optimizer_type="sparse_adam" rule) becomes a list of row ids on the device, and ONE launch per C3DGS_ADAM_MAX_TENSORS
// tensors updates the listed rows with adam.hip's arithmetic (adam_common.hpp). Unlisted rows are neither loaded nor stored.
//
//   select: count   listed rows per SPARSE_ADAM_SELECT_ROWS rows                     -> block_base[b]
//           scan    exclusive, one workgroup (scan_blocks.hpp)                       -> block_base[b], block_base[nb] = total
//           emit    rows[block_base[b] + rank inside the block] = id; count = total  (ascending, stable, no atomics)
//   step:   lanes run over the flattened (list entry, element) space: lane i of a tensor handles element i % row_len of row
//           rows[i / row_len]. A wave's accesses are contiguous inside a row, and consecutive listed rows continue each other.
//           The launch is sized from P; the kernel reads `count` from the workspace, so the host never learns it.
// Rows are disjoint and nothing is accumulated across lanes: results are bitwise reproducible.
#include "common.hpp"
#include "adam_common.hpp"
#include "jobs.hpp"
#include "scan_blocks.hpp"

namespace c3dgs {

constexpr int SA_SEL = SPARSE_ADAM_SELECT_ROWS;     // rows per select workgroup = its threads
constexpr int SA_STEP_UNROLL = 4;                   // elements per thread and trip of the step kernel: 28 memory operations in flight
constexpr int SA_STEP_CHUNK = 256 * SA_STEP_UNROLL;
constexpr int SA_STEP_MAX_BLOCKS = 4096;            // per tensor: two rounds of the 2048 workgroups of 256 the 256 CUs hold

template <int KIND>
__device__ __forceinline__ bool sa_listed(const void* __restrict__ mask, long long row)
{
    if (KIND == 0) return reinterpret_cast<const uint8_t*>(mask)[row] != 0;
    return reinterpret_cast<const int32_t*>(mask)[row] > 0;
}

template <int KIND>
__global__ void __launch_bounds__(SA_SEL) sa_count_kernel(long long P, const void* __restrict__ mask, uint32_t* __restrict__ block_base)
{
    __shared__ uint32_t s_w[SA_SEL / 64];
    const long long row = (long long)blockIdx.x * SA_SEL + threadIdx.x;
    const bool f = row < P && sa_listed<KIND>(mask, row);
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < SA_SEL / 64; w++) n += s_w[w];
        block_base[blockIdx.x] = n;
    }
}

__global__ void __launch_bounds__(SCAN_BLOCKS_THREADS) sa_scan_kernel(int nb, uint32_t* __restrict__ block_base)
{
    scan_blocks_body(nb, block_base, nullptr, nullptr, 0u);
}

template <int KIND>
__global__ void __launch_bounds__(SA_SEL) sa_emit_kernel(long long P, const void* __restrict__ mask, const uint32_t* __restrict__ block_base,
                                                         int nb, uint32_t* __restrict__ rows, uint32_t* __restrict__ count)
{
    __shared__ uint32_t s_w[SA_SEL / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * SA_SEL + threadIdx.x;
    const bool f = row < P && sa_listed<KIND>(mask, row);
    const unsigned long long b = __ballot(f);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (f) {
        uint32_t at = block_base[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));   // < the total <= P
#pragma unroll
        for (int w = 0; w < SA_SEL / 64; w++) if (w < wave) at += s_w[w];
        rows[at] = (uint32_t)row;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = block_base[nb];
}

void launch_sparse_adam_select(int64_t P, const void* mask, int mask_kind, void* workspace, hipStream_t s)
{
    const SparseAdamLayout L = sparse_adam_layout(P);
    char* w = (char*)workspace;
    uint32_t* count = (uint32_t*)(w + L.count);
    uint32_t* rows = (uint32_t*)(w + L.rows);
    uint32_t* base = (uint32_t*)(w + L.block_base);
    const int nb = (int)((P + SA_SEL - 1) / SA_SEL);
    if (mask_kind == 0) sa_count_kernel<0><<<nb, SA_SEL, 0, s>>>(P, mask, base);
    else sa_count_kernel<1><<<nb, SA_SEL, 0, s>>>(P, mask, base);
    sa_scan_kernel<<<1, SCAN_BLOCKS_THREADS, 0, s>>>(nb, base);
    if (mask_kind == 0) sa_emit_kernel<0><<<nb, SA_SEL, 0, s>>>(P, mask, base, nb, rows, count);
    else sa_emit_kernel<1><<<nb, SA_SEL, 0, s>>>(P, mask, base, nb, rows, count);
}

using SparseAdamJobs = JobTable<c3dgs_sparse_adam_tensor, C3DGS_ADAM_MAX_TENSORS>;

// RL: the row length as a constant (the divisions below become multiplies), 0: t.row_len at run time
template <int RL>
__device__ __forceinline__ void sa_step_rows(const c3dgs_sparse_adam_tensor& t, const uint32_t* __restrict__ rows, uint32_t count,
                                             uint32_t block, uint32_t nblocks, float w1, float beta2, float w2, float eps)
{
    const uint32_t L = RL ? (uint32_t)RL : (uint32_t)t.row_len;
    const unsigned long long total = (unsigned long long)count * L, stride = (unsigned long long)nblocks * SA_STEP_CHUNK;
    unsigned long long base = (unsigned long long)block * SA_STEP_CHUNK;
    if (base >= total) return;
    // (e0, r0) = (base / L, base % L), carried from trip to trip: the only 64-bit divisions are these two
    unsigned long long e0 = base / L;
    uint32_t r0 = (uint32_t)(base - e0 * L);
    const unsigned long long adv_e = stride / L;
    const uint32_t adv_r = (uint32_t)(stride - adv_e * L);
    const float neg_step = -t.step_size, bc2 = t.bias_correction2_sqrt;
    for (; base < total; base += stride) {
        size_t off[SA_STEP_UNROLL];
        bool live[SA_STEP_UNROLL];
        float p[SA_STEP_UNROLL], g[SA_STEP_UNROLL], m[SA_STEP_UNROLL], v[SA_STEP_UNROLL];
#pragma unroll
        for (int u = 0; u < SA_STEP_UNROLL; u++) {
            const uint32_t k = (uint32_t)(u * 256) + threadIdx.x;
            live[u] = base + k < total;
            const uint32_t local = r0 + k, q = local / L;                  // < L + SA_STEP_CHUNK
            off[u] = live[u] ? (size_t)rows[e0 + q] * L + (local - q * L) : 0;   // e0 + q < count: an entry of the list
        }
#pragma unroll
        for (int u = 0; u < SA_STEP_UNROLL; u++)
            if (live[u]) { p[u] = t.param[off[u]]; g[u] = t.grad[off[u]]; m[u] = t.exp_avg[off[u]]; v[u] = t.exp_avg_sq[off[u]]; }
#pragma unroll
        for (int u = 0; u < SA_STEP_UNROLL; u++)
            if (live[u]) {
                adam_one(p[u], g[u], m[u], v[u], w1, beta2, w2, eps, neg_step, bc2);
                t.param[off[u]] = p[u]; t.exp_avg[off[u]] = m[u]; t.exp_avg_sq[off[u]] = v[u];
            }
        e0 += adv_e; r0 += adv_r;
        if (r0 >= L) { r0 -= L; e0++; }
    }
}

__global__ void __launch_bounds__(256)
sparse_adam_kernel(const SparseAdamJobs jobs, const uint32_t* __restrict__ count_ptr, const uint32_t* __restrict__ rows, float w1,
                   float beta2, float w2, float eps)
{
    const uint32_t count = *count_ptr;
    if (count == 0) return;
    const int j = job_of_block(jobs);
    const c3dgs_sparse_adam_tensor t = jobs.t[j];
    const uint32_t block = blockIdx.x - (uint32_t)jobs.first_block[j], nblocks = (uint32_t)jobs.nblocks[j];
    switch (t.row_len) {                                 // the row lengths of a Gaussian model at SH degree 3, and 48 of its SH block
    case 1: sa_step_rows<1>(t, rows, count, block, nblocks, w1, beta2, w2, eps); break;
    case 3: sa_step_rows<3>(t, rows, count, block, nblocks, w1, beta2, w2, eps); break;
    case 4: sa_step_rows<4>(t, rows, count, block, nblocks, w1, beta2, w2, eps); break;
    case 45: sa_step_rows<45>(t, rows, count, block, nblocks, w1, beta2, w2, eps); break;
    case 48: sa_step_rows<48>(t, rows, count, block, nblocks, w1, beta2, w2, eps); break;
    default: sa_step_rows<0>(t, rows, count, block, nblocks, w1, beta2, w2, eps); break;
    }
}

void launch_sparse_adam_step(int n_tensors, const c3dgs_sparse_adam_tensor* tensors, int64_t P, const void* workspace, double beta1,
                             double beta2, double eps, hipStream_t s)
{
    const SparseAdamLayout L = sparse_adam_layout(P);
    const char* w = (const char*)workspace;
    SparseAdamJobs J;
    for (int k = 0; k < n_tensors; k++)                    // every row listed: one trip per workgroup
        if (tensors[k].n > 0) J.add(tensors[k], (tensors[k].n + SA_STEP_CHUNK - 1) / SA_STEP_CHUNK, SA_STEP_MAX_BLOCKS);
    if (J.n == 0) return;
    // 1 - beta is formed in double and rounded once, as launch_adam does
    sparse_adam_kernel<<<J.grid(), 256, 0, s>>>(J, (const uint32_t*)(w + L.count), (const uint32_t*)(w + L.rows), (float)(1.0 - beta1),
                                          (float)beta2, (float)(1.0 - beta2), (float)eps);
}

} // namespace c3dgs
