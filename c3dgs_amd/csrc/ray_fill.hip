// ray_fill.hip -- the plan and the positions of GaussianModel.densify_initial (scene/gaussian_model.py:1352-1389): new points
// one `step` apart on the ray from every point to each of its three nearest neighbours (DESIGN.md "Initial densification").
//
// The reference loops over 3 x int(max relative distance) levels and rebuilds the whole scene at each. Its result is a closed
// form of the neighbour table. With rel = fl(fl(sqrt(d2)) / step) of point i and neighbour slot nb, and r2 the second-largest
// rel of that slot counted with multiplicity (levels that only the single farthest point reaches insert nothing: the
// reference's `slot.sum() > 1`), point i receives
//     c = max(0, floor(min(rel, r2)) - 1)     rows, at levels 1..c, at   x[i] * (1 - a) + a * x[j],   a = float(level) / rel
// and the new rows are ordered by slot, then level, then source index. Here:
//     top2     per-workgroup top-2 of rel per slot (lane shuffles, then LDS across the four waves), one small merge workgroup;
//              no float atomics
//     count    one lane per (slot, point): c, saturated at INT32_MAX
//     scan     ONE rocPRIM exclusive scan of the 3P counts in 64 bits; totals and the overflow flag for the host read
//     emit     output driven, one lane per new row in (slot, point, level) order: a binary search in the scanned offsets
//              names its point, so one far outlier costs what its rows cost and no lane loops over a million levels
//     order    per slot a STABLE rocPRIM radix sort of (level, src) on as many key bits as the slot's largest level has:
//              rows of one level keep the ascending source order they were emitted in
//     write    src / slot / level of the rows below `capacity`
//     xyz      one lane per new row: the position, every operation rounded on its own
// Compiled with -ffp-contract=off: the position is one subtraction, two multiplications and one addition in fp32, as torch
// evaluates the reference's expression. HBM-bound streaming passes; the only LDS is the 4-wave merge of the top-2.
#include "common.hpp"
#include <climits>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace c3dgs {

constexpr int RF_TOP2_BLOCKS = 1024;       // workgroups of the top-2 pass; the grid stride covers the rest

struct RayFillHead {                       // the small results at the front of the workspace
    float r2[3];                           // second-largest rel per slot (-1: the slot has fewer than 2 points)
    int32_t info[7];                       // rows of slot 0, 1, 2, overflow, largest level of slot 0, 1, 2
    unsigned long long begin[4];           // first row of each slot in the emitted order, then the total
};

struct Widen {
    __host__ __device__ unsigned long long operator()(uint32_t c) const { return c; }
};
using CountIt = rocprim::transform_iterator<const uint32_t*, Widen, unsigned long long>;

static size_t rf_scan_bytes(size_t n)
{
    size_t bytes = 0;
    CountIt it((const uint32_t*)nullptr, Widen{});
    (void)rocprim::exclusive_scan(nullptr, bytes, it, (unsigned long long*)nullptr, 0ull, n > 0 ? n : 1,
                                  rocprim::plus<unsigned long long>());
    return bytes < 256 ? 256 : bytes;
}

static size_t rf_sort_bytes(size_t rows)
{
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr,
                                    (int32_t*)nullptr, rows > 0 ? rows : 1, 0u, 32u);
    return bytes < 256 ? 256 : bytes;
}

struct RayFillLayout {
    size_t head, partial, cnt, off, scan, scan_bytes, key_in, val_in, key_out, val_out, sort, sort_bytes, total;
};

static RayFillLayout ray_fill_layout(int P, long long rows)
{
    const size_t p3 = 3 * (size_t)(P > 0 ? P : 1), r = (size_t)(rows > 0 ? rows : 0);
    RayFillLayout L{};
    size_t o = 0;
    L.head = o;     o = align_up(o + sizeof(RayFillHead));
    L.partial = o;  o = align_up(o + (size_t)RF_TOP2_BLOCKS * 6 * sizeof(float));
    L.cnt = o;      o = align_up(o + p3 * 4);
    L.off = o;      o = align_up(o + p3 * 8);
    L.scan = o;     L.scan_bytes = rf_scan_bytes(p3);
    o = align_up(o + L.scan_bytes);
    if (r > 0) {
        L.key_in = o;   o = align_up(o + r * 4);
        L.val_in = o;   o = align_up(o + r * 4);
        L.key_out = o;  o = align_up(o + r * 4);
        L.val_out = o;  o = align_up(o + r * 4);
        L.sort = o;     L.sort_bytes = rf_sort_bytes(r);
        o = align_up(o + L.sort_bytes);
    }
    L.total = o;
    return L;
}

size_t ray_fill_plan_workspace_bytes(int P, long long rows) { return ray_fill_layout(P, rows).total; }

// Both operations correctly rounded. sqrtf, not __fsqrt_rn: with this toolchain the intrinsic becomes a bare v_sqrt_f32 (1 ulp),
// while sqrtf gets the refined sequence (hipcc rounds fp32 divide and sqrt correctly by default).
__device__ __forceinline__ float rf_rel(float d2, float step) { return __fdiv_rn(sqrtf(d2), step); }

// top-2 with multiplicity of the union of two top-2 pairs
__device__ __forceinline__ void rf_merge(float& m1, float& m2, float o1, float o2)
{
    const float lo = fminf(m1, o1);
    m1 = fmaxf(m1, o1);
    m2 = fmaxf(lo, fmaxf(m2, o2));
}

// workgroup-wide top-2 of three slots; the result is valid in thread 0
__device__ __forceinline__ void rf_block_top2(float (&m1)[3], float (&m2)[3])
{
    __shared__ float sh[4][6];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rf_merge(m1[a], m2[a], __shfl_xor(m1[a], o), __shfl_xor(m2[a], o));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) { sh[wave][2 * a] = m1[a]; sh[wave][2 * a + 1] = m2[a]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++)
#pragma unroll
            for (int a = 0; a < 3; a++) rf_merge(m1[a], m2[a], sh[w][2 * a], sh[w][2 * a + 1]);
}

__global__ void __launch_bounds__(256)
ray_fill_top2_kernel(int P, const float* __restrict__ d2, float step, float* __restrict__ partial /*[gridDim.x, 6]*/)
{
    float m1[3] = { -1.f, -1.f, -1.f }, m2[3] = { -1.f, -1.f, -1.f };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256)
#pragma unroll
        for (int a = 0; a < 3; a++) rf_merge(m1[a], m2[a], rf_rel(d2[3 * (size_t)i + a], step), -1.f);
    rf_block_top2(m1, m2);
    if (threadIdx.x == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) { partial[6 * blockIdx.x + 2 * a] = m1[a]; partial[6 * blockIdx.x + 2 * a + 1] = m2[a]; }
}

__global__ void __launch_bounds__(256)
ray_fill_top2_merge_kernel(int nblocks, const float* __restrict__ partial, RayFillHead* __restrict__ head)
{
    float m1[3] = { -1.f, -1.f, -1.f }, m2[3] = { -1.f, -1.f, -1.f };
    for (int b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int a = 0; a < 3; a++) rf_merge(m1[a], m2[a], partial[6 * b + 2 * a], partial[6 * b + 2 * a + 1]);
    rf_block_top2(m1, m2);
    if (threadIdx.x == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) head->r2[a] = m2[a];
}

// rows of a point whose capped relative distance is m: max(0, floor(m) - 1), saturated
__device__ __forceinline__ uint32_t rf_count(float m)
{
    if (!(m >= 2.f)) return 0u;
    if (m >= 2147483648.f) return (uint32_t)INT32_MAX;
    return (uint32_t)floorf(m) - 1u;
}

__global__ void __launch_bounds__(256)
ray_fill_count_kernel(int P, const float* __restrict__ d2, float step, const RayFillHead* __restrict__ head,
                      uint32_t* __restrict__ cnt /*[3, P]*/)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= 3ll * P) return;
    const int nb = (int)(k / P);
    const size_t i = (size_t)(k - (long long)nb * P);
    cnt[k] = rf_count(fminf(rf_rel(d2[3 * i + nb], step), head->r2[nb]));
}

__global__ void ray_fill_totals_kernel(int P, const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ off,
                                       RayFillHead* __restrict__ head, int32_t* __restrict__ totals)
{
    const size_t p = (size_t)P;
    unsigned long long b[4] = { 0ull, off[p], off[2 * p], off[3 * p - 1] + cnt[3 * p - 1] };
    const bool overflow = (unsigned long long)P + b[3] > (unsigned long long)(INT32_MAX - 255);
    for (int a = 0; a < 3; a++) {
        const unsigned long long n = b[a + 1] - b[a];
        head->info[a] = totals[a] = (int32_t)(n > (unsigned long long)INT32_MAX ? (unsigned long long)INT32_MAX : n);
        head->info[4 + a] = n > 0 ? (int32_t)rf_count(head->r2[a]) : 0;     // the largest count of a slot is floor(r2) - 1
        head->begin[a] = b[a];
    }
    head->begin[3] = b[3];
    head->info[3] = totals[3] = overflow ? 1 : 0;
}

__global__ void __launch_bounds__(256)
ray_fill_emit_kernel(int P, long long total, const unsigned long long* __restrict__ off, uint32_t* __restrict__ key,
                     int32_t* __restrict__ val)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    long long lo = 0, hi = 3ll * P;                   // the last k with off[k] <= g; off[0] = 0, so there is one
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (off[mid] <= (unsigned long long)g) lo = mid; else hi = mid;
    }
    key[g] = (uint32_t)((unsigned long long)g - off[lo]) + 1u;
    val[g] = (int32_t)(lo % P);
}

__global__ void __launch_bounds__(256)
ray_fill_write_kernel(long long n, const RayFillHead* __restrict__ head, const uint32_t* __restrict__ key,
                      const int32_t* __restrict__ val, int32_t* __restrict__ src, uint8_t* __restrict__ slot,
                      int32_t* __restrict__ level)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    src[g] = val[g];
    level[g] = (int32_t)key[g];
    slot[g] = (uint8_t)(((unsigned long long)g >= head->begin[1]) + ((unsigned long long)g >= head->begin[2]));
}

static int rf_grid(long long n) { return (int)((n + 255) / 256); }

hipError_t run_ray_fill_plan(int P, const float* d2, float step, long long capacity, int32_t* src, uint8_t* slot, int32_t* level,
                             int32_t* totals, void* workspace, size_t workspace_bytes, hipStream_t s, std::string* problem)
{
    const RayFillLayout L0 = ray_fill_layout(P, 0);
    if (workspace_bytes < L0.total) { *problem = "workspace smaller than c3dgs_ray_fill_plan_workspace_bytes(P, 0)"; return hipSuccess; }
    char* w = (char*)workspace;
    RayFillHead* head = (RayFillHead*)(w + L0.head);
    float* partial = (float*)(w + L0.partial);
    uint32_t* cnt = (uint32_t*)(w + L0.cnt);
    unsigned long long* off = (unsigned long long*)(w + L0.off);
    const int pgrid = rf_grid(P), tgrid = pgrid < RF_TOP2_BLOCKS ? pgrid : RF_TOP2_BLOCKS;
    ray_fill_top2_kernel<<<tgrid, 256, 0, s>>>(P, d2, step, partial);
    ray_fill_top2_merge_kernel<<<1, 256, 0, s>>>(tgrid, partial, head);
    ray_fill_count_kernel<<<rf_grid(3ll * P), 256, 0, s>>>(P, d2, step, head, cnt);
    size_t bytes = L0.scan_bytes;
    hipError_t e = rocprim::exclusive_scan((void*)(w + L0.scan), bytes, CountIt(cnt, Widen{}), off, 0ull, 3 * (size_t)P,
                                           rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return e;
    ray_fill_totals_kernel<<<1, 1, 0, s>>>(P, cnt, off, head, totals);
    if (!src) return hipGetLastError();

    // the emitting call sizes its launches and the sorts' key bits from the totals: one small read
    int32_t info[7];
    if ((e = hipMemcpyAsync(info, head->info, sizeof(info), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (info[3]) return hipSuccess;                                  // overflow: nothing is written
    const long long n[3] = { info[0], info[1], info[2] }, total = n[0] + n[1] + n[2];
    if (total == 0) return hipSuccess;
    const RayFillLayout L = ray_fill_layout(P, total);
    if (workspace_bytes < L.total) {
        *problem = "workspace too small for " + std::to_string(total) + " new rows (c3dgs_ray_fill_plan_workspace_bytes(P, rows))";
        return hipSuccess;
    }
    uint32_t *key_in = (uint32_t*)(w + L.key_in), *key_out = (uint32_t*)(w + L.key_out);
    int32_t *val_in = (int32_t*)(w + L.val_in), *val_out = (int32_t*)(w + L.val_out);
    ray_fill_emit_kernel<<<rf_grid(total), 256, 0, s>>>(P, total, off, key_in, val_in);
    long long b = 0;
    for (int a = 0; a < 3; a++) {
        if (n[a] > 0) {
            unsigned bits = 1;
            while (bits < 32 && ((uint32_t)info[4 + a] >> bits)) bits++;
            size_t sb = L.sort_bytes;
            e = rocprim::radix_sort_pairs((void*)(w + L.sort), sb, key_in + b, key_out + b, val_in + b, val_out + b, (size_t)n[a],
                                          0u, bits, s);
            if (e != hipSuccess) return e;
        }
        b += n[a];
    }
    const long long nw = total < capacity ? total : capacity;
    if (nw > 0) ray_fill_write_kernel<<<rf_grid(nw), 256, 0, s>>>(nw, head, key_out, val_out, src, slot, level);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ positions
__global__ void __launch_bounds__(256)
ray_fill_xyz_kernel(int P, const float* __restrict__ xyz, const int32_t* __restrict__ idx, const float* __restrict__ d2, float step,
                    long long n_new, const int32_t* __restrict__ src, const uint8_t* __restrict__ slot,
                    const int32_t* __restrict__ level, float* __restrict__ out)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_new) return;
    const int i = src[r], nb = slot[r];
    float v[3] = { 0.f, 0.f, 0.f };
    if (i >= 0 && i < P && nb < 3) {                                 // a bad plan writes zeros, never reads out of bounds
        const int j = idx[3 * (size_t)i + nb];
        if (j >= 0 && j < P) {
            const float a = __fdiv_rn((float)level[r], rf_rel(d2[3 * (size_t)i + nb], step));
            const float na = 1.0f - a;
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = xyz[3 * (size_t)i + c] * na + a * xyz[3 * (size_t)j + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * (size_t)r + c] = v[c];
}

void launch_ray_fill_xyz(int P, const float* xyz, const int32_t* idx, const float* d2, float step, long long n_new,
                         const int32_t* src, const uint8_t* slot, const int32_t* level, float* out, hipStream_t s)
{
    ray_fill_xyz_kernel<<<rf_grid(n_new), 256, 0, s>>>(P, xyz, idx, d2, step, n_new, src, slot, level, out);
}

} // namespace c3dgs
