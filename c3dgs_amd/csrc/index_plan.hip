// index_plan.hip -- the plan of a prune / codebook compaction of an INDEXED model (scene/gaussian_model.py:1101-1158).
//
// The reference builds the index remap with a Python loop over every referenced codebook id, one device write each
// (:1110-1113). Here:
//     flags      one lane per Gaussian: a survivor sets the used flag of the codebook row each of its index arrays names (plain
//                byte stores of the constant 1: lanes that meet on a row all write the same value); an index outside [0, K) is
//                counted and never dereferenced
//     scans      rocPRIM exclusive scans of keep and of the two flag arrays (the scan run_rows_plan uses)
//     emit       one pass: surviving Gaussians in source order with their remapped indices (new index = rank of the old id
//                among the referenced ids), referenced codebook rows in ascending old id
// The rows themselves are moved by rows_apply (densify.hip) with these maps. Streaming passes: no LDS, one atomic per BAD index.
// Both calls of the two-call protocol run flags, scans and totals; only the second runs emit. Sizes are at most
// INT32_MAX - 255 (c_abi.hip), so the one-lane-per-row grids fit int arithmetic.
#include "common.hpp"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace c3dgs {

struct NonZero {
    __host__ __device__ int32_t operator()(uint8_t c) const { return c ? 1 : 0; }
};
using FlagIt = rocprim::transform_iterator<const uint8_t*, NonZero, int32_t>;

static size_t flag_scan_bytes(size_t n)
{
    size_t bytes = 0;
    FlagIt it((const uint8_t*)nullptr, NonZero{});
    (void)rocprim::exclusive_scan(nullptr, bytes, it, (int32_t*)nullptr, (int32_t)0, n > 0 ? n : 1, rocprim::plus<int32_t>());
    return bytes;
}

struct IndexPlanLayout {
    size_t scan_bytes, flag0, flag1, off_keep, off0, off1, total;
};

static IndexPlanLayout index_plan_layout(int P, int K0, int K1)
{
    const size_t p = P > 0 ? P : 1, k0 = K0 > 0 ? K0 : 1, k1 = K1 > 0 ? K1 : 1;
    IndexPlanLayout L;
    size_t b = flag_scan_bytes(p);
    const size_t b0 = flag_scan_bytes(k0), b1 = flag_scan_bytes(k1);
    b = b0 > b ? b0 : b;
    b = b1 > b ? b1 : b;
    L.scan_bytes = b;
    size_t o = align_up(b < 256 ? 256 : b);
    L.flag0 = o;    o = align_up(o + k0);        // flag0 and flag1 are adjacent: one clear covers both
    L.flag1 = o;    o = align_up(o + k1);
    L.off_keep = o; o = align_up(o + p * 4);
    L.off0 = o;     o = align_up(o + k0 * 4);
    L.off1 = o;     o = align_up(o + k1 * 4);
    L.total = o;
    return L;
}

size_t index_plan_workspace_bytes(int P, int K0, int K1) { return index_plan_layout(P, K0, K1).total; }

__global__ void __launch_bounds__(256)
index_flags_kernel(int P, const uint8_t* __restrict__ keep, const int64_t* __restrict__ idx0, int K0, const int64_t* __restrict__ idx1,
                   int K1, uint8_t* __restrict__ flag0, uint8_t* __restrict__ flag1, int32_t* __restrict__ totals)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const bool kept = !keep || keep[i];
    int bad = 0;
    if (idx0) {
        const int64_t v = idx0[i];
        if (v < 0 || v >= K0) bad++;
        else if (kept) flag0[v] = 1;
    }
    if (idx1) {
        const int64_t v = idx1[i];
        if (v < 0 || v >= K1) bad++;
        else if (kept) flag1[v] = 1;
    }
    if (bad) atomicAdd(&totals[3], bad);
}

__global__ void index_totals_kernel(int P, const uint8_t* __restrict__ keep, const int32_t* __restrict__ off_keep, int K0,
                                    const uint8_t* __restrict__ flag0, const int32_t* __restrict__ off0, int K1,
                                    const uint8_t* __restrict__ flag1, const int32_t* __restrict__ off1, int32_t* __restrict__ totals)
{
    totals[0] = keep ? off_keep[P - 1] + (keep[P - 1] ? 1 : 0) : P;
    totals[1] = flag0 ? off0[K0 - 1] + flag0[K0 - 1] : 0;
    totals[2] = flag1 ? off1[K1 - 1] + flag1[K1 - 1] : 0;
}

__global__ void __launch_bounds__(256)
index_emit_kernel(int P, const uint8_t* __restrict__ keep, const int32_t* __restrict__ off_keep, const int64_t* __restrict__ idx0,
                  int K0, const uint8_t* __restrict__ flag0, const int32_t* __restrict__ off0, const int64_t* __restrict__ idx1, int K1,
                  const uint8_t* __restrict__ flag1, const int32_t* __restrict__ off1, long long cap_rows, long long cap_cb0,
                  long long cap_cb1, int32_t* __restrict__ src, int64_t* __restrict__ new_idx0, int64_t* __restrict__ new_idx1,
                  int32_t* __restrict__ cb_src0, int32_t* __restrict__ cb_src1)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P && (!keep || keep[i])) {
        const long long j = keep ? off_keep[i] : i;
        if (j < cap_rows) {
            src[j] = i;
            if (idx0) {
                const int64_t v = idx0[i];
                new_idx0[j] = (v < 0 || v >= K0) ? -1 : off0[v];
            }
            if (idx1) {
                const int64_t v = idx1[i];
                new_idx1[j] = (v < 0 || v >= K1) ? -1 : off1[v];
            }
        }
    }
    if (flag0 && i < K0 && flag0[i]) {
        const long long r = off0[i];
        if (r < cap_cb0) cb_src0[r] = i;
    }
    if (flag1 && i < K1 && flag1[i]) {
        const long long r = off1[i];
        if (r < cap_cb1) cb_src1[r] = i;
    }
}

hipError_t run_index_plan(int P, const uint8_t* keep, const int64_t* idx0, int K0, const int64_t* idx1, int K1, long long cap_rows,
                          long long cap_cb0, long long cap_cb1, int32_t* src, int64_t* new_idx0, int64_t* new_idx1, int32_t* cb_src0,
                          int32_t* cb_src1, int32_t* totals, void* workspace, hipStream_t s)
{
    const IndexPlanLayout L = index_plan_layout(P, K0, K1);
    char* ws = static_cast<char*>(workspace);
    uint8_t* flag0 = idx0 ? reinterpret_cast<uint8_t*>(ws + L.flag0) : nullptr;
    uint8_t* flag1 = idx1 ? reinterpret_cast<uint8_t*>(ws + L.flag1) : nullptr;
    int32_t* off_keep = reinterpret_cast<int32_t*>(ws + L.off_keep);
    int32_t* off0 = reinterpret_cast<int32_t*>(ws + L.off0);
    int32_t* off1 = reinterpret_cast<int32_t*>(ws + L.off1);
    hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    if (idx0 || idx1) {
        e = hipMemsetAsync(ws + L.flag0, 0, L.off_keep - L.flag0, s);
        if (e != hipSuccess) return e;
        index_flags_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, keep, idx0, K0, idx1, K1, flag0, flag1, totals);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    size_t bytes = L.scan_bytes;
    if (keep) {
        e = rocprim::exclusive_scan(workspace, bytes, FlagIt(keep, NonZero{}), off_keep, (int32_t)0, (size_t)P, rocprim::plus<int32_t>(), s);
        if (e != hipSuccess) return e;
    }
    if (idx0) {
        bytes = L.scan_bytes;
        e = rocprim::exclusive_scan(workspace, bytes, FlagIt(flag0, NonZero{}), off0, (int32_t)0, (size_t)K0, rocprim::plus<int32_t>(), s);
        if (e != hipSuccess) return e;
    }
    if (idx1) {
        bytes = L.scan_bytes;
        e = rocprim::exclusive_scan(workspace, bytes, FlagIt(flag1, NonZero{}), off1, (int32_t)0, (size_t)K1, rocprim::plus<int32_t>(), s);
        if (e != hipSuccess) return e;
    }
    index_totals_kernel<<<1, 1, 0, s>>>(P, keep, off_keep, K0, flag0, off0, K1, flag1, off1, totals);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (src) {
        int n = P;
        if (idx0 && K0 > n) n = K0;
        if (idx1 && K1 > n) n = K1;
        index_emit_kernel<<<(n + 255) / 256, 256, 0, s>>>(P, keep, off_keep, idx0, K0, flag0, off0, idx1, K1, flag1, off1, cap_rows,
                                                         cap_cb0, cap_cb1, src, new_idx0, new_idx1, cb_src0, cb_src1);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace c3dgs
