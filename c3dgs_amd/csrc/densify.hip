// densify.hip -- adaptive density control (scene/gaussian_model.py:1187-1403, train.py:101-106) for non-indexed models.
//
// The reference changes the number of Gaussians in four full passes per densify_and_prune (clone cat, split cat, the split's
// own prune_points, the final prune_points), each over 7 parameter tensors and their 14 Adam moment tensors, each boolean
// mask a nonzero with a host synchronisation. Here:
//     classify   one thread per row: the reference's predicates on the activated values -> one code byte
//     plan       ONE rocPRIM exclusive scan of the four per-row counts (the scan qat.hip uses for the visible rows, on a
//                4-lane counter) + an emit pass: source row, kind and draw row of every row of the new scene, in the
//                reference's row order; four totals for the single host read
//     apply      ONE output-driven gather launch over a table of tensors: every float of every new parameter tensor and
//                both its moments is written exactly once (one dword per lane, every wave-instruction its own 256
//                contiguous bytes), reads are monotone gathers of whole rows; the
//                split children's xyz and scaling rows are computed in the same launch
//     stats      the per-iteration accumulators, one launch, no allocation
// HBM-bound streaming: no LDS, no atomics. Compiled with -ffp-contract=off (sqrt(gx*gx + gy*gy) and sqrt(g*g) are the
// two-rounding expressions torch evaluates).
#include "common.hpp"
#include "jobs.hpp"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <hip/hip_fp16.h>

namespace c3dgs {

// ------------------------------------------------------------------------------------------------ classify
__device__ __forceinline__ float max3(const float* __restrict__ p, size_t i)
{
    // torch.max(dim=1).values propagates NaN; fmaxf would drop it. A NaN scale compares false either way round, like torch's.
    const float a = p[3 * i], b = p[3 * i + 1], c = p[3 * i + 2];
    float m = (b > a || b != b) ? b : a;
    m = (c > m || c != c) ? c : m;
    return a != a ? a : m;
}

__global__ void __launch_bounds__(256)
densify_classify_kernel(int P, const float* __restrict__ accum, const float* __restrict__ denom, const float* __restrict__ scale_clone,
                        const float* __restrict__ scale_split, const float* __restrict__ scale_prune_self,
                        const float* __restrict__ scale_prune_child, const float* __restrict__ opacity, float max_grad,
                        float dense_extent, float min_opacity, float big_extent, uint8_t* __restrict__ code)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float g = accum[i] / denom[i];
    if (g != g) g = 0.f;
    const bool clone = sqrtf(g * g) >= max_grad && max3(scale_clone, i) <= dense_extent;       // torch.norm(grads, dim=-1)
    const bool split = g >= max_grad && max3(scale_split, i) > dense_extent;
    const bool low = opacity[i] < min_opacity;
    bool prune_self = low, prune_child = low;
    if (scale_prune_self) {
        prune_self = prune_self || max3(scale_prune_self, i) > big_extent;
        prune_child = prune_child || max3(scale_prune_child, i) > big_extent;
    }
    unsigned c = 0;
    if (!split && !prune_self) c |= C3DGS_ROW_KEEP;
    if (clone && !prune_self) c |= C3DGS_ROW_CLONE;
    if (split) c |= C3DGS_ROW_SPLIT;
    if (split && !prune_child) c |= C3DGS_ROW_CHILD_KEPT;
    code[i] = (uint8_t)c;
}

void launch_densify_classify(int P, const float* accum, const float* denom, const float* scale_clone, const float* scale_split,
                             const float* scale_prune_self, const float* scale_prune_child, const float* opacity, float max_grad,
                             float dense_extent, float min_opacity, float big_extent, uint8_t* code, hipStream_t s)
{
    densify_classify_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, accum, denom, scale_clone, scale_split, scale_prune_self,
                                                            scale_prune_child, opacity, max_grad, dense_extent, min_opacity,
                                                            big_extent, code);
}

// ------------------------------------------------------------------------------------------------ plan
struct Cnt4 { int32_t k, c, s, ck; };
struct CntPlus {
    __host__ __device__ Cnt4 operator()(const Cnt4& a, const Cnt4& b) const { return { a.k + b.k, a.c + b.c, a.s + b.s, a.ck + b.ck }; }
};
__host__ __device__ inline Cnt4 code_counts(uint8_t c)
{
    const int split = (c & C3DGS_ROW_SPLIT) ? 1 : 0;
    return { (int32_t)(c & C3DGS_ROW_KEEP), (int32_t)((c >> 1) & 1), split, (split && (c & C3DGS_ROW_CHILD_KEPT)) ? 1 : 0 };
}
struct CodeToCnt {
    __host__ __device__ Cnt4 operator()(uint8_t c) const { return code_counts(c); }
};
using CntIt = rocprim::transform_iterator<const uint8_t*, CodeToCnt, Cnt4>;

static size_t plan_scan_bytes(int P)
{
    size_t bytes = 0;
    CntIt it((const uint8_t*)nullptr, CodeToCnt{});
    (void)rocprim::exclusive_scan(nullptr, bytes, it, (Cnt4*)nullptr, Cnt4{ 0, 0, 0, 0 }, (size_t)(P > 0 ? P : 1), CntPlus{});
    return align_up(bytes < 256 ? 256 : bytes);
}

size_t rows_plan_workspace_bytes(int P)
{
    return plan_scan_bytes(P) + align_up(sizeof(Cnt4) * (size_t)(P > 0 ? P : 1));
}

__global__ void rows_totals_kernel(int P, const uint8_t* __restrict__ code, const Cnt4* __restrict__ off, int32_t* __restrict__ totals)
{
    const Cnt4 t = CntPlus{}(off[P - 1], code_counts(code[P - 1]));
    totals[0] = t.k; totals[1] = t.c; totals[2] = t.s; totals[3] = t.ck;
}

__global__ void __launch_bounds__(256)
rows_emit_kernel(int P, const uint8_t* __restrict__ code, const Cnt4* __restrict__ off, const int32_t* __restrict__ totals, int N,
                 long long capacity, int32_t* __restrict__ src, uint8_t* __restrict__ kind, int32_t* __restrict__ draw_row)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const Cnt4 c = code_counts(code[i]);
    const Cnt4 o = off[i];
    const long long K = totals[0], C = totals[1], S = totals[2], CK = totals[3];
    if (c.k) {
        const long long j = o.k;
        if (j < capacity) { src[j] = i; kind[j] = C3DGS_KIND_ORIGINAL; draw_row[j] = -1; }
    }
    if (c.c) {
        const long long j = K + o.c;
        if (j < capacity) { src[j] = i; kind[j] = C3DGS_KIND_CLONE; draw_row[j] = -1; }
    }
    if (c.ck)
        for (int k = 0; k < N; k++) {
            const long long j = K + C + k * CK + o.ck;
            if (j < capacity) { src[j] = i; kind[j] = (uint8_t)(C3DGS_KIND_CHILD + k); draw_row[j] = (int32_t)(k * S + o.s); }
        }
}

hipError_t run_rows_plan(int P, const uint8_t* code, int N, long long capacity, int32_t* src, uint8_t* kind, int32_t* draw_row,
                         int32_t* totals, void* workspace, hipStream_t s)
{
    size_t bytes = plan_scan_bytes(P);
    Cnt4* off = reinterpret_cast<Cnt4*>(static_cast<char*>(workspace) + bytes);
    CntIt it(code, CodeToCnt{});
    hipError_t e = rocprim::exclusive_scan(workspace, bytes, it, off, Cnt4{ 0, 0, 0, 0 }, (size_t)P, CntPlus{}, s);
    if (e != hipSuccess) return e;
    rows_totals_kernel<<<1, 1, 0, s>>>(P, code, off, totals);
    if (src)
        rows_emit_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, code, off, totals, N, capacity, src, kind, draw_row);
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------ apply
constexpr int ROWS_BLOCK_CAP = 16384;      // workgroups per tensor, the grid stride covers the rest

struct ChildArgs {
    const float* rotation_raw;
    const float* std;
    const float* z;
    long long n_draws;
    float shrink;        // 0.8 N
    int log_scaling;
    int half_xyz;        // the parent position is get_xyz: rounded through fp16 when the model is quantisation aware
};

// component `col` of R(q) (z * std) + get_xyz, R = build_rotation (utils/general_utils.py:84-107) of the raw quaternion
__device__ __forceinline__ float child_xyz(const ChildArgs& a, const float* __restrict__ xyz, int srow, long long draw, int col)
{
    const float* q4 = a.rotation_raw + 4 * (size_t)srow;
    const float qr = q4[0], qx = q4[1], qy = q4[2], qz = q4[3];
    const float norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
    const float r = qr / norm, x = qx / norm, y = qy / norm, z = qz / norm;
    const float* sd = a.std + 3 * (size_t)srow;
    const float* zz = a.z + 3 * (size_t)draw;
    const float s0 = zz[0] * sd[0], s1 = zz[1] * sd[1], s2 = zz[2] * sd[2];
    float R0, R1, R2;
    if (col == 0)      { R0 = 1.f - 2.f * (y * y + z * z); R1 = 2.f * (x * y - r * z); R2 = 2.f * (x * z + r * y); }
    else if (col == 1) { R0 = 2.f * (x * y + r * z); R1 = 1.f - 2.f * (x * x + z * z); R2 = 2.f * (y * z - r * x); }
    else               { R0 = 2.f * (x * z - r * y); R1 = 2.f * (y * z + r * x); R2 = 1.f - 2.f * (x * x + y * y); }
    float parent = xyz[3 * (size_t)srow + col];
    if (a.half_xyz) parent = __half2float(__float2half_rn(parent));
    return R0 * s0 + R1 * s1 + R2 * s2 + parent;
}

__global__ void __launch_bounds__(256)
rows_apply_kernel(const RowsJobs jobs, int P, long long P_new, const int32_t* __restrict__ src, const uint8_t* __restrict__ kind,
                  const int32_t* __restrict__ draw_row, const ChildArgs ca)
{
    const int jb = job_of_block(jobs);
    const c3dgs_rows_tensor t = jobs.t[jb];
    const int rf = t.row_floats;
    const long long total = P_new * rf;
    const bool small = total < (1ll << 32);
    const bool has_m = t.in_exp_avg != nullptr;
    // Lane-transposed: a workgroup step covers 1024 consecutive output floats, wave-instruction u of a wave its own 256 contiguous
    // bytes. Four consecutive floats per lane (float4 stores) made the four gather instructions of a lane share every source line
    // and fetched each line about twice (profiles/r06_apply_pmc.txt).
    const long long stride = (long long)jobs.nblocks[jb] * 1024;
    for (long long base = (long long)(blockIdx.x - jobs.first_block[jb]) * 1024 + threadIdx.x; base < total; base += stride) {
        float v[4], m[4], q[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long f = base + u * 256;
            v[u] = m[u] = q[u] = 0.f;
            if (f >= total) continue;
            const long long row = small ? (long long)((uint32_t)f / (uint32_t)rf) : f / rf;
            const int col = (int)(f - row * rf);
            int srow = src[row];
            const int kd = kind[row];
            const bool child = kd >= C3DGS_KIND_CHILD;
            long long draw = -1;
            if (child && t.role == C3DGS_ROLE_XYZ) {
                draw = draw_row[row];
                if (draw < 0 || draw >= ca.n_draws) srow = -1;
            }
            if (srow < 0 || srow >= P) continue;                                 // a bad plan writes zeros, never reads out of bounds
            const size_t at = (size_t)srow * rf + col;
            if (child && t.role == C3DGS_ROLE_XYZ) v[u] = child_xyz(ca, t.in_param, srow, draw, col);
            else if (child && t.role == C3DGS_ROLE_SCALING) {
                const float sc = ca.std[at] / ca.shrink;
                v[u] = ca.log_scaling ? logf(sc) : sc;
            } else v[u] = t.in_param[at];
            if (has_m && kd == C3DGS_KIND_ORIGINAL) { m[u] = t.in_exp_avg[at]; q[u] = t.in_exp_avg_sq[at]; }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long f = base + u * 256;
            if (f >= total) continue;
            t.out_param[f] = v[u];
            if (has_m) { t.out_exp_avg[f] = m[u]; t.out_exp_avg_sq[f] = q[u]; }
        }
    }
}

void launch_rows_apply(int P, long long P_new, const int32_t* src, const uint8_t* kind, const int32_t* draw_row, int n_tensors,
                       const c3dgs_rows_tensor* tensors, int N, long long n_draws, const float* rotation_raw, const float* std,
                       const float* z, int log_scaling, int half_xyz, hipStream_t s)
{
    RowsJobs J;
    for (int k = 0; k < n_tensors; k++) {
        if (!tensors[k].out_param) continue;
        const long long steps = (P_new * tensors[k].row_floats + 1023) / 1024;     // 1024 floats per workgroup step
        J.add(tensors[k], (steps + 1) / 2, ROWS_BLOCK_CAP);
    }
    if (J.n == 0 || P_new <= 0) return;
    const ChildArgs ca = { rotation_raw, std, z, n_draws, (float)(0.8 * N), log_scaling, half_xyz };
    rows_apply_kernel<<<J.grid(), 256, 0, s>>>(J, P, P_new, src, kind, draw_row, ca);
}

// ------------------------------------------------------------------------------------------------ stats
__global__ void __launch_bounds__(256)
densify_stats_kernel(int P, const float* __restrict__ grad, const uint8_t* __restrict__ filter, const int32_t* __restrict__ radii,
                     float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ max_radii)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !filter[i]) return;
    const float gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.f;
    if (radii) {
        const float r = (float)radii[i], mr = max_radii[i];
        max_radii[i] = (r > mr || r != r) ? r : mr;
    }
}

void launch_densify_stats(int P, const float* grad, const uint8_t* filter, const int32_t* radii, float* accum, float* denom,
                          float* max_radii, hipStream_t s)
{
    densify_stats_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, grad, filter, radii, accum, denom, max_radii);
}

} // namespace c3dgs
