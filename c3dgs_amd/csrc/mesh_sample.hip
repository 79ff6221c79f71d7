// mesh_sample.hip -- points on a triangle mesh at a given number per unit area (no reference counterpart): what a DTU-style
// evaluation compares with the scanned cloud. Defined without a floating-point prefix sum, so nothing depends on a scan order, and
// compiled without contraction: every fp32 operation is rounded on its own, in the order written, and tests/geometry_ref.py repeats
// them in NumPy bit for bit.
//
//   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16        (32-bit, wrapping)
//   base(f) = mix(mix(f) ^ seed);   u24(x) = float(x >> 8) * 2^-24                              (exact: in [0, 1))
// COUNT, one lane per face (mesh_sample_count_kernel): with the corners a, b, c and u = b - a, v = c - a,
//   cx = u.y v.z - u.z v.y, cy = u.z v.x - u.x v.z, cz = u.x v.y - u.y v.x;  area = 0.5 sqrt((cx cx + cy cy) + cz cz)   (sqrt_rn)
//   t = area * density;   n_f = int(floor(t)) + (u24(base(f)) < t - floor(t) ? 1 : 0)            stochastic rounding, E[n_f] = t
//   a non-finite t: n_f = 0. A vertex index outside [0, V) (never dereferenced) or a finite t >= 2^24 sets a bit of the flag word.
// The lane stores the face's exclusive prefix WITHIN its workgroup of 256 faces; lane 0 the workgroup's total.
// SCAN (mesh_sample_scan_kernel, one workgroup): the 64-bit grand total, then scan_blocks.hpp over the workgroup totals; the total
// and the flag word sit side by side, the host's one read. A workgroup total or a grand total above 2^31 - 1 sets a flag bit.
// EMIT, one lane per SAMPLE (mesh_sample_emit_kernel): sample s belongs to the last face f whose prefix is <= s -- a binary search
// over the workgroup bases, then one over the 256 prefixes of that workgroup -- and is its sample k = s - prefix(f):
//   u1 = u24(mix(base(f) + 2k + 1)), u2 = u24(mix(base(f) + 2k + 2));  if u1 + u2 > 1: u1 = 1 - u1, u2 = 1 - u2
//   p = (a + u1 (b - a)) + u2 (c - a)  per component
// so the output is ordered by face, then by k. A lane per face looping n_f times would leave a wave waiting on its largest triangle.
// Bounds: count reads 12 B of indices and three gathered vertices per face; emit is one 16-byte row out per sample behind about
// 8 + log2(F / 256) dependent 4-byte loads of the search, which neighbouring lanes share: latency of the search, then store bandwidth.
#include "common.hpp"
#include "scan_blocks.hpp"
#include <cfloat>

namespace c3dgs {

namespace {

constexpr int MS_BLOCK = 256;
constexpr uint32_t MS_BAD_INDEX = 1u, MS_BAD_COUNT = 2u, MS_BAD_TOTAL = 4u;

__device__ __forceinline__ uint32_t ms_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t ms_base(const uint32_t f, const uint32_t seed) { return ms_mix(ms_mix(f) ^ seed); }
__device__ __forceinline__ float ms_u24(const uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-08f; }

struct MsTri { float a[3], b[3], c[3]; bool ok; };

// the three corners of face f; ok = every index is inside [0, V) (else nothing was loaded)
__device__ __forceinline__ MsTri ms_load(const int V, const float* __restrict__ vertices, const int32_t* __restrict__ faces, const size_t f)
{
    MsTri t{};
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    t.ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
    if (!t.ok) return t;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        t.a[q] = vertices[3 * (size_t)i0 + q]; t.b[q] = vertices[3 * (size_t)i1 + q]; t.c[q] = vertices[3 * (size_t)i2 + q];
    }
    return t;
}

// totals: [0..1] the 64-bit grand total, [2] the flag word
__global__ void __launch_bounds__(MS_BLOCK)
mesh_sample_count_kernel(const int V, const float* __restrict__ vertices, const int F, const int32_t* __restrict__ faces,
                         const float density, const uint32_t seed, uint32_t* __restrict__ prefix, uint32_t* __restrict__ block_t,
                         uint32_t* __restrict__ totals)
{
    __shared__ uint32_t s_w[MS_BLOCK / 64];
    const uint32_t f = blockIdx.x * (uint32_t)MS_BLOCK + threadIdx.x;
    uint32_t n = 0, bad = 0;
    if (f < (uint32_t)F) {
        const MsTri tri = ms_load(V, vertices, faces, f);
        if (!tri.ok) bad = MS_BAD_INDEX;
        else {
            const float ux = tri.b[0] - tri.a[0], uy = tri.b[1] - tri.a[1], uz = tri.b[2] - tri.a[2];
            const float vx = tri.c[0] - tri.a[0], vy = tri.c[1] - tri.a[1], vz = tri.c[2] - tri.a[2];
            const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
            const float area = 0.5f * sqrtf(cx * cx + cy * cy + cz * cz);
            const float t = area * density;
            if (fabsf(t) <= FLT_MAX) {                                     // a NaN or an overflowed area: no sample
                if (t >= 16777216.f) bad = MS_BAD_COUNT;
                else if (t > 0.f) {
                    const float fl = floorf(t);
                    n = (uint32_t)fl + (ms_u24(ms_base(f, seed)) < t - fl ? 1u : 0u);
                }
            }
        }
    }
    // exclusive prefix within the workgroup: n <= 2^24 each, so 256 of them reach 2^32 only when all are 2^24 -- caught below
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t off = 0;
    unsigned long long total = 0;
#pragma unroll
    for (int q = 0; q < MS_BLOCK / 64; q++) { const uint32_t x = s_w[q]; if (q < wave) off += x; total += x; }
    if (f < (uint32_t)F) prefix[f] = off + incl - n;
    if (total > 0x7fffffffull) { bad |= MS_BAD_TOTAL; total = 0; }         // each wave's sum is at most 2^30: `total` is exact
    if (threadIdx.x == 0) block_t[blockIdx.x] = (uint32_t)total;
    if (bad) atomicOr(&totals[2], bad);
}

__global__ void __launch_bounds__(SCAN_BLOCKS_THREADS)
mesh_sample_scan_kernel(const int nb, uint32_t* __restrict__ block_t, uint32_t* __restrict__ totals)
{
    __shared__ unsigned long long s_t[SCAN_BLOCKS_THREADS / 64];
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < nb; i += SCAN_BLOCKS_THREADS) sum += block_t[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) s_t[threadIdx.x >> 6] = sum;
    __syncthreads();                                        // every read of the totals precedes the scan's stores
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < SCAN_BLOCKS_THREADS / 64; w++) all += s_t[w];
        totals[0] = (uint32_t)all; totals[1] = (uint32_t)(all >> 32);
    }
    scan_blocks_body(nb, block_t, nullptr, nullptr, 0u);
}

__global__ void __launch_bounds__(MS_BLOCK)
mesh_sample_emit_kernel(const int V, const float* __restrict__ vertices, const int F, const int32_t* __restrict__ faces,
                        const uint32_t seed, const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ block_t, const int nb,
                        const uint32_t S, float* __restrict__ points, int32_t* __restrict__ face)
{
    const uint32_t s = blockIdx.x * (uint32_t)MS_BLOCK + threadIdx.x;
    if (s >= S) return;
    // the last workgroup whose base is <= s, then the last face of it whose prefix is <= s - base (both exist: entry 0 is 0)
    int lo = 0, hi = nb;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (block_t[mid] <= s) lo = mid; else hi = mid; }
    const uint32_t base = block_t[lo], r = s - base;
    int f0 = lo * MS_BLOCK, f1 = min(F, f0 + MS_BLOCK);
    while (f1 - f0 > 1) { const int mid = (f0 + f1) >> 1; if (prefix[mid] <= r) f0 = mid; else f1 = mid; }
    const uint32_t k = r - prefix[f0];
    const MsTri tri = ms_load(V, vertices, faces, (size_t)f0);
    float p[3] = { 0.f, 0.f, 0.f };
    if (tri.ok) {                                           // (the count refused the mesh otherwise)
        const uint32_t h = ms_base((uint32_t)f0, seed);
        float u1 = ms_u24(ms_mix(h + 2u * k + 1u)), u2 = ms_u24(ms_mix(h + 2u * k + 2u));
        if (u1 + u2 > 1.f) { u1 = 1.f - u1; u2 = 1.f - u2; }
#pragma unroll
        for (int q = 0; q < 3; q++) p[q] = (tri.a[q] + u1 * (tri.b[q] - tri.a[q])) + u2 * (tri.c[q] - tri.a[q]);
    }
    points[3 * (size_t)s] = p[0]; points[3 * (size_t)s + 1] = p[1]; points[3 * (size_t)s + 2] = p[2];
    face[s] = f0;
}

inline int ms_blocks(const int F) { return (F + MS_BLOCK - 1) / MS_BLOCK; }

struct MsWs { uint32_t* prefix; uint32_t* block_t; uint32_t* totals; size_t bytes; };

// [prefix: a word per face][block_t: a word per workgroup, scan_blocks.hpp's slack][totals: the grand total and the flag word]
MsWs ms_ws(void* ws, const int F)
{
    const size_t nb = (size_t)ms_blocks(F);
    char* p = (char*)ws;
    MsWs w;
    size_t at = 0;
    w.prefix = (uint32_t*)(p + at); at += align_up((size_t)(F > 0 ? F : 1) * 4);
    w.block_t = (uint32_t*)(p + at); at += align_up(((nb + 2 + 15) & ~(size_t)15) * 4);
    w.totals = (uint32_t*)(p + at); at += 256;
    w.bytes = at;
    return w;
}

} // namespace

size_t mesh_sample_workspace_bytes(int F) { return ms_ws(nullptr, F).bytes; }

hipError_t mesh_sample_clear(int F, void* ws, hipStream_t s) { return hipMemsetAsync(ms_ws(ws, F).totals, 0, 16, s); }

void launch_mesh_sample_count(int V, const float* vertices, int F, const int32_t* faces, float density, uint32_t seed, void* ws,
                              hipStream_t s)
{
    const MsWs w = ms_ws(ws, F);
    mesh_sample_count_kernel<<<ms_blocks(F), MS_BLOCK, 0, s>>>(V, vertices, F, faces, density, seed, w.prefix, w.block_t, w.totals);
}

// -> the device words {total low, total high, flags}
const uint32_t* launch_mesh_sample_scan(int F, void* ws, hipStream_t s)
{
    const MsWs w = ms_ws(ws, F);
    mesh_sample_scan_kernel<<<1, SCAN_BLOCKS_THREADS, 0, s>>>(ms_blocks(F), w.block_t, w.totals);
    return w.totals;
}

void launch_mesh_sample_emit(int V, const float* vertices, int F, const int32_t* faces, uint32_t seed, const void* ws, uint32_t S,
                             float* points, int32_t* face, hipStream_t s)
{
    const MsWs w = ms_ws(const_cast<void*>(ws), F);
    mesh_sample_emit_kernel<<<(S + MS_BLOCK - 1) / MS_BLOCK, MS_BLOCK, 0, s>>>(V, vertices, F, faces, seed, w.prefix, w.block_t,
                                                                               ms_blocks(F), S, points, face);
}

} // namespace c3dgs
