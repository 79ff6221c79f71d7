// mcmc.hip -- MCMC density control ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy) for non-indexed
// models (gfx950, wave64). Not in the reference. A hard budget of Gaussians instead of clone / split thresholds:
//
//   sample   weights   one thread per row: o = sigmoid(raw opacity) in fp32, q = floor(o 2^20) as an INTEGER weight (0 for an
//                      excluded row), the inclusive prefix of q inside its block of 256 rows, the block's total; counts zeroed
//            scan      one workgroup: the 64-bit exclusive prefix of the block totals, base[nb] = T  (5000 rows of opacity 0.99
//                      already exceed 2^32; scan_blocks.hpp is a 32-bit scan, this is the 64-bit level)
//            search    one thread per draw: t = min(T - 1, floor(u T)), first the block by bisection of base[], then the row by
//                      bisection of the block's local prefix; counts by integer atomics
//            Integer weights make the prefix exact and independent of the scan order: the sources are bitwise reproducible and
//            can be checked index for index against a host restatement.
//   values   one thread per row with count > 0: the relocation opacity and scale factor (the paper's eq. 9), in DOUBLE from the
//            raw fp32 opacity (fp32 is off by 1e-4 relative at N = 51), written in raw space into the workspace
//   apply    ONE launch over a table of tensors, in place: destination rows take their source's row (copy_rows) and its staged
//            opacity / scale, every source takes its own staged values, both moments of both become zero. Every value it reads
//            is either staged or in a row this launch does not write.
//   noise    the per-iteration step, one lane per Gaussian: xyz += R (s^2 * (R^T xi)) g(o) noise_lr xyz_lr; the 3x3 covariance
//            is never formed in memory. fp32, no LDS, no atomics, about 72 bytes per row.
// Compiled with -ffp-contract=off: t = floor(u * T) is ONE IEEE multiply, which the host restatement repeats bit for bit.
#include "mcmc.hpp"
#include "jobs.hpp"
#include <cfloat>

namespace c3dgs {

constexpr int MB = MCMC_BLOCK_ROWS;

// ------------------------------------------------------------------------------------------------ sample
__device__ __forceinline__ float mcmc_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// DERIVE: dead_i = (o_i <= min_opacity), written to dead_out; otherwise `dead` (or nobody, when it is null) is excluded
template <bool DERIVE>
__global__ void __launch_bounds__(MB)
mcmc_weights_kernel(long long P, const float* __restrict__ raw_opacity, const uint8_t* __restrict__ dead, float min_opacity,
                    uint8_t* __restrict__ dead_out, uint32_t* __restrict__ q_out, int32_t* __restrict__ counts,
                    uint32_t* __restrict__ local, uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_w[MB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * MB + threadIdx.x;
    uint32_t q = 0;
    if (row < P) {
        const float o = mcmc_sigmoid(raw_opacity[row]);
        bool excluded;
        if (DERIVE) { excluded = o <= min_opacity; dead_out[row] = excluded ? 1 : 0; }
        else excluded = dead != nullptr && dead[row] != 0;
        if (!excluded && o > 0.f) q = (uint32_t)floorf(o * 1048576.f);       // o <= 1: q <= 2^20; a NaN opacity weighs nothing
        q_out[row] = q;
        counts[row] = 0;
    }
    uint32_t incl = q;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d); if (lane >= d) incl += u; }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MB / 64; w++) if (w < wave) incl += s_w[w];          // <= 256 * 2^20 = 2^28
    if (row < P) local[row] = incl;
    if (threadIdx.x == MB - 1) total[blockIdx.x] = incl;
}

// exclusive 64-bit prefix of the nb block totals, one workgroup; base[nb] = *T_out = T
__global__ void __launch_bounds__(MCMC_SCAN_THREADS)
mcmc_scan_kernel(int nb, const uint32_t* __restrict__ total, unsigned long long* __restrict__ base, unsigned long long* __restrict__ T_out)
{
    __shared__ unsigned long long s_w[2][MCMC_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int SWEEP = MCMC_SCAN_THREADS * MCMC_SCAN_PER_THREAD;
    unsigned long long carry = 0;                         // every thread tracks the running total itself
    int buf = 0;
    for (int c0 = 0; c0 < nb; c0 += SWEEP, buf ^= 1) {
        const int i0 = c0 + t * MCMC_SCAN_PER_THREAD;
        uint32_t v[MCMC_SCAN_PER_THREAD];
        unsigned long long mine = 0;
#pragma unroll
        for (int k = 0; k < MCMC_SCAN_PER_THREAD; k++) { v[k] = i0 + k < nb ? total[i0 + k] : 0u; mine += v[k]; }
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long u = __shfl_up(incl, d); if (lane >= d) incl += u; }
        if (lane == 63) s_w[buf][wave] = incl;
        __syncthreads();                                  // s_w is double-buffered: one barrier per sweep
        unsigned long long off = carry, all = 0;
#pragma unroll
        for (int w = 0; w < MCMC_SCAN_THREADS / 64; w++) { const unsigned long long x = s_w[buf][w]; if (w < wave) off += x; all += x; }
        unsigned long long run = off + incl - mine;
#pragma unroll
        for (int k = 0; k < MCMC_SCAN_PER_THREAD; k++) { if (i0 + k < nb) base[i0 + k] = run; run += v[k]; }
        carry += all;
    }
    if (t == 0) { base[nb] = carry; *T_out = carry; }
}

__global__ void __launch_bounds__(256)
mcmc_search_kernel(long long P, int nb, long long n, const double* __restrict__ draws, const unsigned long long* __restrict__ base,
                   const uint32_t* __restrict__ local, int32_t* __restrict__ sources, int32_t* __restrict__ counts)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long T = base[nb];
    if (T == 0) { sources[j] = -1; return; }              // nothing has weight: nothing is sampled
    const double x = floor(draws[j] * (double)T);         // T < 2^51 is exact in a double; one multiply
    unsigned long long t = x > 0.0 ? (unsigned long long)x : 0ull;
    if (t > T - 1) t = T - 1;
    int lo = 0, hi = nb;                                  // the largest b with base[b] <= t: base[0] = 0 <= t < T = base[nb]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t r = (uint32_t)(t - base[lo]);          // < the block's total, since base[lo + 1] > t
    const long long first = (long long)lo * MB;
    const long long rows = P - first < MB ? P - first : MB;
    int a = -1, b = (int)rows - 1;                        // the smallest i with local[first + i] > r: local[first + rows - 1] = total > r
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (local[first + mid] > r) b = mid; else a = mid;
    }
    const long long src = first + b;
    sources[j] = (int32_t)src;
    atomicAdd(&counts[src], 1);
}

void launch_mcmc_weights(int64_t P, const float* raw_opacity, const uint8_t* dead, int derive, float min_opacity, uint8_t* dead_out,
                         uint32_t* q, int32_t* counts, unsigned long long* T, void* workspace, hipStream_t s)
{
    const McmcLayout L = mcmc_layout(P);
    char* w = (char*)workspace;
    uint32_t* local = (uint32_t*)(w + L.local);
    uint32_t* total = (uint32_t*)(w + L.total);
    unsigned long long* base = (unsigned long long*)(w + L.base);
    const int nb = (int)((P + MB - 1) / MB);
    if (derive) mcmc_weights_kernel<true><<<nb, MB, 0, s>>>(P, raw_opacity, nullptr, min_opacity, dead_out, q, counts, local, total);
    else mcmc_weights_kernel<false><<<nb, MB, 0, s>>>(P, raw_opacity, dead, min_opacity, nullptr, q, counts, local, total);
    mcmc_scan_kernel<<<1, MCMC_SCAN_THREADS, 0, s>>>(nb, total, base, T);
}

void launch_mcmc_search(int64_t P, int64_t n, const double* draws, int32_t* sources, int32_t* counts, const void* workspace,
                        hipStream_t s)
{
    const McmcLayout L = mcmc_layout(P);
    const char* w = (const char*)workspace;
    const int nb = (int)((P + MB - 1) / MB);
    mcmc_search_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(P, nb, n, draws, (const unsigned long long*)(w + L.base),
                                                                  (const uint32_t*)(w + L.local), sources, counts);
}

// ------------------------------------------------------------------------------------------------ relocation values
struct McmcBinom {
    double c[MCMC_MAX_N][MCMC_MAX_N];       // c[n][k] = C(n, k), exact in a double (C(50, 25) < 2^47)
    constexpr McmcBinom() : c{}
    {
        for (int n = 0; n < MCMC_MAX_N; n++) {
            for (int k = 0; k < MCMC_MAX_N; k++) c[n][k] = 0.0;
            c[n][0] = 1.0;
            for (int k = 1; k <= n; k++) c[n][k] = c[n - 1][k - 1] + c[n - 1][k];
        }
    }
};
__constant__ McmcBinom kMcmcBinom = McmcBinom();

// o' = 1 - (1 - o)^(1/N) clamped to [min_opacity, 1 - FLT_EPSILON];  c = o / sum_{i=1..N} sum_{k<i} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1).
// The double sum runs k outermost, so that o'^(k+1) / sqrt(k+1) is formed once per k and no per-lane array is needed.
__global__ void __launch_bounds__(256)
mcmc_values_kernel(long long P, const int32_t* __restrict__ counts, const float* __restrict__ raw_opacity,
                   const float* __restrict__ raw_scale, int scale_floats, float min_opacity, float* __restrict__ new_opacity,
                   float* __restrict__ new_scale)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int cnt = counts[i];
    if (cnt <= 0) return;
    const int N = cnt + 1 < MCMC_MAX_N ? cnt + 1 : MCMC_MAX_N;
    // o itself in double from the raw fp32 parameter: near o = 1 the fp32 sigmoid has lost 1 - o, which o' is made of
    const double x = (double)raw_opacity[i];
    const double o = 1.0 / (1.0 + exp(-x));
    double on = -expm1(-log1p(exp(x)) / (double)N);                       // 1 - (1 - o)^(1/N), with log(1 - o) = -log(1 + e^x)
    const double lo = (double)min_opacity, hi = 1.0 - (double)FLT_EPSILON;
    on = on < lo ? lo : (on > hi ? hi : on);
    double denom = 0.0, pw = on, sign = 1.0;
    for (int k = 0; k < N; k++) {
        const double a = sign * pw / sqrt((double)(k + 1));
        double bsum = 0.0;
        for (int m = k; m < N; m++) bsum += kMcmcBinom.c[m][k];          // i - 1 = m: the rows of the triangle that hold column k
        denom += bsum * a;
        pw *= on; sign = -sign;
    }
    const double logc = log(o / denom);
    new_opacity[i] = (float)(log(on) - log1p(-on));                       // logit, rounded once
    for (int col = 0; col < scale_floats; col++)
        new_scale[3 * i + col] = (float)((double)raw_scale[i * scale_floats + col] + logc);
}

void launch_mcmc_values(int64_t P, const int32_t* counts, const float* raw_opacity, const float* raw_scale, int scale_floats,
                        float min_opacity, void* workspace, hipStream_t s)
{
    const McmcLayout L = mcmc_layout(P);
    char* w = (char*)workspace;
    mcmc_values_kernel<<<(unsigned)((P + 255) / 256), 256, 0, s>>>(P, counts, raw_opacity, raw_scale, scale_floats, min_opacity,
                                                                  (float*)(w + L.new_opacity), (float*)(w + L.new_scale));
}

// ------------------------------------------------------------------------------------------------ apply
constexpr int MCMC_APPLY_BLOCK_CAP = 8192;     // workgroups per tensor, the grid stride covers the rest

// A tensor's lanes run over 2 n row_floats elements: the first half are the destination rows, the second half the source of
// every pair (a source drawn k times is written k times with the same staged words). Reads: sources[], dst[], the staged
// values, and with copy_rows the source's row of a COPY tensor, which no lane writes (a source is never a destination).
__global__ void __launch_bounds__(256)
mcmc_apply_kernel(const RowsJobs jobs, long long P, long long n, const int32_t* __restrict__ dst, long long dst_base,
                  const int32_t* __restrict__ sources, int copy_rows, const float* __restrict__ new_opacity,
                  const float* __restrict__ new_scale)
{
    const int jb = job_of_block(jobs);
    const c3dgs_rows_tensor t = jobs.t[jb];
    const int rf = t.row_floats;
    const long long half = n * rf, total = 2 * half;
    const long long stride = (long long)jobs.nblocks[jb] * 256;
    const bool has_m = t.out_exp_avg != nullptr;
    for (long long e = (long long)(blockIdx.x - jobs.first_block[jb]) * 256 + threadIdx.x; e < total; e += stride) {
        const bool is_src = e >= half;
        const long long f = is_src ? e - half : e;
        const long long j = f / rf;
        const int col = (int)(f - j * rf);
        const long long src = sources[j];
        if (src < 0 || src >= P) continue;                                    // T == 0: nothing was sampled
        const long long row = is_src ? src : (dst ? (long long)dst[j] : dst_base + j);
        if (row < 0 || row >= P) continue;                                    // a bad list writes nothing
        const size_t at = (size_t)row * rf + col;
        if (t.role == C3DGS_MCMC_ROLE_OPACITY) t.out_param[at] = new_opacity[src];
        else if (t.role == C3DGS_MCMC_ROLE_SCALE) t.out_param[at] = new_scale[3 * src + col];
        else if (!is_src && copy_rows) t.out_param[at] = t.in_param[(size_t)src * rf + col];
        if (has_m) { t.out_exp_avg[at] = 0.f; t.out_exp_avg_sq[at] = 0.f; }
    }
}

void launch_mcmc_apply(int64_t P, int64_t n, const int32_t* dst, int64_t dst_base, const int32_t* sources, int n_tensors,
                       const c3dgs_rows_tensor* tensors, int copy_rows, const void* workspace, hipStream_t s)
{
    const McmcLayout L = mcmc_layout(P);
    const char* w = (const char*)workspace;
    RowsJobs J;
    for (int k = 0; k < n_tensors; k++) J.add(tensors[k], (2 * n * tensors[k].row_floats + 255) / 256, MCMC_APPLY_BLOCK_CAP);
    if (J.n == 0 || n <= 0) return;
    mcmc_apply_kernel<<<J.grid(), 256, 0, s>>>(J, P, n, dst, dst_base, sources, copy_rows, (const float*)(w + L.new_opacity),
                                         (const float*)(w + L.new_scale));
}

// ------------------------------------------------------------------------------------------------ noise
__global__ void __launch_bounds__(256)
mcmc_noise_kernel(long long P, float* __restrict__ xyz, const float* __restrict__ rotation, const float* __restrict__ scaling,
                  const float* __restrict__ scaling_factor, const float* __restrict__ raw_opacity, const float* __restrict__ xi,
                  float noise_lr, float xyz_lr)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float qr = rotation[4 * i], qx = rotation[4 * i + 1], qy = rotation[4 * i + 2], qz = rotation[4 * i + 3];
    const float qn = fmaxf(sqrtf(qr * qr + qx * qx + qy * qy + qz * qz), 1e-12f);          // torch.nn.functional.normalize
    const float r = qr / qn, x = qx / qn, y = qy / qn, z = qz / qn;
    float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
    if (scaling_factor) {                                                                  // normalize(relu(.)) * exp(factor)
        s0 = fmaxf(s0, 0.f); s1 = fmaxf(s1, 0.f); s2 = fmaxf(s2, 0.f);
        const float sn = fmaxf(sqrtf(s0 * s0 + s1 * s1 + s2 * s2), 1e-12f), fac = expf(scaling_factor[i]);
        s0 = s0 / sn * fac; s1 = s1 / sn * fac; s2 = s2 / sn * fac;
    } else { s0 = expf(s0); s1 = expf(s1); s2 = expf(s2); }
    const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
    const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
    const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    const float e0 = xi[3 * i], e1 = xi[3 * i + 1], e2 = xi[3 * i + 2];
    const float v0 = (R00 * e0 + R10 * e1 + R20 * e2) * (s0 * s0);                         // s^2 * (R^T xi)
    const float v1 = (R01 * e0 + R11 * e1 + R21 * e2) * (s1 * s1);
    const float v2 = (R02 * e0 + R12 * e1 + R22 * e2) * (s2 * s2);
    const float o = mcmc_sigmoid(raw_opacity[i]);
    const float g = 1.f / (1.f + expf(-100.f * ((1.f - o) - 0.995f)));
    const float k = g * noise_lr * xyz_lr;
    xyz[3 * i] += (R00 * v0 + R01 * v1 + R02 * v2) * k;
    xyz[3 * i + 1] += (R10 * v0 + R11 * v1 + R12 * v2) * k;
    xyz[3 * i + 2] += (R20 * v0 + R21 * v1 + R22 * v2) * k;
}

void launch_mcmc_noise(int64_t P, float* xyz, const float* rotation, const float* scaling, const float* scaling_factor,
                       const float* raw_opacity, const float* xi, float noise_lr, float xyz_lr, hipStream_t s)
{
    mcmc_noise_kernel<<<(unsigned)((P + 255) / 256), 256, 0, s>>>(P, xyz, rotation, scaling, scaling_factor, raw_opacity, xi,
                                                                 noise_lr, xyz_lr);
}

} // namespace c3dgs
