// render_common.hpp -- what the blend kernels of render.hip (forward, backward) and render_depth.hip (depth / alpha / median
// replay) must share to take the same decisions bit for bit: the staged batch size, the pre-scaled conic, the alpha
// expression, the quadrant cull and the workgroup -> tile banding; the slot numbering of the (Gaussian, tile) entries; and the
// transposing butterfly that the per-Gaussian passes reduce with, so that they sum in the same order. One owner; device code
// only (but for banded_grid). The skeleton of the passes that replay a finished forward is replay.hpp.
#pragma once
#include "common.hpp"

namespace c3dgs {

constexpr int BATCH = 256;

// The staged LDS records carry the conic PRE-SCALED for the blend loops: {-0.5 a, -b, -0.5 c} x log2(e), so that the
// exponent of  G = exp(-0.5 (a dx^2 + c dy^2) - b dx dy)  is three multiplies and three multiply-adds feeding v_exp_f32
// (= 2^x) directly: two vector instructions per (pixel, Gaussian) pair fewer than the reference's form + exp (which is
// exp2 of a product with log2(e) on this hardware anyway). Done once per staged entry, after the culling mask, which
// works on the true conic.
__device__ __forceinline__ void prescale_conic(float4& a, float4& b)
{
    constexpr float LOG2E = 1.4426950408889634f;
    a.z *= -0.5f * LOG2E;
    a.w *= -LOG2E;
    b.x *= -0.5f * LOG2E;
}

// alpha of one Gaussian at one pixel; the SAME instruction sequence in forward and backward so both
// take identical skip decisions (explicit fma placement, independent of -ffp-contract).
// (ka, kb, kc) = the pre-scaled conic of prescale_conic().
// returns false when the reference `continue`s (forward.cu:344-354 / backward.cu:494-501).
__device__ __forceinline__ bool gaussian_alpha(float mx, float my, float ka, float kb, float kc, float op,
                                               float pxf, float pyf, float& dx, float& dy, float& G, float& alpha)
{
    dx = mx - pxf;
    dy = my - pyf;
    const float power2 = fmaf(kb, dx * dy, fmaf(kc, dy * dy, ka * (dx * dx)));     // = power * log2(e)
    // no early return: G and alpha are always written (callers select on the result anyway), which saves the compiler
    // a select per call; for power > 0 they hold values nobody uses
    G = __builtin_amdgcn_exp2f(power2);
    alpha = fminf(0.99f, op * G);
    return !(power2 > 0.0f) && !(alpha < 1.0f / 255.0f);
}

// Which of the tile's four 8x8 quadrants (= waves) can this Gaussian touch at all?  A pixel only blends the
// Gaussian if alpha = min(0.99, o*exp(power)) >= 1/255, i.e. f(d) = 0.5*d^T C d <= tau with tau = ln(255*o).
// f is convex, so its minimum over a quadrant's pixel rectangle is 0 if the mean lies inside it and otherwise sits
// on one of the four edges, where it is a clamped 1-D parabola minimum. A quadrant whose minimum exceeds tau
// (inflated by 1e-4 relative + 1e-4 absolute and 0.01 px of rectangle slack, far above the fp32 error of the
// per-pixel test) contains no contributing pixel, so skipping it changes no result. Bit q = qy*2+qx.
// Anything non-finite or non-positive-definite -> no culling.
__device__ __forceinline__ float min_power_on_rect(float ca, float cb, float cc, float nb_c, float nb_a,
                                                   float dx0, float dx1, float dy0, float dy1)
{
    if (dx0 <= 0.f && dx1 >= 0.f && dy0 <= 0.f && dy1 >= 0.f) return 0.f;
    auto f = [&](float dx, float dy) { return 0.5f * (ca * dx * dx + cc * dy * dy) + cb * dx * dy; };
    const float ya = fminf(fmaxf(nb_c * dx0, dy0), dy1), yb = fminf(fmaxf(nb_c * dx1, dy0), dy1);
    const float xa = fminf(fmaxf(nb_a * dy0, dx0), dx1), xb = fminf(fmaxf(nb_a * dy1, dx0), dx1);
    return fminf(fminf(f(dx0, ya), f(dx1, yb)), fminf(f(xa, dy0), f(xb, dy1)));
}

__device__ __forceinline__ uint32_t quadrant_mask(const float4 a, const float4 b, float tile_x0, float tile_y0)
{
    const float mx = a.x, my = a.y, ca = a.z, cb = a.w, cc = b.x, op = b.y;
    if (op < (1.0f / 255.0f) * 0.999f) return 0u;          // alpha <= o < 1/255 everywhere
    const float det = ca * cc - cb * cb;
    const float tau = __logf(255.0f * op) * 1.0001f + 1e-4f;
    if (!(det > 0.0f) || !(ca > 0.0f) || !(cc > 0.0f) || !(tau < 1e30f)) return 0xfu;
    const float nb_c = -cb / cc, nb_a = -cb / ca;           // argmin of f along a vertical / horizontal line
    uint32_t mask = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float x0 = tile_x0 + (float)((q & 1) * 8) - 0.01f - mx, y0 = tile_y0 + (float)((q >> 1) * 8) - 0.01f - my;
        const float fmin = min_power_on_rect(ca, cb, cc, nb_c, nb_a, x0, x0 + 7.02f, y0, y0 + 7.02f);
        mask |= (uint32_t)(!(fmin > tau)) << q;              // NaN -> keep
    }
    return mask;
}

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// XCD-aware tile order: workgroups b, b+8, b+16, ... share an XCD (and its L2) under the observed
// round-robin dispatch, so give every XCD one contiguous band of row-major tiles. Speed only.
__device__ __forceinline__ int tile_of_block(int b, int T)
{
    const int chunk = (T + 7) >> 3;
    return (b & 7) * chunk + (b >> 3);
}
// the grid of that order: 8 bands of ceil(T / 8) workgroups; those that fall off the end of a band, or past T, have no tile
inline int banded_grid(int T) { return ((T + 7) / 8) * 8; }
__device__ __forceinline__ bool block_has_no_tile(uint32_t b, int T)
{
    return tile_of_block((int)b, T) >= T || (b >> 3) >= (uint32_t)((T + 7) >> 3);
}

// ---- the slots of the (Gaussian, tile) entries: the numbering of the backward's partial sums, which the per-Gaussian passes share
// The slot of Gaussian `id` in tile (tx, ty): first slot of the Gaussian + the tile's place in its rectangle. c = the third
// float4 of the Gaussian's splat record {-, first slot relative to block_base[id >> 8], y0 << 16 | x0, y1 << 16 | x1}.
__device__ __forceinline__ uint32_t entry_slot(const float4 c, const uint32_t* __restrict__ block_base, uint32_t id, int tx, int ty)
{
    const uint32_t off = __float_as_uint(c.y), lo = __float_as_uint(c.z), hi = __float_as_uint(c.w);
    const int x0 = lo & 0xffff, y0 = lo >> 16, x1 = hi & 0xffff;
    return block_base[id >> 8] + off + (uint32_t)((ty - y0) * (x1 - x0) + (tx - x0));
}

// Gaussian i's slots [start, end): the id-order scan of tiles_touched = per-workgroup inclusive offsets of the forward +
// block_base[] (preprocess.hip); the run's length is the rectangle's area
struct SlotRun { uint32_t start, end; };
__device__ __forceinline__ SlotRun slot_run(int i, const uint32_t* __restrict__ inst_offset, const uint32_t* __restrict__ block_base)
{
    SlotRun r;
    r.end = inst_offset[i] + block_base[i >> 8];
    r.start = (i == 0) ? 0u : inst_offset[i - 1] + block_base[(i - 1) >> 8];
    return r;
}

// ---- the transposing butterfly of the per-Gaussian passes (render_contrib.hip, render_error.hip): one network, so that both
// reduce in the same order
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

struct OpAdd { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// One level of the transposing butterfly: a lane pair (lane, its DPP partner) exchanges halves. Each lane keeps half of the N
// values it held and combines its partner's copy of that half into them.
template <int N, int CTRL, class Op>
__device__ __forceinline__ void transpose_step(float* v, bool hi, Op op)
{
#pragma unroll
    for (int k = 0; k < N / 2; k++) {
        const float keep = hi ? v[k + N / 2] : v[k];
        const float send = hi ? v[k] : v[k + N / 2];
        v[k] = op(keep, dpp_get<CTRL>(send));
    }
}

// v[0..7] = this pixel's value for the row's 8 candidates -> the reduction over the wave's 64 pixels of candidate
// beta(lane) = 4 * bit2 + 2 * bit0 + bit1 (render_backward's lane -> Gaussian map), in every lane.
//   8 -> 4  row_half_mirror (i <-> 7 - i), 4 -> 2  quad_perm [1,0,3,2], 2 -> 1  quad_perm [2,3,0,1]: 8 lanes per value
//   then three plain levels over the 8 pixel rows: row_ror:8, v_permlane16_swap, v_permlane32_swap
// Both operands of every combination are the same in the two lanes of a pair and op is commutative: all lanes that hold a
// candidate hold the same bits, and the order of the float sum is the network's, not the timing's.
// The network's two halves are also used apart (render_maps_backward.hip forms the y-moments of a pixel row between them, as
// render_backward_kernel does between its column and row levels: the same pairings, so the same sums).
__device__ __forceinline__ int candidate_of_lane(int lane)      // beta(lane): where this lane's reduced values belong
{
    return ((lane >> 2) & 1) * 4 + (lane & 1) * 2 + ((lane >> 1) & 1);
}

// columns: v[0..7] -> the reduction over the 8 pixels of this lane's pixel ROW of candidate beta(lane), in all 8 lanes of the row
template <class Op>
__device__ __forceinline__ float reduce_columns_of_8(float* v, int lane, Op op)
{
    transpose_step<8, 0x141>(v, (lane & 4) != 0, op);
    transpose_step<4, 0xB1>(v, (lane & 1) != 0, op);
    transpose_step<2, 0x4E>(v, (lane & 2) != 0, op);
    return v[0];
}

// rows: this lane's row value -> the reduction over the 8 pixel rows that share the lane's column
template <class Op>
__device__ __forceinline__ float reduce_rows_of_8(float r, Op op)
{
    r = op(r, dpp_get<0x128>(r));
    auto s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(r), __float_as_uint(r), false, false);
    r = op(__uint_as_float(s0[0]), __uint_as_float(s0[1]));
    auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(r), __float_as_uint(r), false, false);
    return op(__uint_as_float(s1[0]), __uint_as_float(s1[1]));
}

template <class Op>
__device__ __forceinline__ float reduce_row_of_8(float* v, int lane, Op op)
{
    return reduce_rows_of_8(reduce_columns_of_8(v, lane, op), op);
}

} // namespace c3dgs
