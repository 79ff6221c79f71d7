// common.hpp -- shared host/device helpers for libc3dgs_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/c3dgs_hip.h"

namespace c3dgs {

constexpr int TILE = 16;          // reference BLOCK_X = BLOCK_Y = 16 (cuda_rasterizer/config.h:16-17)
constexpr int TILE_PIX = 256;
constexpr int SPLAT_F4 = 3;       // float4 per splat record (48 B)
constexpr int PARTIAL_FLOATS = 9; // dcolor(3) dmean2D(2) dconic(3) dopacity(1) per (Gaussian,tile) instance
constexpr int BWD_LIST = 1024;    // Gaussians that share one list of blended ones = threads of a sum_partials_kernel workgroup

// ---------------------------------------------------------------- errors
void set_error(const std::string& msg);
inline int fail(int code, const std::string& msg) { set_error(msg); return code; }

#define C3DGS_HIP_TRY(expr)                                                                         \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return ::c3dgs::fail(C3DGS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));  \
    } while (0)

// after a kernel launch: always catch launch errors; with debug also synchronise (reference CHECK_CUDA,
// cuda_rasterizer/auxiliary.h:168-175)
#define C3DGS_STAGE(name, debug, stream)                                                            \
    do {                                                                                            \
        hipError_t e__ = hipGetLastError();                                                         \
        if (e__ == hipSuccess && (debug)) e__ = hipStreamSynchronize(stream);                       \
        if (e__ != hipSuccess)                                                                      \
            return ::c3dgs::fail(C3DGS_E_HIP, std::string("stage ") + name + ": " + hipGetErrorString(e__)); \
    } while (0)

// ---------------------------------------------------------------- order-preserving float <-> uint mapping
// atomicMin / atomicMax on the mapped words order the floats (bounding boxes of encode.hip and knn.hip)
__device__ __forceinline__ uint32_t f2ord(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __host__ __forceinline__ float ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---------------------------------------------------------------- depth-sort digit plan
// A depth key is the bit pattern of view-space z; preprocess culls z <= 0.01 unless `prefiltered`, and marks culled Gaussians with
// DEPTH_KEY_CULLED. Every visible key of a forward that is not prefiltered is therefore at least DEPTH_KEY_BIAS (the bits of
// 2^-7), and key - bias keeps the order of the keys. The sentinel keeps its value. Digits of the sort are taken from that biased
// key, least significant first: three 9-bit digits order every key below DEPTH_KEY_LIMIT3 (depths below 512; the largest 27-bit
// value is left to the sentinel's low digits, so no visible key ties with it), a fourth digit of 5 bits orders the rest.
// Not biased (prefiltered input: keys below the bias can occur): the raw key in four 8-bit digits.
constexpr uint32_t DEPTH_KEY_CULLED = 0xFFFFFFFFu, DEPTH_KEY_BIAS = 0x3C000000u;
constexpr int DEPTH_SORT3_BITS = 9;
constexpr uint32_t DEPTH_KEY_LIMIT3 = DEPTH_KEY_BIAS + (1u << (3 * DEPTH_SORT3_BITS)) - 1u;
__host__ __device__ __forceinline__ uint32_t depth_key_biased(uint32_t key) { return key == DEPTH_KEY_CULLED ? key : key - DEPTH_KEY_BIAS; }
struct DepthSortPlan { int passes; int bits[4]; uint32_t bias; };
// max_visible_key: the largest key that is not the sentinel (0 = none visible)
inline DepthSortPlan depth_sort_plan(bool biased, uint32_t max_visible_key)
{
    if (!biased) return { 4, { 8, 8, 8, 8 }, 0u };
    if (max_visible_key < DEPTH_KEY_LIMIT3) return { 3, { DEPTH_SORT3_BITS, DEPTH_SORT3_BITS, DEPTH_SORT3_BITS, 0 }, DEPTH_KEY_BIAS };
    return { 4, { DEPTH_SORT3_BITS, DEPTH_SORT3_BITS, DEPTH_SORT3_BITS, 32 - 3 * DEPTH_SORT3_BITS }, DEPTH_KEY_BIAS };
}
inline uint32_t depth_sort_digit(const DepthSortPlan& plan, uint32_t key, int pass)
{
    const uint32_t t = plan.bias ? depth_key_biased(key) : key;
    int shift = 0;
    for (int p = 0; p < pass; p++) shift += plan.bits[p];
    return (t >> shift) & ((1u << plan.bits[pass]) - 1u);
}

// ---------------------------------------------------------------- scratch layouts
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

size_t scan_temp_bytes(int P);      // max(scan, depth sort) temporary storage for P Gaussians
size_t sort_temp_bytes(int R, int end_bit, int key_bytes = 2);

inline int tiles_x(int W) { return (W + TILE - 1) / TILE; }
inline int tiles_y(int H) { return (H + TILE - 1) / TILE; }

// reference getHigherMsb, rasterizer_impl.cu:35-50
inline uint32_t higher_msb(uint32_t n)
{
    uint32_t msb = sizeof(n) * 4, step = msb;
    while (step > 1) {
        step /= 2;
        if (n >> msb) msb += step; else msb -= step;
    }
    if (n >> msb) msb++;
    return msb;
}

inline void geom_layout(int P, c3dgs_geom_layout* L)
{
    size_t o = 0, p = (size_t)(P > 0 ? P : 1);
    L->splat = o;             o = align_up(o + p * SPLAT_F4 * 16);
    L->depth_keys = o;        o = align_up(o + p * 4);
    L->depth_keys_sorted = o; o = align_up(o + p * 4);
    L->depth_order = o;       o = align_up(o + p * 4);
    L->sorted_offsets = o;    o = align_up(o + p * 8);
    L->inst_offset = o;       o = align_up(o + p * 4);
    L->rects = o;             o = align_up(o + p * 8);
    L->clamped = o;           o = align_up(o + p);
    L->block_base = o;        o = align_up(o + ((p + 255) / 256 + 2) * 4);   // + num_rendered + sort error word
    L->depth_base = o;        o = align_up(o + ((p + 255) / 256 + 1) * 4);
    L->scan_temp = o;         L->scan_temp_bytes = scan_temp_bytes((int)p);
    o = align_up(o + L->scan_temp_bytes);
    L->total_bytes = o;
}

// The indexed variant gathers a Gaussian's rotation (16 B) and scale (12 B) from two codebooks by the same random index:
// four gather instructions over up to 256 different cache lines per wave. Packed once per forward into ONE 32-byte row per
// codebook entry {rotation | scale, 0} (stored behind the P-sized part of the geometry buffer, so the backward finds it too),
// the same data arrives with two 16-byte loads from one line per Gaussian (preprocess 0.268 -> see DESIGN.md).
inline size_t geom_gtab_bytes(const c3dgs_raster_params& p) { return (p.g_indices && p.scales) ? align_up((size_t)(p.GS > 0 ? p.GS : 1) * 32) : 0; }

// Tile keys are 16-bit up to 65,536 tiles (4096 x 4096 pixels) and 32-bit above (e.g. 7680 x 4320 = 129,600 tiles): the
// reference's 64-bit keys (rasterizer_impl.cu:98-108) have no tile limit, and neither has this path; the common case keeps
// its 6-byte instances and two digit passes.
inline int tile_key_bytes_for(long long T) { return T > 65536 ? 4 : 2; }
inline int tile_key_bytes(int W, int H) { return tile_key_bytes_for((long long)tiles_x(W) * tiles_y(H)); }
// Bits the tile sort orders on: the reference's higher_msb(T) (rasterizer_impl.cu:298), clamped to the key width. They differ
// only at exactly 65,536 tiles (4096 x 4096 pixels): 17 bits, but every tile id < 2^16 fits the 16-bit key, and the 16-bit sort
// has no third digit pass. The scratch sizing (binning_layout) and the sort (forward_impl) both take it from here.
inline int tile_sort_end_bit_for(long long T)
{
    const int msb = (int)higher_msb((uint32_t)T), kbits = 8 * tile_key_bytes_for(T);
    return msb < kbits ? msb : kbits;
}
inline int tile_sort_end_bit(int W, int H) { return tile_sort_end_bit_for((long long)tiles_x(W) * tiles_y(H)); }

inline void binning_layout(int R, int W, int H, c3dgs_binning_layout* L)
{
    size_t o = 0, r = (size_t)(R > 0 ? R : 1);
    const int end_bit = tile_sort_end_bit(W, H);
    const size_t kb = (size_t)tile_key_bytes(W, H);
    L->keys_unsorted = o;   o = align_up(o + r * kb);
    L->values_unsorted = o; o = align_up(o + r * 4);
    L->keys_sorted = o;     o = align_up(o + r * kb);
    L->point_list = o;      o = align_up(o + r * 4);
    L->sort_temp = o;       L->sort_temp_bytes = sort_temp_bytes((int)r, end_bit, (int)kb);
    o = align_up(o + L->sort_temp_bytes);
    L->total_bytes = o;
}

// The whole image buffer: the public fields (c3dgs_image_layout) and, behind them and private to the library, the same two
// per-tile / per-pixel quantities in compact-list indices (below).
struct ImageLayout : c3dgs_image_layout { size_t tile_used_c, n_contrib_c; };
inline void image_layout(int W, int H, ImageLayout* L)
{
    size_t o = 0, n = (size_t)W * H, t = (size_t)tiles_x(W) * tiles_y(H);
    L->final_T = o;     o = align_up(o + n * 4);
    L->n_contrib = o;   o = align_up(o + n * 4);
    L->ranges = o;      o = align_up(o + t * 8);
    L->tile_used = o;   o = align_up(o + t * 4);
    L->tile_order = o;  o = align_up(o + t * 4);
    L->tile_used_c = o; o = align_up(o + t * 4);
    L->n_contrib_c = o; o = align_up(o + n * 4);
    L->total_bytes = o;
}

// Compact per-tile lists (render.hip): of a tile's visited list entries only those whose quadrant mask is non-zero ("live") can
// touch a pixel of the tile. The forward writes their Gaussian ids (cid) and masks (cqm) densely from the start of the tile's
// own segment [range.x, ...) of two arrays in the idle sort scratch, and per pixel / per tile the 1-based COMPACT index of the last
// contributor (ImageLayout: n_contrib_c, tile_used_c); the backward walks only those. Offsets are private to the library
// (tests: c3dgs_get_compact_layout); the public layout structs do not change.
struct CompactBinLayout { size_t cqm, cid, bin_bytes; };       // relative to sort_temp
inline CompactBinLayout compact_bin_layout(int R)
{
    const size_t r = (size_t)(R > 0 ? R : 1);
    CompactBinLayout C;
    C.cqm = 0; C.cid = align_up(r); C.bin_bytes = C.cid + align_up(r * 4);
    return C;
}

// Backward workspace: partial sums f32[R][9] | their 1-byte "written" flags | the lists of blended Gaussians, one per BWD_LIST
// Gaussians in id order and filled from the front: ids, where each one's nine sums are parked (slot), and the lists' lengths
inline void backward_layout(int P, int R, c3dgs_backward_layout* L)
{
    size_t o = 0, r = (size_t)(R > 0 ? R : 1), n_lists = ((size_t)(P > 0 ? P : 1) + BWD_LIST - 1) / BWD_LIST;
    L->partials = o;   o = align_up(o + r * PARTIAL_FLOATS * sizeof(float));
    L->touched = o;    o = align_up(o + r);
    L->live_ids = o;   o = align_up(o + n_lists * BWD_LIST * 4);
    L->live_slots = o; o = align_up(o + n_lists * BWD_LIST * 4);
    L->live_count = o; o = align_up(o + n_lists * 4);
    L->list_len = BWD_LIST;
    L->total_bytes = o;
}

// Workspace of a backward with depth / alpha map gradients (render_maps_backward.hip): the backward's layout above, unchanged and
// at the same offsets, and behind it the dL/dz plane, f32 [R], in the slot numbering of the partials. The plane is never cleared:
// an element means something only where the slot's "written" flag is set behind render_maps_backward_kernel.
struct DepthBackwardLayout { size_t dz, total_bytes; };
inline DepthBackwardLayout depth_backward_layout(int P, int R)
{
    c3dgs_backward_layout B; backward_layout(P, R, &B);
    const size_t r = (size_t)(R > 0 ? R : 1);
    DepthBackwardLayout L;
    L.dz = B.total_bytes;
    L.total_bytes = align_up(L.dz + r * sizeof(float));
    return L;
}

// Workspace of a backward with a gradient through the normal map (render_maps_backward.hip): depth_backward_layout's, unchanged and
// at the same offsets, and behind it the dn plane, three floats per slot in the same numbering: sum over the tile's pixels of
// w gN for the slot's (Gaussian, tile). Never cleared either: valid where the slot's flag is set behind the replay.
struct NormalSlot { float x, y, z; };
struct NormalBackwardLayout { size_t dz, dn, total_bytes; };
inline NormalBackwardLayout normal_backward_layout(int P, int R)
{
    const DepthBackwardLayout D = depth_backward_layout(P, R);
    const size_t r = (size_t)(R > 0 ? R : 1);
    NormalBackwardLayout L;
    L.dz = D.dz; L.dn = D.total_bytes;
    L.total_bytes = align_up(L.dn + r * sizeof(NormalSlot));
    return L;
}

// s = f(z) of the distortion passes (render_distortion.hip, render_maps_backward.hip). ndc == 0: raw, f(z) = z. Otherwise
// f(z) = far / (far - near) * (1 - near / z) = c0 - c1 / z, c0 and c1 rounded from double (raw: c0 = 0), on the correctly rounded
// rz = 1 / z. The map and its gradient only see differences of s, and a sum of w s of the size of s cannot carry them in fp32
// where a ray's spread is small (ndc: s near 1, spreads of 0.01). So no pass forms s itself per entry: rel() is s - c0, which the
// forward sums about the pixel's first entry, and about() is s - p for a pivot p, given q = c0 - p, in ONE rounding at the size
// of the difference. f'(z) = c1 rz^2. The backward's workspace is depth_backward_layout's.
struct DistortionMap {
    float c0, c1;
    int ndc;
    __device__ __forceinline__ float rz(float z) const { return (ndc && z > 0.f) ? 1.0f / z : 0.f; }
    __device__ __forceinline__ float rel(float z, float rz_) const { return ndc ? -c1 * rz_ : z; }
    __device__ __forceinline__ float about(float z, float rz_, float q) const { return ndc ? fmaf(-c1, rz_, q) : z + q; }
    __device__ __forceinline__ float ds(float rz_) const { return ndc ? (c1 * rz_) * rz_ : 1.0f; }
};
inline DistortionMap distortion_map(float near_, float far_)          // far <= 0: raw
{
    DistortionMap f = { 0.f, 0.f, 0 };
    if (far_ > 0.f) {
        const double c0 = (double)far_ / ((double)far_ - (double)near_);
        f.c0 = (float)c0; f.c1 = (float)(c0 * (double)near_); f.ndc = 1;
    }
    return f;
}

// Blend-statistics workspace (render_contrib.hip): one {sum, max, hits} record per backward slot, f32 f32 u32 [R] | their
// 1-byte "written" flags. Same slot numbering as the backward's partials; only the flags are cleared per call.
struct ContribSlot { float sum, max; uint32_t hits; };
struct ContribLayout { size_t slots, touched, touched_bytes, total_bytes; };
inline ContribLayout contrib_layout(int P, int R)
{
    (void)P;
    size_t o = 0, r = (size_t)(R > 0 ? R : 1);
    ContribLayout L;
    L.slots = o;   o = align_up(o + r * sizeof(ContribSlot));
    L.touched = o; o = align_up(o + r);
    L.touched_bytes = o - L.touched;
    L.total_bytes = o;
    return L;
}

// Error-score workspace (render_error.hip): one float per backward slot, f32 [R] | their 1-byte "written" flags. Same slot
// numbering as the backward's partials; only the flags are cleared per call.
struct ErrorLayout { size_t slots, touched, touched_bytes, total_bytes; };
inline ErrorLayout error_layout(int P, int R)
{
    (void)P;
    size_t o = 0, r = (size_t)(R > 0 ? R : 1);
    ErrorLayout L;
    L.slots = o;   o = align_up(o + r * sizeof(float));
    L.touched = o; o = align_up(o + r);
    L.touched_bytes = o - L.touched;
    L.total_bytes = o;
    return L;
}

// Sparse-Adam workspace (sparse_adam.hip), caller-owned: count u32 (the number of listed rows) at offset 0 | rows u32[P], the
// ascending ids of the listed rows, filled from the front | the exclusive scan of the listed rows per SPARSE_ADAM_SELECT_ROWS
// rows, u32[ceil(P / 256) + 2] (scan_blocks.hpp's base[]: its last-but-one word is the total). Every region 256-byte aligned.
constexpr int SPARSE_ADAM_SELECT_ROWS = 256;
struct SparseAdamLayout { size_t count, rows, block_base, total_bytes; };
inline SparseAdamLayout sparse_adam_layout(int64_t P)
{
    const size_t p = (size_t)(P > 0 ? P : 1);
    SparseAdamLayout L;
    size_t o = 0;
    L.count = o;      o = align_up(o + 4);
    L.rows = o;       o = align_up(o + p * 4);
    L.block_base = o; o = align_up(o + ((p + SPARSE_ADAM_SELECT_ROWS - 1) / SPARSE_ADAM_SELECT_ROWS + 2) * 4);
    L.total_bytes = o;
    return L;
}

// ---------------------------------------------------------------- kernel launchers (one per .hip file)
struct GeomPtrs {
    float4* splat; uint32_t* depth_keys; uint32_t* depth_keys_sorted;
    uint32_t* depth_order; uint2* sorted_offsets; uint32_t* inst_offset; uint16_t* rects;
    uint8_t* clamped; uint32_t* block_base; uint32_t* depth_base; void* scan_temp; size_t scan_temp_bytes;
    float4* gtab;     // indexed variant: the scale / rotation codebooks packed as one 32-byte row per entry (behind the P-sized part)
};
struct BinPtrs {
    void* keys_unsorted; uint32_t* values_unsorted; void* keys_sorted; uint32_t* point_list;   // keys: u16, or u32 above 65,536 tiles
    void* sort_temp; size_t sort_temp_bytes; int key_bytes;
};
struct ImgPtrs { float* final_T; uint32_t* n_contrib; uint2* ranges; uint32_t* tile_used; uint32_t* tile_order;
                 uint32_t* tile_used_c; uint32_t* n_contrib_c; };
struct CompactPtrs { uint8_t* cqm; uint32_t* cid; };   // inside BinPtrs::sort_temp, valid once the tile sort has run
struct BwdPtrs { float* partials; uint8_t* touched; size_t touched_bytes;   // the flags' whole region: what a call clears
                 uint32_t* live_ids; uint32_t* live_slots; uint32_t* live_count; };
struct ContribPtrs { ContribSlot* slots; uint8_t* touched; size_t touched_bytes; };
struct ErrorPtrs { float* slots; uint8_t* touched; size_t touched_bytes; };

inline GeomPtrs geom_ptrs(void* base, int P)
{
    c3dgs_geom_layout L; geom_layout(P, &L);
    char* b = (char*)base;
    return { (float4*)(b + L.splat), (uint32_t*)(b + L.depth_keys), (uint32_t*)(b + L.depth_keys_sorted), (uint32_t*)(b + L.depth_order),
             (uint2*)(b + L.sorted_offsets), (uint32_t*)(b + L.inst_offset), (uint16_t*)(b + L.rects),
             (uint8_t*)(b + L.clamped), (uint32_t*)(b + L.block_base), (uint32_t*)(b + L.depth_base), (void*)(b + L.scan_temp),
             L.scan_temp_bytes, (float4*)(b + L.total_bytes) };
}
inline BinPtrs bin_ptrs(void* base, int R, int W, int H)
{
    c3dgs_binning_layout L; binning_layout(R, W, H, &L);
    char* b = (char*)base;
    return { (void*)(b + L.keys_unsorted), (uint32_t*)(b + L.values_unsorted), (void*)(b + L.keys_sorted),
             (uint32_t*)(b + L.point_list), (void*)(b + L.sort_temp), L.sort_temp_bytes, tile_key_bytes(W, H) };
}
inline ImgPtrs img_ptrs(void* base, int W, int H)
{
    ImageLayout L; image_layout(W, H, &L);
    char* b = (char*)base;
    return { (float*)(b + L.final_T), (uint32_t*)(b + L.n_contrib), (uint2*)(b + L.ranges), (uint32_t*)(b + L.tile_used),
             (uint32_t*)(b + L.tile_order), (uint32_t*)(b + L.tile_used_c), (uint32_t*)(b + L.n_contrib_c) };
}
inline CompactPtrs compact_ptrs(const BinPtrs& bp, int R)
{
    const CompactBinLayout C = compact_bin_layout(R);
    return { (uint8_t*)bp.sort_temp + C.cqm, (uint32_t*)((char*)bp.sort_temp + C.cid) };
}
inline BwdPtrs bwd_ptrs(void* base, int P, int R)
{
    c3dgs_backward_layout L; backward_layout(P, R, &L);
    char* b = (char*)base;
    return { (float*)(b + L.partials), (uint8_t*)(b + L.touched), L.live_ids - L.touched,
             (uint32_t*)(b + L.live_ids), (uint32_t*)(b + L.live_slots), (uint32_t*)(b + L.live_count) };
}

inline ContribPtrs contrib_ptrs(void* base, int P, int R)
{
    const ContribLayout L = contrib_layout(P, R);
    char* b = (char*)base;
    return { (ContribSlot*)(b + L.slots), (uint8_t*)(b + L.touched), L.touched_bytes };
}

inline ErrorPtrs error_ptrs(void* base, int P, int R)
{
    const ErrorLayout L = error_layout(P, R);
    char* b = (char*)base;
    return { (float*)(b + L.slots), (uint8_t*)(b + L.touched), L.touched_bytes };
}

// preprocess.hip
void launch_camera_from_pose(const float* pose, float inv_tan_x, float inv_tan_y, float* view, float* proj, float* campos, hipStream_t s);
void launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t s);
void launch_mark_visible_pose(int P, const float* means3D, const float* pose7, uint8_t* present, hipStream_t s);
void launch_pack_codebook(const c3dgs_raster_params& p, float4* gtab, hipStream_t s);
// zero_span / zero_n16: 16-byte words every workgroup clears a slice of before anything else (the depth sort's control words).
// Leaves the workgroup totals in g.block_base: the caller runs the scan behind it (launch_scan_blocks / run_depth_hist_scan)
void launch_preprocess(const c3dgs_raster_params& p, const GeomPtrs& g, int32_t* radii, uint2* ranges, void* zero_span, size_t zero_n16,
                       hipStream_t s);
// exclusive scan of nb workgroup totals in place, base[nb] = total; sort_err: the sticky sort time-out word, copied to base[nb + 1];
// host_out / host_seq: mapped host words {num_rendered, sort error flag, host_seq} the scan writes last (or null)
void launch_scan_blocks(int nb, uint32_t* base, const uint32_t* sort_err, uint32_t* host_out, uint32_t host_seq, hipStream_t s);
void launch_depth_order_scan(int P, const GeomPtrs& g, hipStream_t s);   // block totals of tiles_sorted -> depth_base[]
void launch_duplicate_with_keys(int P, const GeomPtrs& g, const BinPtrs& b, int grid_x, const uint32_t* sort_err,
                                void* zero_span, size_t zero_n16, hipStream_t s);   // zero span: the tile sort's control words
void launch_identify_ranges(int R, const void* keys_sorted, int key_bytes, uint2* ranges, const uint32_t* sort_err, hipStream_t s);
// binning.hip
// ctrl_cleared: the first *_sort_clear_bytes(...) bytes of `temp` were zeroed by an earlier kernel on the same stream
// (0 bytes = this configuration's sort clears its own control words: pass false)
// rects_fit_bytes: all rectangle coordinates < 256 (at most 255 x 255 tiles): the rectangles may ride through the sort packed
// hist_done: run_depth_hist_scan has run on this scratch (only with ctrl_cleared)
hipError_t run_depth_sort(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin,
                          uint32_t* vout, int P, const uint2* rects, uint2* rects_sorted, hipStream_t s, bool ctrl_cleared = false,
                          bool rects_fit_bytes = false, bool hist_done = false);
// launch_scan_blocks and the depth sort's digit histograms in one launch. Only where depth_sort_clear_bytes(P) is not 0 (the
// hand-written sort) and those bytes of `temp` have been cleared by an earlier kernel on the stream
hipError_t run_depth_hist_scan(void* temp, size_t temp_bytes, const uint32_t* keys, int P, int nb, uint32_t* base,
                               const uint32_t* sort_err, uint32_t* host_out, uint32_t host_seq, hipStream_t s);
hipError_t run_tile_sort(void* temp, size_t temp_bytes, const void* kin, void* kout, int key_bytes, const uint32_t* vin,
                         uint32_t* vout, int R, int end_bit, hipStream_t s, bool ctrl_cleared = false);
size_t depth_sort_clear_bytes(int P);
// may this forward's depth sort take the biased three-pass plan (onesweep_depth3_* below)? The caller adds what only it knows:
// not prefiltered, control words cleared, a mapped host pad to read the largest visible key from
bool depth_sort3_available(int P, size_t temp_bytes, bool rects_fit_bytes);
size_t tile_sort_clear_bytes(int R, int end_bit, int key_bytes);
// radix_sort.hip (hand-written onesweep; C3DGS_SORT_ROCPRIM=1 selects the rocPRIM path of binning.hip instead)
bool onesweep_enabled();
int onesweep_timed_out(hipStream_t s);   // debug mode only (synchronises): reads + clears the sticky error word
uint32_t* onesweep_error_word();          // device address of the sticky look-back time-out word (0 = fine)
size_t onesweep_depth_temp_bytes(int P);
size_t onesweep_tile_temp_bytes(int R, int end_bit, int key_bytes = 2);
size_t onesweep_depth_clear_bytes(int P);
size_t onesweep_tile_clear_bytes(int R, int end_bit, int key_bytes);
hipError_t onesweep_depth_sort(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout,
                               int P, const uint2* gather_src, uint2* gather_dst, hipStream_t s, bool ctrl_cleared = false,
                               bool rects_fit_bytes = false, bool hist_done = false);
hipError_t onesweep_depth_hist_scan(void* temp, size_t temp_bytes, const uint32_t* keys, int P, int nb, uint32_t* base,
                                    const uint32_t* sort_err, uint32_t* host_out, uint32_t host_seq, hipStream_t s);
// the depth sort on biased keys (depth_sort_plan above), in two halves around the forward's host read: histogram (+ id-order scan,
// + the largest visible key to the two mapped host words at `host_max`: {key, host_seq}), passes 1-2, then -- once the host knows
// the largest visible key -- the last pass or two. Needs the packed-rectangle payload (grids up to 255 x 255 tiles) and the first
// onesweep_depth_clear_bytes(P) bytes of `temp` cleared by an earlier kernel on the stream.
hipError_t onesweep_depth3_hist_scan(void* temp, size_t temp_bytes, const uint32_t* keys, int P, int nb, uint32_t* base,
                                     const uint32_t* sort_err, uint32_t* host_out, uint32_t host_seq, uint32_t* host_max, hipStream_t s);
const uint32_t* onesweep_depth3_max_word(void* temp, int P);   // device word that holds the largest visible key behind that launch
hipError_t onesweep_depth3_head(void* temp, size_t temp_bytes, const uint32_t* kin, int P, const uint2* rects, hipStream_t s);
hipError_t onesweep_depth3_tail(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, uint32_t* vout, int P,
                                const uint2* rects, uint2* rects_sorted, uint32_t max_visible_key, hipStream_t s);
hipError_t onesweep_tile_sort32(void* temp, size_t temp_bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout,
                                int R, int end_bit, hipStream_t s, bool ctrl_cleared = false);   // 32-bit tile keys (more than 65,536 tiles)
hipError_t onesweep_tile_sort(void* temp, size_t temp_bytes, const uint16_t* kin, uint16_t* kout, const uint32_t* vin, uint32_t* vout,
                              int R, int end_bit, hipStream_t s, bool ctrl_cleared = false);
// render.hip
void launch_render_forward(int W, int H, const ImgPtrs& img, const uint32_t* point_list, const float4* splat,
                           const float* bg, float* out_color, const CompactPtrs& cl, const uint32_t* sort_err, hipStream_t s);
void launch_backward_prep(int W, int H, const ImgPtrs& img, void* zero_a, size_t n16_a, void* zero_b, size_t n16_b, hipStream_t s);
void launch_render_backward(int W, int H, const ImgPtrs& img, const float4* splat,
                            const uint32_t* block_base, const float* bg, const float* dL_dpix, float* partials,
                            uint8_t* touched, const CompactPtrs& cl, void* zero_span, size_t zero_n16, hipStream_t s);
// render_depth.hip (forward-only replay of the blend: depth / accumulated opacity / median depth; null outputs are skipped)
void launch_render_depth(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const uint32_t* depth_keys,
                         float* out_depth, float* out_alpha, float* out_median, const uint32_t* sort_err, hipStream_t s);
// render_maps_backward.hip (gradients through the depth, alpha, distortion and normal maps in ONE blend replay; dL_ddepth /
// dL_dalpha may be null = zeros; dL_ddistortion not null: with the distortion map, moment is required; dL_dnormal not null: with
// the normal map, normals and dn_plane are required): the blend replay that adds its six moments into the backward's partial-sum
// slots (behind render_backward or the flag clear, in front of launch_backward_preprocess) and writes the dL/dz plane and, with
// the normal map, the dn plane; and the fold of the dL/dz plane into dL_dmeans3D behind launch_backward_preprocess (it walks
// that launch's lists of blended Gaussians).
void launch_render_maps_backward(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const BwdPtrs& w,
                                 float* dz_plane, NormalSlot* dn_plane, const float* normals, const float* dL_ddepth,
                                 const float* dL_dalpha, const float* dL_dnormal, const float* dL_ddistortion, const float* moment,
                                 const DistortionMap& f, const uint32_t* sort_err, hipStream_t s);
void launch_depth_backward_fold(int P, const GeomPtrs& g, const BwdPtrs& w, const float* dz_plane, const float* view,
                                float* dL_dmeans3D, const uint32_t* sort_err, hipStream_t s);
// render_distortion.hip (forward-only replay of the blend: the distortion map and the first moment sum w s; out_moment may be null)
void launch_render_distortion(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const uint32_t* depth_keys,
                              const DistortionMap& f, float* out_distortion, float* out_moment, const uint32_t* sort_err, hipStream_t s);
// normals.hip: the per-Gaussian normals [P, 4] = {n_x, n_y, n_z, sigma (m + 1)} (g_indices null: the rows are the Gaussians' own),
// the fold of the dn plane into dL_drotations behind launch_backward_preprocess (beside launch_depth_backward_fold), and the
// depth -> normal stencil with its gather backward
void launch_gaussian_normals(int P, const float* means3D, const float* scales, const float* rotations, const int64_t* g_indices,
                             const float* view, float* out, hipStream_t s);
void launch_normal_backward_fold(int P, const GeomPtrs& g, const BwdPtrs& w, const NormalSlot* dn_plane, const float* normals,
                                 const float* rotations, const int64_t* g_indices, const float* view, float* dL_drotations,
                                 const uint32_t* sort_err, hipStream_t s);
void launch_depth_to_normal(int W, int H, const float* z, float tan_fovx, float tan_fovy, float* out, hipStream_t s);
void launch_depth_to_normal_backward(int W, int H, const float* z, const float* dL_dnormal, float tan_fovx, float tan_fovy,
                                     float* dL_dz, hipStream_t s);
// render_normal.hip (forward-only replay of the blend: the normal map [3, H, W] = sum w n)
void launch_render_normal(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const float4* splat, const float* normals,
                          float* out_normal, const uint32_t* sort_err, hipStream_t s);
// render_contrib.hip (forward-only replay of the blend: per-Gaussian sum / max of alpha T and blended-pair count; null outputs are
// skipped): the blend replay into the slots (the caller has cleared w.touched on the stream), the per-Gaussian fold of the slots,
// and the fold of one view's rows into model-sized accumulators.
void launch_render_contrib(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const ContribPtrs& w,
                           const uint32_t* sort_err, hipStream_t s);
void launch_contrib_sum(int P, const GeomPtrs& g, const ContribPtrs& w, float* out_sum, float* out_max, uint32_t* out_hits,
                        const uint32_t* sort_err, hipStream_t s);
void launch_contrib_accumulate(int P_model, int P_rows, const uint8_t* visible, const int32_t* rank, const float* weight_sum,
                               const float* weight_max, const uint32_t* hits, float* acc_sum, float* acc_max, int64_t* acc_hits,
                               uint32_t* acc_views, hipStream_t s);
// render_error.hip (forward-only replay of the blend: per-Gaussian sum of alpha T x a per-pixel map): the blend replay into the
// slots (the caller has cleared w.touched on the stream), the per-Gaussian fold of the slots, the fold of one view's row into
// model-sized accumulators, and the mean-absolute-difference map of two planar images.
void launch_render_error(int W, int H, const ImgPtrs& img, const CompactPtrs& cl, const GeomPtrs& g, const ErrorPtrs& w,
                         const float* pixel_map, const uint32_t* sort_err, hipStream_t s);
void launch_error_sum(int P, const GeomPtrs& g, const ErrorPtrs& w, float* out_sum, const uint32_t* sort_err, hipStream_t s);
void launch_error_accumulate(int P_model, int P_rows, const uint8_t* visible, const int32_t* rank, const float* err_sum,
                             float* acc_max, float* acc_sum, hipStream_t s);
void launch_error_map_l1(int C, int H, int W, const float* img, const float* gt, float* out, hipStream_t s);
// pose_grad.hip (exact gradient with respect to the camera's 7-element pose, behind a finished backward): the 24 per-workgroup
// sums into `rows` (pose_grad_workspace_bytes(P) bytes), then their fold and the pose-dependent epilogue into out[7]. P > 0.
struct PoseGradIn {
    int P, D, M; float scale_modifier;
    const float* means3D; const float* dL_dmeans3D; const float* dL_dcov3D; const float* dL_dcolors;
    const float* sh; const int64_t* sh_indices;
    const float* cov3D_precomp; const float* scales; const float* rotations; const float* scale_factors; const int64_t* g_indices;
    const uint8_t* clamped; const int32_t* radii; const float* pose;
};
size_t pose_grad_workspace_bytes(int P);
void launch_pose_sums(const PoseGradIn& in, float* rows, hipStream_t s);
void launch_pose_fold(int P, const float* rows, const float* pose, float* out, hipStream_t s);
// aa_opacity.hip (antialiased rasterization: o' = o rho in front of the forward, the chain through rho behind the backward)
void launch_aa_opacity(const c3dgs_raster_params& p, float* opacity_out, float* rho, hipStream_t s);
void launch_aa_opacity_backward(const c3dgs_raster_params& p, const int32_t* radii, const c3dgs_raster_grads& gr, hipStream_t s);
// filter3d.hip (the 3D smoothing filter: per-Gaussian minimum size over a camera table, applied around the rasterizer)
void launch_filter3d_dist(int P, int C, const float* xyz, const float* cams, float* filter, uint32_t* ws, hipStream_t s);
void launch_filter3d_finish(int P, const uint32_t* ws, float* filter, uint8_t* seen, hipStream_t s);
void launch_filter3d_apply(const c3dgs_filter3d_rows& p, float* cov3D_out, float* opacity_out, hipStream_t s);
void launch_filter3d_apply_backward(const c3dgs_filter3d_rows& p, const c3dgs_filter3d_grads& g, hipStream_t s);
// mesh.hip (mesh extraction: TSDF fusion of depth maps into a dense volume, welded marching tetrahedra over it)
void launch_tsdf_integrate(const c3dgs_lattice& l, int K, int W, int H, const float* depth, const float* color, const float* cams,
                           float sdf_trunc, float depth_min, float depth_max, float* tsdf, float* weight, float* vol_color,
                           hipStream_t s);
size_t mesh_extract_workspace_bytes(int Nx, int Ny, int Nz);
void launch_mesh_classify(const c3dgs_lattice& l, const float* tsdf, const float* weight, void* ws, hipStream_t s);
const uint32_t* launch_mesh_scan(const c3dgs_lattice& l, void* ws, hipStream_t s);     // -> the device words {vertices, faces}
void launch_mesh_vertices(const c3dgs_lattice& l, const float* tsdf, const float* vol_color, void* ws, uint32_t V, float* vertices,
                          float* colors, hipStream_t s);
void launch_mesh_faces(const c3dgs_lattice& l, const float* tsdf, void* ws, uint32_t F, int32_t* faces, hipStream_t s);
// backward_preprocess.hip
void launch_backward_preprocess(const c3dgs_raster_params& p, const int32_t* radii, const GeomPtrs& g, const BwdPtrs& w,
                                const c3dgs_raster_grads& gr, hipStream_t s);
// vq.hip
int launch_weighted_distance(int64_t N, int C, int K, const float* coefs, const int64_t* gather, const float* codebook,
                             float* out_dist, int64_t* out_idx, hipStream_t s, void* ws = nullptr, size_t ws_bytes = 0, int presplit = -1);
bool wd_presplit_supported(int C, int K, const float* coefs, const float* codebook, const void* ws, size_t ws_bytes);
int launch_vq_apply_split(int K, int D, float* S, float* codebook, float* entry_importance, float decay, float alpha, float eps,
                          int scale_normalize, void* ws, size_t ws_bytes, int parity, hipStream_t s);
void launch_vq_seed_words(int K, int D, void* ws, hipStream_t s);
uint32_t* vq_next_absmax_word(int K, int D, void* ws, int parity);
size_t wd_ws_bytes(int64_t N, int C, int K);
int launch_wd_debug_scores(int64_t N, int C, int K, const float* coefs, const float* codebook, float* scores, void* ws, size_t ws_bytes,
                           float* out_dist, int64_t* out_idx, hipStream_t s);
void launch_vq_accumulate(int64_t B, int K, int D, const float* x, const float* w, const int64_t* gather,
                          const int64_t* idx, const float* dist, float* S, double* dist_sum, hipStream_t s, uint32_t* clear_word = nullptr);
void launch_vq_apply(int K, int D, const float* S, float* codebook, float* entry_importance, float decay, float alpha,
                     float eps, int scale_normalize, hipStream_t s);

// encode.hip
size_t morton_workspace_bytes(int P);
int run_morton_order(int P, const float* xyz, int64_t* codes_out, int64_t* order_out, void* workspace, hipStream_t s);
void launch_extract_rot_scale(int n, const float* cov6, float* rot, float* scale, hipStream_t s);
// knn.hip (3-nearest-neighbour mean squared distance): sort, then bounds, then query, on one workspace
size_t knn_workspace_bytes(int P);
int run_knn_sort(int P, const float* xyz, void* workspace, hipStream_t s);
void launch_knn_bounds(int P, void* workspace, hipStream_t s);
void launch_knn_query(int P, const void* workspace, float* out, hipStream_t s);
void launch_knn_query_neighbours(int P, const void* workspace, int32_t* idx, float* d2, hipStream_t s);
// nn_query.hip (nearest neighbour of external queries in the tree run_knn_sort + launch_knn_bounds left in `index`)
size_t nn_query_workspace_bytes(int Q);
int run_nn_query_sort(int P, const void* index, int Q, const float* queries, void* workspace, hipStream_t s);
void launch_nn_query(int P, const void* index, int Q, const float* queries, bool sorted, const void* workspace, int32_t* idx, float* d2,
                     uint32_t* leaves, hipStream_t s);
// mesh_sample.hip (surface sampling): clear, count, scan -> the device words {total low, total high, flags}; then emit
size_t mesh_sample_workspace_bytes(int F);
hipError_t mesh_sample_clear(int F, void* ws, hipStream_t s);
void launch_mesh_sample_count(int V, const float* vertices, int F, const int32_t* faces, float density, uint32_t seed, void* ws,
                              hipStream_t s);
const uint32_t* launch_mesh_sample_scan(int F, void* ws, hipStream_t s);
void launch_mesh_sample_emit(int V, const float* vertices, int F, const int32_t* faces, uint32_t seed, const void* ws, uint32_t S,
                             float* points, int32_t* face, hipStream_t s);
// geometry_metrics.hip (count, sum of distances and counts below thresholds of one direction)
size_t geometry_reduce_workspace_bytes(int64_t N);
void launch_geometry_reduce(int64_t N, const float* d2, const float* points, const float* bounds, float max_dist, int T,
                            const float* thresholds, void* workspace, double* out, hipStream_t s);
// ray_fill.hip (initial densification): top-2 -> counts -> scan -> emit -> per-slot level sort; then the positions.
// A request the workspace cannot serve comes back in `problem` (hipSuccess, nothing written).
size_t ray_fill_plan_workspace_bytes(int P, long long rows);
hipError_t run_ray_fill_plan(int P, const float* d2, float step, long long capacity, int32_t* src, uint8_t* slot, int32_t* level,
                             int32_t* totals, void* workspace, size_t workspace_bytes, hipStream_t s, std::string* problem);
void launch_ray_fill_xyz(int P, const float* xyz, const int32_t* idx, const float* d2, float step, long long n_new,
                         const int32_t* src, const uint8_t* slot, const int32_t* level, float* out, hipStream_t s);
// image_io.hip
void launch_image_from_u8(int Hs, int Ws, int C, const uint8_t* src, int flip, const float* bg, int Hd, int Wd, float* out,
                          hipStream_t s);
// adam.hip
void launch_adam(int n_tensors, const c3dgs_adam_tensor* tensors, double beta1, double beta2, double eps, hipStream_t s);
void launch_abs_accumulate(int64_t n, const float* g, float* acc, hipStream_t s);
// sparse_adam.hip: the list of the rows a mask names (mask_kind 0: u8 != 0, 1: i32 > 0) into the workspace, and the Adam step
// over the listed rows of up to C3DGS_ADAM_MAX_TENSORS tensors. 0 < P < 2^31.
void launch_sparse_adam_select(int64_t P, const void* mask, int mask_kind, void* workspace, hipStream_t s);
void launch_sparse_adam_step(int n_tensors, const c3dgs_sparse_adam_tensor* tensors, int64_t P, const void* workspace, double beta1,
                             double beta2, double eps, hipStream_t s);
// densify.hip (adaptive density control): classify -> plan (scan + emit) -> apply, and the per-iteration stats
void launch_densify_classify(int P, const float* accum, const float* denom, const float* scale_clone, const float* scale_split,
                             const float* scale_prune_self, const float* scale_prune_child, const float* opacity, float max_grad,
                             float dense_extent, float min_opacity, float big_extent, uint8_t* code, hipStream_t s);
size_t rows_plan_workspace_bytes(int P);
hipError_t run_rows_plan(int P, const uint8_t* code, int N, long long capacity, int32_t* src, uint8_t* kind, int32_t* draw_row,
                         int32_t* totals, void* workspace, hipStream_t s);
void launch_rows_apply(int P, long long P_new, const int32_t* src, const uint8_t* kind, const int32_t* draw_row, int n_tensors,
                       const c3dgs_rows_tensor* tensors, int N, long long n_draws, const float* rotation_raw, const float* std,
                       const float* z, int log_scaling, int half_xyz, hipStream_t s);
void launch_densify_stats(int P, const float* grad, const uint8_t* filter, const int32_t* radii, float* accum, float* denom,
                          float* max_radii, hipStream_t s);
// index_plan.hip (prune / codebook compaction of an indexed model): flags -> scans -> emit
size_t index_plan_workspace_bytes(int P, int K0, int K1);
hipError_t run_index_plan(int P, const uint8_t* keep, const int64_t* idx0, int K0, const int64_t* idx1, int K1, long long cap_rows,
                          long long cap_cb0, long long cap_cb1, int32_t* src, int64_t* new_idx0, int64_t* new_idx1, int32_t* cb_src0,
                          int32_t* cb_src1, int32_t* totals, void* workspace, hipStream_t s);
// loss.hip
void launch_l1_ssim_value(const double* sums, double l1_scale, double ssim_scale, double constant, float* out, hipStream_t s);
void launch_l1_ssim_forward(int C, int H, int W, const float* img, const float* gt, float* Dmu, float* Ds1, float* Ds12,
                            double* sums, hipStream_t s);
void launch_l1_ssim_backward(int C, int H, int W, const float* img, const float* gt, const float* Dmu, const float* Ds1,
                             const float* Ds12, const float* grad_loss, float l1_coeff, float ssim_coeff, float* dL_dimg,
                             hipStream_t s);
// metrics.hip: one launch of the tile kernel is at most 2^24 - 1 workgroups (2^32 work-items of 256 threads)
constexpr int64_t IMAGE_METRICS_MAX_WORKGROUPS = (int64_t(1) << 24) - 1;
int64_t image_metrics_workgroups(int N, int C, int H, int W);
size_t image_metrics_ws_bytes(int N, int C, int H, int W);
void launch_image_metrics(int N, int C, int H, int W, const float* img, const float* gt, double* partials, double* out,
                          hipStream_t s);

// qat.hip
size_t qat_workspace_bytes();
size_t qat_scan_bytes(int P);
void launch_qat_observe(const c3dgs_qat_params& q, void* workspace, hipStream_t s);
void launch_qat_codebooks(const c3dgs_qat_params& q, float* scales_n, float* rotations, float* shs, hipStream_t s);
void launch_qat_codebooks_backward(const c3dgs_qat_params& q, const float* g_scales, const float* g_rot, const float* g_shs,
                                   float* d_scaling, float* d_rotation, float* d_dc, float* d_rest, hipStream_t s);
hipError_t run_qat_visible(const c3dgs_qat_params& q, const float* view, uint8_t* visible, int32_t* rank, int32_t* count,
                           void* scan_ws, hipStream_t s);
void launch_qat_points(const c3dgs_qat_params& q, const uint8_t* visible, const int32_t* rank, const int64_t* sh_idx,
                       const int64_t* g_idx, float* means3D, float* opac, float* sfac, int64_t* sh_out, int64_t* g_out,
                       hipStream_t s);
void launch_qat_points_backward(const c3dgs_qat_params& q, const uint8_t* visible, const int32_t* rank, const float* g_m3,
                                const float* g_m2, const float* g_op, const float* g_sf, float* d_xyz, float* d_screen,
                                float* d_op, float* d_sf, hipStream_t s);
void launch_qat_quantize(const c3dgs_qat_params& q, int scaling_exp, int8_t* opacity, int8_t* scaling, int8_t* scaling_factor,
                         int8_t* rotation, int8_t* features_dc, int8_t* features_rest, hipStream_t s);
void launch_fake_quantize(long long n, const float* x, c3dgs_fq_state* state, int observe, int enabled, float c, float* out,
                          void* workspace, hipStream_t s);
void launch_fake_quantize_backward(long long n, const float* x, const c3dgs_fq_state* state, int enabled, const float* g,
                                   float* dx, hipStream_t s);

} // namespace c3dgs
