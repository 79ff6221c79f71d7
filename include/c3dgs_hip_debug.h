/*
 * c3dgs_hip_debug.h -- entry points of libc3dgs_hip.so that are NOT part of its public ABI (include/c3dgs_hip.h): no caller
 * of the library needs them, and they may change without a new C3DGS_ABI_VERSION. Conventions as in c3dgs_hip.h.
 */
#ifndef C3DGS_HIP_DEBUG_H
#define C3DGS_HIP_DEBUG_H

#include "c3dgs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ================= test hooks into product code: exported by the product library (csrc/c_abi_debug.hip) =================
 * The GPU tests drive the product's own sorts and codeword search through these. */

/* tests only: the binning stage's stable LSD radix sort (radix_sort.hip) on caller-provided pairs. key_bytes = 2 (tile
 * keys) or 4 (depth keys); bits [0, end_bit) are sorted; ties keep input order. temp >= c3dgs_debug_sort_temp_bytes(). */
size_t c3dgs_debug_sort_temp_bytes(int32_t key_bytes, int64_t n, int32_t end_bit);
int c3dgs_debug_sort_pairs(int32_t key_bytes, int64_t n, int32_t end_bit, const void* keys_in, void* keys_out,
                           const uint32_t* values_in, uint32_t* values_out, void* temp, size_t temp_bytes, void* stream);

/* tests only: the forward's tile-key sort for a grid of `tiles` tiles (1 .. 256 x 65535), taking the forward's own route: keys
 * are uint16 up to 65,536 tiles and uint32 above, sorted on min(higher_msb(tiles), key bits) bits, through the same dispatch
 * (hand-written sort, or rocPRIM with C3DGS_SORT_ROCPRIM=1). Ties keep input order. temp >= c3dgs_debug_tile_sort_temp_bytes(),
 * which is the forward's own sizing of that scratch (0 = bad arguments, see c3dgs_last_error). */
size_t c3dgs_debug_tile_sort_temp_bytes(int32_t tiles, int64_t n);
int c3dgs_debug_tile_sort_pairs(int32_t tiles, int64_t n, const void* keys_in, void* keys_out, const uint32_t* values_in,
                                uint32_t* values_out, void* temp, size_t temp_bytes, void* stream);

/* diagnostics for tests: scores[n * C + c] = ||c||^2 - 2 x_n.c as the split-fp16 search forms them (fp32 accumulation of the three fp16 piece products,
 * divided back by the call's scale) (K = 48, N <= 256, C >= 32; ws as for c3dgs_weighted_distance_ws), so the error the ambiguity margin must cover can be measured against float64. */
int c3dgs_debug_wd_scores(int64_t N, int32_t C, int32_t K, const float* coefs, const float* codebook, float* scores, void* ws,
                          size_t ws_bytes, float* out_dist, int64_t* out_idx, void* stream);

/* ================= measurement entries: exported ONLY by the diag variants of the library (csrc/diag.hip) =================
 * c3dgs_amd/build.py DIAG_VARIANTS ("lanes", "bwdtime", "ostime": python -m c3dgs_amd.build --diag). Every variant exports all
 * three; a variant that does not collect a kind of data reports zeros for it. */

/* phase time stamps of the last digit pass the onesweep sorts ran, 64 tiles x 8 stamps of the shader clock. All zero unless the
 * library is the "ostime" variant (radix_sort.hip compiled with -DC3DGS_OS_TIMING). */
int c3dgs_debug_sort_times(uint64_t* out /*[512], host*/);

/* access patterns with a KNOWN byte count, for calibrating the rocprofv3 FETCH_SIZE / WRITE_SIZE counters on this
 * GPU (tools/pmc_calibrate.py -> profiles/r03_pmc_calibration.txt). kind 0: coalesced 16-byte-per-lane read of n x 16 bytes of
 * `table`; 1: n lanes each read the 48-byte record index[i] (three 16-byte loads); 2: the 192-byte row index[i] (twelve); 3: n
 * lanes each store nine floats to the 36-byte slot index[i]. `out`: one word, practically never written. */
int c3dgs_debug_gather_probe(int32_t kind, int64_t n, void* table, const uint32_t* index, uint32_t* out, void* stream);

/* lane-efficiency counters of the two blend kernels, accumulated since the last call and cleared by it.
 * out[0..7] forward, out[8..15] backward: { (wave, Gaussian) pairs run, slots incl. list padding, pixel lanes that used the pair,
 * pairs with >= 1 such lane, iterations an 8x4-pixel half-wave unit would run, iterations a 4x4-pixel unit would run,
 * candidate lists walked, forward: lanes hit incl. finished pixels }. All zero unless the library is the "lanes"
 * variant (render.hip compiled with -DC3DGS_COUNT_LANES). In the "bwdtime" variant (-DC3DGS_BWD_TIMING) the same 16 words hold
 * render_backward's phase clock instead: out[0..8] = shader-clock ticks per phase (csrc/render_diag.hpp PhaseClock::Phase), summed
 * over the waves that had work, out[9] = the sum of their lifetimes, out[10] = their number. Synchronises the stream. */
int c3dgs_debug_lane_counters(uint64_t* out /*[16], host*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* C3DGS_HIP_DEBUG_H */
