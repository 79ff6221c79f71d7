/*
 * c3dgs_hip_depth_sort_debug.h -- test hooks into the depth sort of the binning stage (csrc/radix_sort.hip, csrc/common.hpp:
 * depth_sort_plan). Exported by the product library (csrc/c_abi_debug.hip); NOT part of its public ABI, like the entries of
 * c3dgs_hip_debug.h. Conventions as in c3dgs_hip.h.
 */
#ifndef C3DGS_HIP_DEPTH_SORT_DEBUG_H
#define C3DGS_HIP_DEPTH_SORT_DEBUG_H

#include "c3dgs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* host only, no device work: the digit plan the depth sort takes for a forward whose largest visible key is max_visible_key
 * (`biased` = the forward is not prefiltered). plan[0] = passes, plan[1..4] = bits per pass (least significant digit first),
 * plan[5] = the bias. digits (optional, host, [n][4]): the digits of the n host keys under that plan, unused passes 0. */
int c3dgs_debug_depth_plan(int32_t biased, uint32_t max_visible_key, int64_t n, const uint32_t* keys, uint32_t* plan /*[6]*/,
                           uint32_t* digits);

/* the forward's depth sort on caller-provided device arrays: n keys, n tile rectangles (two words each, every coordinate below
 * 256, as preprocess writes them for grids up to 255 x 255 tiles) -> ids in (key, id) order, the keys and the rectangles in that
 * order. prefiltered = 0 takes the biased plan exactly as the forward does (histogram with the largest visible key, two passes,
 * then one or two more); 1 the four 8-bit passes. *passes_run reports the number of digit passes. Synchronises the stream.
 * temp >= c3dgs_debug_depth_sort_temp_bytes(n). */
size_t c3dgs_debug_depth_sort_temp_bytes(int64_t n);
int c3dgs_debug_depth_sort(int64_t n, int32_t prefiltered, const uint32_t* keys, const void* rects, uint32_t* order,
                           uint32_t* keys_sorted, void* rects_sorted, void* temp, size_t temp_bytes, int32_t* passes_run, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* C3DGS_HIP_DEPTH_SORT_DEBUG_H */
