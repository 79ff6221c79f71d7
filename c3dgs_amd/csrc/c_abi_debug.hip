// c_abi_debug.hip -- the test hooks of include/c3dgs_hip_debug.h: entry points the GPU tests use to drive the product's own sorts
// and codeword search directly. Part of the product library; not part of its public ABI.
#include "common.hpp"
#include "../../include/c3dgs_hip_debug.h"
#include "../../include/c3dgs_hip_depth_sort_debug.h"

using namespace c3dgs;

extern "C" {

size_t c3dgs_debug_sort_temp_bytes(int32_t key_bytes, int64_t n, int32_t end_bit)
{
    if (n <= 0 || n > 0x3fffffff) return 256;
    return key_bytes == 2 ? onesweep_tile_temp_bytes((int)n, end_bit) : onesweep_depth_temp_bytes((int)n);
}

int c3dgs_debug_sort_pairs(int32_t key_bytes, int64_t n, int32_t end_bit, const void* keys_in, void* keys_out,
                           const uint32_t* values_in, uint32_t* values_out, void* temp, size_t temp_bytes, void* stream)
{
    if ((key_bytes != 2 && key_bytes != 4) || n < 0 || n > 0x3fffffff || end_bit < 1 || end_bit > 8 * key_bytes)
        return fail(C3DGS_E_INVALID, "debug_sort_pairs: bad arguments");
    if (key_bytes == 4 && end_bit != 32) return fail(C3DGS_E_INVALID, "debug_sort_pairs: 4-byte keys are sorted on all 32 bits");
    if (n == 0) return C3DGS_OK;
    if (!keys_in || !keys_out || !values_in || !values_out || !temp) return fail(C3DGS_E_INVALID, "debug_sort_pairs: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    if (key_bytes == 2)
        C3DGS_HIP_TRY(onesweep_tile_sort(temp, temp_bytes, (const uint16_t*)keys_in, (uint16_t*)keys_out, values_in, values_out, (int)n,
                                         end_bit, s));
    else
        C3DGS_HIP_TRY(onesweep_depth_sort(temp, temp_bytes, (const uint32_t*)keys_in, (uint32_t*)keys_out, values_in, values_out, (int)n,
                                          nullptr, nullptr, s));
    C3DGS_STAGE("debug_sort_pairs", 1, s);
    if (onesweep_timed_out(s)) return fail(C3DGS_E_HIP, "debug_sort_pairs: look-back timed out");
    return C3DGS_OK;
}

// the forward's tile sort for a grid of `tiles` tiles: key width and end_bit as forward_impl / binning_layout choose them.
// Largest grid validate() admits: 256 x 65,535 tiles (tiles_x^2 x tiles_y < 2^32, tiles_y <= 65,535)
static bool debug_tile_sort_args_ok(int32_t tiles, int64_t n)
{
    return tiles >= 1 && (long long)tiles <= 256LL * 65535 && n >= 0 && n <= 0x3fffffff;
}

size_t c3dgs_debug_tile_sort_temp_bytes(int32_t tiles, int64_t n)
{
    if (!debug_tile_sort_args_ok(tiles, n)) { set_error("debug_tile_sort_temp_bytes: bad arguments"); return 0; }
    return sort_temp_bytes((int)n, tile_sort_end_bit_for(tiles), tile_key_bytes_for(tiles));
}

int c3dgs_debug_tile_sort_pairs(int32_t tiles, int64_t n, const void* keys_in, void* keys_out, const uint32_t* values_in,
                                uint32_t* values_out, void* temp, size_t temp_bytes, void* stream)
{
    if (!debug_tile_sort_args_ok(tiles, n)) return fail(C3DGS_E_INVALID, "debug_tile_sort_pairs: bad arguments");
    if (n == 0) return C3DGS_OK;
    if (!keys_in || !keys_out || !values_in || !values_out || !temp)
        return fail(C3DGS_E_INVALID, "debug_tile_sort_pairs: NULL buffer");
    const int kb = tile_key_bytes_for(tiles), end_bit = tile_sort_end_bit_for(tiles);
    if (temp_bytes < sort_temp_bytes((int)n, end_bit, kb))
        return fail(C3DGS_E_INVALID, "debug_tile_sort_pairs: temp smaller than c3dgs_debug_tile_sort_temp_bytes()");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_HIP_TRY(run_tile_sort(temp, temp_bytes, keys_in, keys_out, kb, values_in, values_out, (int)n, end_bit, s, false));
    C3DGS_STAGE("debug_tile_sort_pairs", 1, s);
    if (onesweep_timed_out(s)) return fail(C3DGS_E_HIP, "debug_tile_sort_pairs: look-back timed out");
    return C3DGS_OK;
}

int c3dgs_debug_depth_plan(int32_t biased, uint32_t max_visible_key, int64_t n, const uint32_t* keys, uint32_t* plan, uint32_t* digits)
{
    if (!plan || n < 0 || (n > 0 && digits && !keys)) return fail(C3DGS_E_INVALID, "debug_depth_plan: bad arguments");
    const DepthSortPlan dp = depth_sort_plan(biased != 0, max_visible_key);
    plan[0] = (uint32_t)dp.passes;
    for (int q = 0; q < 4; q++) plan[1 + q] = q < dp.passes ? (uint32_t)dp.bits[q] : 0u;
    plan[5] = dp.bias;
    if (digits)
        for (int64_t i = 0; i < n; i++)
            for (int q = 0; q < 4; q++) digits[4 * i + q] = q < dp.passes ? depth_sort_digit(dp, keys[i], q) : 0u;
    return C3DGS_OK;
}

static bool debug_depth_sort_args_ok(int64_t n) { return n >= 1 && n <= 0x3fffffff && onesweep_enabled(); }

size_t c3dgs_debug_depth_sort_temp_bytes(int64_t n)
{
    if (!debug_depth_sort_args_ok(n)) return 256;
    return onesweep_depth_temp_bytes((int)n) + 256;                 // + the one word the histogram launch's scan half leaves
}

int c3dgs_debug_depth_sort(int64_t n, int32_t prefiltered, const uint32_t* keys, const void* rects, uint32_t* order,
                           uint32_t* keys_sorted, void* rects_sorted, void* temp, size_t temp_bytes, int32_t* passes_run, void* stream)
{
    if (!debug_depth_sort_args_ok(n)) return fail(C3DGS_E_INVALID, "debug_depth_sort: bad arguments (or the rocPRIM path is selected)");
    if (!keys || !rects || !order || !keys_sorted || !rects_sorted || !temp || !passes_run)
        return fail(C3DGS_E_INVALID, "debug_depth_sort: NULL buffer");
    if (temp_bytes < c3dgs_debug_depth_sort_temp_bytes(n))
        return fail(C3DGS_E_INVALID, "debug_depth_sort: temp smaller than c3dgs_debug_depth_sort_temp_bytes()");
    hipStream_t s = (hipStream_t)stream;
    const int P = (int)n;
    const size_t sort_bytes = onesweep_depth_temp_bytes(P);
    const uint2* r_in = (const uint2*)rects;
    uint2* r_out = (uint2*)rects_sorted;
    if (prefiltered || !depth_sort3_available(P, sort_bytes, true)) {
        C3DGS_HIP_TRY(run_depth_sort(temp, sort_bytes, keys, keys_sorted, nullptr, order, P, r_in, r_out, s, false, true, false));
        *passes_run = 4;
    } else {
        uint32_t* scan_word = (uint32_t*)((char*)temp + sort_bytes);
        uint32_t max_key = 0;
        C3DGS_HIP_TRY(hipMemsetAsync(temp, 0, depth_sort_clear_bytes(P), s));
        C3DGS_HIP_TRY(onesweep_depth3_hist_scan(temp, sort_bytes, keys, P, 0, scan_word, nullptr, nullptr, 0u, nullptr, s));
        C3DGS_HIP_TRY(onesweep_depth3_head(temp, sort_bytes, keys, P, r_in, s));
        C3DGS_HIP_TRY(hipMemcpyAsync(&max_key, onesweep_depth3_max_word(temp, P), sizeof(max_key), hipMemcpyDeviceToHost, s));
        C3DGS_HIP_TRY(hipStreamSynchronize(s));
        C3DGS_HIP_TRY(onesweep_depth3_tail(temp, sort_bytes, keys, keys_sorted, order, P, r_in, r_out, max_key, s));
        *passes_run = depth_sort_plan(true, max_key).passes;
    }
    C3DGS_STAGE("debug_depth_sort", 1, s);
    if (onesweep_timed_out(s)) return fail(C3DGS_E_HIP, "debug_depth_sort: look-back timed out");
    return C3DGS_OK;
}

int c3dgs_debug_wd_scores(int64_t N, int32_t C, int32_t K, const float* coefs, const float* codebook, float* scores, void* ws,
                          size_t ws_bytes, float* out_dist, int64_t* out_idx, void* stream)
{
    if (!coefs || !codebook || !scores || !out_dist || !out_idx) return fail(C3DGS_E_INVALID, "debug_wd_scores: bad arguments");
    if (launch_wd_debug_scores(N, C, K, coefs, codebook, scores, ws, ws_bytes, out_dist, out_idx, (hipStream_t)stream))
        return fail(C3DGS_E_INVALID, "debug_wd_scores: K = 48, 1 <= N <= 256, C >= 32 and scratch of c3dgs_weighted_distance_ws_bytes");
    return C3DGS_OK;
}

} // extern "C"
