// c_abi_debug.hip -- the test hooks of include/c3dgs_hip_debug.h: entry points the GPU tests use to drive the product's own sorts
// and codeword search directly. Part of the product library; not part of its public ABI.
#include "common.hpp"
#include "../../include/c3dgs_hip_debug.h"

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

int c3dgs_debug_wd_scores(int64_t N, int32_t C, int32_t K, const float* coefs, const float* codebook, float* scores, void* ws,
                          size_t ws_bytes, float* out_dist, int64_t* out_idx, void* stream)
{
    if (!coefs || !codebook || !scores || !out_dist || !out_idx) return fail(C3DGS_E_INVALID, "debug_wd_scores: bad arguments");
    if (launch_wd_debug_scores(N, C, K, coefs, codebook, scores, ws, ws_bytes, out_dist, out_idx, (hipStream_t)stream))
        return fail(C3DGS_E_INVALID, "debug_wd_scores: K = 48, 1 <= N <= 256, C >= 32 and scratch of c3dgs_weighted_distance_ws_bytes");
    return C3DGS_OK;
}

} // extern "C"
