// c_abi.hip -- extern "C" entry points of libc3dgs_hip.so (declared in include/c3dgs_hip.h).
// Stage order follows the reference's Rasterizer::forward / backward (cuda_rasterizer/rasterizer_impl.cu:194-334,
// 338-435, 440-586, 590-697); the stages themselves are the gfx950 kernels in this directory.
#include "common.hpp"
#include "mcmc.hpp"
#include "bilagrid.hpp"
#include <cfloat>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace c3dgs {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// ---- optional per-stage timing with HIP events recorded on the caller's stream (bench.py's roofline leg).
// Disabled by default: zero cost. When enabled, every stage launch is bracketed by two events; nothing
// synchronises until c3dgs_profile_read().
// The timed stages: ST_<id> and the name c3dgs_profile_read() reports and c3dgs_profile_only() selects (bench.py and tools/ go
// by these names). Launches outside this table are checked with C3DGS_STAGE under a name of their own and never timed.
#define C3DGS_STAGE_TABLE(X)                                                                                                   \
    X(MARK_VISIBLE, "mark_visible") X(PREPROCESS, "preprocess") X(DEPTH_SORT, "depth_sort") X(SCAN, "scan")                    \
    X(DUPLICATE, "duplicate_with_keys") X(SORT, "sort") X(RANGES, "identify_ranges") X(RENDER_FWD, "render_forward")           \
    X(RENDER_DEPTH, "render_depth") X(RENDER_DISTORTION, "render_distortion")                                                  \
    X(RENDER_CONTRIB, "render_contrib") X(RENDER_CONTRIB_BLEND, "render_contrib_blend") X(RENDER_CONTRIB_SUM, "render_contrib_sum") \
    X(RENDER_ERROR, "render_error") X(RENDER_ERROR_BLEND, "render_error_blend") X(RENDER_ERROR_SUM, "render_error_sum")           \
    X(ERROR_MAP_L1, "error_map_l1")                                                                                            \
    X(POSE_GRAD, "pose_grad") X(POSE_GRAD_SUMS, "pose_grad_sums") X(POSE_GRAD_FOLD, "pose_grad_fold")                          \
    X(ZERO_PARTIALS, "zero_partials") X(RENDER_BWD, "render_backward") X(BWD_PREPROCESS, "backward_preprocess")                \
    X(RENDER_DEPTH_BWD, "render_depth_backward") X(DEPTH_BWD_FOLD, "depth_backward_fold")                                      \
    X(RENDER_DISTORTION_BWD, "render_distortion_backward")                                                                     \
    X(GAUSSIAN_NORMALS, "gaussian_normals") X(RENDER_NORMAL, "render_normal") X(RENDER_NORMAL_BWD, "render_normal_backward")   \
    X(NORMAL_BWD_FOLD, "normal_backward_fold") X(DEPTH_TO_NORMAL, "depth_to_normal")                                           \
    X(DEPTH_TO_NORMAL_BWD, "depth_to_normal_backward")                                                                         \
    X(WDIST, "weighted_distance") X(VQ_ACC, "vq_accumulate") X(VQ_APPLY, "vq_apply") X(LOSS_FWD, "l1_ssim_forward")            \
    X(LOSS_BWD, "l1_ssim_backward") X(QAT_OBSERVE, "qat_observe") X(QAT_CODEBOOKS, "qat_codebooks")                            \
    X(QAT_VISIBLE, "qat_visible") X(QAT_POINTS, "qat_points") X(QAT_POINTS_BWD, "qat_points_backward")                         \
    X(QAT_CODEBOOKS_BWD, "qat_codebooks_backward") X(ADAM, "adam_step") X(KNN_SORT, "knn_sort") X(KNN_BOUNDS, "knn_bounds")    \
    X(KNN_QUERY, "knn_query") X(SPARSE_ADAM_SELECT, "sparse_adam_select") X(SPARSE_ADAM_STEP, "sparse_adam_step")              \
    X(AA_OPACITY, "aa_opacity") X(AA_OPACITY_BWD, "aa_opacity_backward")                                                       \
    X(MCMC_WEIGHTS, "mcmc_weights") X(MCMC_SEARCH, "mcmc_search") X(MCMC_VALUES, "mcmc_values") X(MCMC_APPLY, "mcmc_apply")    \
    X(MCMC_NOISE, "mcmc_noise")                                                                                                \
    X(BILAGRID_SLICE, "bilagrid_slice") X(BILAGRID_SLICE_BWD, "bilagrid_slice_backward") X(BILAGRID_GATHER, "bilagrid_gather") \
    X(BILAGRID_FOLD, "bilagrid_fold") X(BILAGRID_RGB_BWD, "bilagrid_rgb_backward") X(BILAGRID_TV, "bilagrid_tv")               \
    X(BILAGRID_TV_BWD, "bilagrid_tv_backward")                                                                                 \
    X(FILTER3D_COMPUTE, "filter3d_compute") X(FILTER3D_APPLY, "filter3d_apply") X(FILTER3D_APPLY_BWD, "filter3d_apply_backward") \
    X(TSDF_INTEGRATE, "tsdf_integrate") X(MESH_CLASSIFY, "mesh_classify") X(MESH_SCAN, "mesh_scan")                            \
    X(MESH_EMIT_VERTICES, "mesh_emit_vertices") X(MESH_EMIT_FACES, "mesh_emit_faces")                                          \
    X(NN_QUERY_SORT, "nn_query_sort") X(NN_QUERY, "nn_query") X(MESH_SAMPLE_COUNT, "mesh_sample_count")                        \
    X(MESH_SAMPLE_SCAN, "mesh_sample_scan") X(MESH_SAMPLE_EMIT, "mesh_sample_emit") X(GEOMETRY_REDUCE, "geometry_reduce")
#define C3DGS_X(id, name) ST_##id,
enum Stage { C3DGS_STAGE_TABLE(C3DGS_X) ST_COUNT };
#undef C3DGS_X
#define C3DGS_X(id, name) name,
static const char* const kStageNames[ST_COUNT] = { C3DGS_STAGE_TABLE(C3DGS_X) };
#undef C3DGS_X
struct ProfRec { int stage; hipEvent_t a, b; };
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static int g_prof_only = -1;        // >= 0: bracket only this stage (two events per launch of ONE kernel)
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_prof_pool;

struct StageTimer {
    bool on; int stage; hipStream_t s; hipEvent_t a{}, b{};
    StageTimer(int stage_, hipStream_t s_) : on(g_prof_on && (g_prof_only < 0 || g_prof_only == stage_)), stage(stage_), s(s_)
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        auto get = [&](hipEvent_t& e) {
            if (!g_prof_pool.empty()) { e = g_prof_pool.back(); g_prof_pool.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) on = false;
        };
        get(a); get(b);
        if (on) (void)hipEventRecord(a, s);
    }
    ~StageTimer()
    {
        if (!on) return;
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof_recs.push_back({ stage, a, b });
    }
};
// after a timed stage: the launch check of C3DGS_STAGE under the stage's name in the table
#define C3DGS_STAGE_CHECK(stage, debug, stream) C3DGS_STAGE(kStageNames[stage], debug, stream)
// a timed stage that is ONE launch call: the events around it, then the check (a body that can return early stays written out)
#define C3DGS_TIMED_STAGE(stage, debug, stream, ...)                                                \
    do {                                                                                            \
        { StageTimer t_(stage, stream); __VA_ARGS__; }                                              \
        C3DGS_STAGE_CHECK(stage, debug, stream);                                                    \
    } while (0)

// Landing pad of the forward's single device->host read (one per calling thread): 64 bytes of page-locked host memory. When
// the allocation can be MAPPED into the device's address space (coherent, fine-grained: the normal case), the kernel that
// produces num_rendered stores {num_rendered, sort error word, sequence number} straight into it and the host polls the
// sequence number -- no copy command on the stream (a ~4 us launch + a ~6 us bubble per forward). Otherwise (`dev` null):
// a hipMemcpyAsync into it behind an event, as before.
// One read is begin() -> [the producing kernel is launched with `dev` and the sequence number] -> queue_copy() -> wait().
// Words 3 and 4 of the mapped pad are a second read of the same kind, {largest visible depth key, sequence number}, which the
// biased depth sort's histogram stores when its last workgroup finishes: wait_max().
struct HostRead {
    uint32_t* pinned = nullptr;
    uint32_t* dev = nullptr;      // device-side address of `pinned`, or null
    uint32_t seq = 0;             // mapped pad: sequence number of the read in flight
    hipEvent_t ev{};
    HostRead()
    {
        const char* e = std::getenv("C3DGS_HOST_READ_COPY");            // "1": force the copy path (test / diagnosis)
        const bool want_map = !(e && e[0] == '1');
        if (want_map && hipHostMalloc((void**)&pinned, 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) == hipSuccess) {
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, pinned, 0) == hipSuccess) dev = (uint32_t*)d;
            std::memset(pinned, 0, 64);
        } else {
            (void)hipGetLastError();
            if (hipHostMalloc((void**)&pinned, 64, hipHostMallocDefault) != hipSuccess) { pinned = nullptr; return; }
        }
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(pinned); pinned = nullptr; dev = nullptr; }
    }
    // -> the sequence number the producing kernel stores behind the two words (0 on the copy path: nothing is stored)
    uint32_t begin()
    {
        if (!dev) return 0u;
        if (++seq == 0u) seq = 1u;                                       // (wrap-around: 0 is the pad's initial value)
        return seq;
    }
    // the two words at `src`, {num_rendered, sort error word}, into the pad
    int copy_words(const uint32_t* src, hipStream_t s)
    {
        C3DGS_HIP_TRY(hipMemcpyAsync(pinned, src, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return C3DGS_OK;
    }
    // copy path: the copy lands in pinned memory behind an event; to be queued as soon as the words exist on the stream
    int queue_copy(const uint32_t* src, hipStream_t s)
    {
        if (dev) return C3DGS_OK;
        if (int rc = copy_words(src, s)) return rc;
        C3DGS_HIP_TRY(hipEventRecord(ev, s));
        return C3DGS_OK;
    }
    // -> words[2] of this read. Polls instead of sleeping in the driver: on a busy host the wake-up from a blocking event wait
    // can take milliseconds (seen as a 2x slower step with unchanged kernel times); the words are normally there within ~100 us.
    int wait(const uint32_t* src, hipStream_t s, uint32_t words[2])
    {
        if (dev) {
            // mapped pad: wait for this read's sequence number. Every ~64k polls the stream is queried as well: if it has drained
            // (or failed) and the number still is not there, the store never became visible -> fetch the two words with a copy
            volatile uint32_t* pad = pinned;
            bool seen = false;
            for (long spins = 0; !seen; spins++) {
                seen = __atomic_load_n(&pad[2], __ATOMIC_ACQUIRE) == seq;
                if (!seen && (spins & 0xffff) == 0xffff) {
                    const hipError_t q = hipStreamQuery(s);
                    if (q == hipErrorNotReady) continue;
                    if (q != hipSuccess) return fail(C3DGS_E_HIP, std::string("num_rendered read: ") + hipGetErrorString(q));
                    seen = __atomic_load_n(&pad[2], __ATOMIC_ACQUIRE) == seq;
                    if (!seen) {
                        if (int rc = copy_words(src, s)) return rc;
                        C3DGS_HIP_TRY(hipStreamSynchronize(s));
                        seen = true;
                    }
                }
            }
        } else {
            hipError_t q = hipErrorNotReady;
            for (long spins = 0; spins < 20000000L && (q = hipEventQuery(ev)) == hipErrorNotReady; spins++) { }
            if (q == hipErrorNotReady) q = hipEventSynchronize(ev);
            if (q != hipSuccess) return fail(C3DGS_E_HIP, std::string("num_rendered read: ") + hipGetErrorString(q));
        }
        words[0] = pinned[0]; words[1] = pinned[1];
        return C3DGS_OK;
    }
    // mapped pad only: the largest visible depth key of this read (device copy of the word at `src`), polled like wait()
    int wait_max(const uint32_t* src, hipStream_t s, uint32_t* max_key)
    {
        volatile uint32_t* pad = pinned;
        for (long spins = 0;; spins++) {
            if (__atomic_load_n(&pad[4], __ATOMIC_ACQUIRE) == seq) { *max_key = pinned[3]; return C3DGS_OK; }
            if ((spins & 0xffff) != 0xffff) continue;
            const hipError_t q = hipStreamQuery(s);
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) return fail(C3DGS_E_HIP, std::string("depth key range read: ") + hipGetErrorString(q));
            if (__atomic_load_n(&pad[4], __ATOMIC_ACQUIRE) == seq) { *max_key = pinned[3]; return C3DGS_OK; }
            C3DGS_HIP_TRY(hipMemcpyAsync(pinned + 3, src, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            C3DGS_HIP_TRY(hipStreamSynchronize(s));
            *max_key = pinned[3];
            return C3DGS_OK;
        }
    }
};
static HostRead& host_read()
{
    static thread_local HostRead h;
    return h;
}

static int validate(const c3dgs_raster_params* p, bool indexed, bool is_backward)
{
    if (!p) return fail(C3DGS_E_INVALID, "params is NULL");
    if (p->P < 0 || p->W <= 0 || p->H <= 0) return fail(C3DGS_E_INVALID, "P, W, H must be non-negative / positive");
    if (p->P == 0) return C3DGS_OK;
    if (!p->means3D) return fail(C3DGS_E_INVALID, "means3D must have dimensions (num_points, 3)"); // rasterize_points.cu:58-60
    if (!p->background || !p->viewmatrix || !p->projmatrix || !p->campos)
        return fail(C3DGS_E_INVALID, "background, viewmatrix, projmatrix and campos are required");
    if (!is_backward && !p->opacities) // the backward reads opacities from the geometry buffer, as the reference does
        return fail(C3DGS_E_INVALID, "opacities is required");
    if ((p->sh == nullptr) == (p->colors_precomp == nullptr))
        return fail(C3DGS_E_INVALID, "Please provide excatly one of either SHs or precomputed colors!");
    const bool has_sr = p->scales != nullptr && p->rotations != nullptr;
    if ((p->scales != nullptr) != (p->rotations != nullptr) || has_sr == (p->cov3D_precomp != nullptr))
        return fail(C3DGS_E_INVALID, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (p->sh) {
        if (p->D < 0 || p->D > 3) return fail(C3DGS_E_INVALID, "SH degree must be in [0,3]");
        if (p->M < (p->D + 1) * (p->D + 1)) return fail(C3DGS_E_INVALID, "sh has fewer coefficients than the active degree needs");
    }
    if (indexed) {
        if (p->sh && !p->sh_indices) return fail(C3DGS_E_INVALID, "indexed rasterizer: sh_indices is required with sh");
        if (has_sr && (!p->g_indices || !p->scale_factors))
            return fail(C3DGS_E_INVALID, "indexed rasterizer: g_indices and scale_factors are required with scales/rotations");
    } else if (p->sh_indices || p->g_indices || p->scale_factors) {
        return fail(C3DGS_E_INVALID, "non-indexed rasterizer: sh_indices / g_indices / scale_factors must be NULL");
    }
    if (tiles_x(p->W) > 65535 || tiles_y(p->H) > 65535) return fail(C3DGS_E_INVALID, "image too large for 16-bit tile coordinates");
    // Up to 65,536 tiles the tile keys are 16 bits, above 32 bits (common.hpp: tile_key_bytes). The bound that remains: the pair
    // emission divides an instance's number inside its rectangle by the rectangle's width with a multiply-high that is exact
    // while (tiles per row)^2 x (tile rows) < 2^32 -- e.g. 16384 x 16384 pixels = 2^30, 7680 x 4320 = 6.2e7.
    if ((unsigned long long)tiles_x(p->W) * tiles_x(p->W) * tiles_y(p->H) >= (1ull << 32))
        return fail(C3DGS_E_INVALID, "image too large: (tiles per row)^2 x (tile rows) must stay below 2^32");
    return C3DGS_OK;
}

static int forward_impl(const c3dgs_raster_params* pp, bool indexed, c3dgs_resize_fn geom_resize, void* geom_user,
                        c3dgs_resize_fn binning_resize, void* binning_user, c3dgs_resize_fn image_resize, void* image_user,
                        float* out_color, int32_t* radii, int32_t* num_rendered, void* stream_)
{
    if (int rc = validate(pp, indexed, false)) return rc;
    if (!out_color || !num_rendered) return fail(C3DGS_E_INVALID, "out_color and num_rendered are required");
    if (!geom_resize || !binning_resize || !image_resize) return fail(C3DGS_E_INVALID, "resize callbacks are required");
    c3dgs_raster_params p = *pp;
    if (!indexed) { p.sh_indices = nullptr; p.g_indices = nullptr; p.scale_factors = nullptr; }
    hipStream_t s = (hipStream_t)stream_;
    const int P = p.P, W = p.W, H = p.H;
    const int gx = tiles_x(W), gy = tiles_y(H);
    *num_rendered = 0;

    ImageLayout IL; image_layout(W, H, &IL);
    void* img_base = image_resize(image_user, IL.total_bytes);
    if (!img_base) return fail(C3DGS_E_ALLOC, "image buffer allocation failed");
    const ImgPtrs img = img_ptrs(img_base, W, H);

    if (P == 0) { // reference returns zero-filled outputs (rasterize_points.cu:69-70,82)
        C3DGS_HIP_TRY(hipMemsetAsync(out_color, 0, (size_t)3 * W * H * sizeof(float), s));
        C3DGS_HIP_TRY(hipMemsetAsync(img_base, 0, IL.total_bytes, s));
        return C3DGS_OK;
    }
    if (!radii) return fail(C3DGS_E_INVALID, "radii is required");

    c3dgs_geom_layout GL; geom_layout(P, &GL);
    void* geom_base = geom_resize(geom_user, GL.total_bytes + geom_gtab_bytes(p));
    if (!geom_base) return fail(C3DGS_E_ALLOC, "geometry buffer allocation failed");
    const GeomPtrs g = geom_ptrs(geom_base, P);

    // K2 / K2i, with the id-order scan of tiles_touched folded in (per-workgroup offsets + block_base[])
    uint32_t* sort_err = onesweep_error_word();
    if (!sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    HostRead& hr = host_read();
    if (!hr.pinned) return fail(C3DGS_E_HIP, "pinned host buffer allocation failed");
    const uint32_t host_seq = hr.begin();
    // the depth sort's control words are cleared by preprocess's workgroups (0 bytes: that sort clears its own)
    const size_t dclear = depth_sort_clear_bytes(P) <= g.scan_temp_bytes ? depth_sort_clear_bytes(P) : 0;
    // the id-order scan behind preprocess shares its launch with the depth sort's histograms where that sort is the hand-written
    // one and preprocess has cleared its control words; otherwise it runs alone and the sort does everything itself
    const bool hist_with_scan = dclear != 0;
    // the depth sort on biased keys in three passes (radix_sort.hip): every visible key has passed the near-plane test, and the
    // host can read the largest one from the mapped pad. Otherwise the four 8-bit passes on the raw keys.
    const bool rects_fit_bytes = gx <= 255 && gy <= 255;
    const bool sort3 = hist_with_scan && hr.dev && !p.prefiltered && depth_sort3_available(P, g.scan_temp_bytes, rects_fit_bytes);
    const int nb = (P + 255) / 256;
    { StageTimer t_(ST_PREPROCESS, s);
      if (geom_gtab_bytes(p)) launch_pack_codebook(p, g.gtab, s);
      launch_preprocess(p, g, radii, img.ranges, g.scan_temp, dclear / 16, s);
      if (sort3)
          C3DGS_HIP_TRY(onesweep_depth3_hist_scan(g.scan_temp, g.scan_temp_bytes, g.depth_keys, P, nb, g.block_base, sort_err, hr.dev, host_seq,
                                                  hr.dev + 3, s));
      else if (hist_with_scan)
          C3DGS_HIP_TRY(run_depth_hist_scan(g.scan_temp, g.scan_temp_bytes, g.depth_keys, P, nb, g.block_base, sort_err, hr.dev, host_seq, s));
      else
          launch_scan_blocks(nb, g.block_base, sort_err, hr.dev, host_seq, s); }
    C3DGS_STAGE_CHECK(ST_PREPROCESS, p.debug, s);
    // The one device->host read of the forward (K4, num_rendered) is issued as EARLY as its value exists: R is the last
    // entry of block_base[]. It lands in the host pad while the depth sort and the depth-order scan are already queued, so
    // the GPU keeps working while the host waits, sizes the binning buffer and queues the rest (the reference blocks the
    // stream at this point, rasterizer_impl.cu:279).
    // second word: the device's sticky sort time-out flag as of the start of this call (radix_sort.hip)
    const uint32_t* r_words = g.block_base + nb;
    if (int rc = hr.queue_copy(r_words, s)) return rc;
    uint32_t words[2];
    if (sort3) {
        // The host read moves in front of the last pass: passes 1 and 2 are the same whatever the key range, so they are queued
        // first and run while the host wakes up; the largest visible key then decides between one more pass and two.
        // One timed stage around both halves: a bubble in front of the last pass would show in it.
        StageTimer t_(ST_DEPTH_SORT, s);                                             // binning stage 1: P Gaussians by depth
        C3DGS_HIP_TRY(onesweep_depth3_head(g.scan_temp, g.scan_temp_bytes, g.depth_keys, P, reinterpret_cast<const uint2*>(g.rects), s));
        uint32_t max_key = 0;
        if (int rc = hr.wait_max(onesweep_depth3_max_word(g.scan_temp, P), s, &max_key)) return rc;
        C3DGS_HIP_TRY(onesweep_depth3_tail(g.scan_temp, g.scan_temp_bytes, g.depth_keys, g.depth_keys_sorted, g.depth_order, P,
                                           reinterpret_cast<const uint2*>(g.rects), g.sorted_offsets, max_key, s));
    } else {
        StageTimer t_(ST_DEPTH_SORT, s);
        C3DGS_HIP_TRY(run_depth_sort(g.scan_temp, g.scan_temp_bytes, g.depth_keys, g.depth_keys_sorted, nullptr, g.depth_order, P,
                                     reinterpret_cast<const uint2*>(g.rects), g.sorted_offsets, s, dclear != 0, rects_fit_bytes, hist_with_scan));
    }
    C3DGS_STAGE_CHECK(ST_DEPTH_SORT, p.debug, s);
    if (p.debug && onesweep_timed_out(s)) return fail(C3DGS_E_HIP, "depth sort: look-back timed out");
    C3DGS_TIMED_STAGE(ST_SCAN, p.debug, s, launch_depth_order_scan(P, g, s));        // K3, in depth order (two-level)
    if (int rc = hr.wait(r_words, s, words)) return rc;
    const uint32_t R_u = words[0];
    if (words[1] != 0) {
        // A radix-sort look-back timed out in an EARLIER rasterizer call on this device (that call's image was poisoned with
        // NaN by render_forward). Not silent outside debug mode: fail here, at the forward's one natural host read.
        C3DGS_HIP_TRY(hipMemsetAsync(sort_err, 0, sizeof(uint32_t), s));
        return fail(C3DGS_E_HIP, "radix sort look-back timed out in an earlier rasterizer call on this device: that call's "
                                 "image is NaN and its gradients are invalid (flag cleared, this call was not run)");
    }
    if (R_u > 0x7fffffffu) return fail(C3DGS_E_INVALID, "num_rendered overflows int32");
    const int R = (int)R_u;
    *num_rendered = R;

    c3dgs_binning_layout BL; binning_layout(R, W, H, &BL);
    void* bin_base = binning_resize(binning_user, BL.total_bytes);
    if (!bin_base) return fail(C3DGS_E_ALLOC, "binning buffer allocation failed");
    const BinPtrs b = bin_ptrs(bin_base, R, W, H);

    if (R > 0) {
        const int end_bit = tile_sort_end_bit(W, H);                                // tile bits only (rasterizer_impl.cu:298)
        // the tile sort's control words are cleared by the pair emission's workgroups (0 bytes: that sort clears its own, or --
        // the table-driven sort of 16-bit keys -- has none to clear)
        size_t tclear = tile_sort_clear_bytes(R, end_bit, b.key_bytes);
        if (tclear > b.sort_temp_bytes) tclear = 0;
        C3DGS_TIMED_STAGE(ST_DUPLICATE, p.debug, s, launch_duplicate_with_keys(P, g, b, gx, sort_err, b.sort_temp, tclear / 16, s)); // K5
        { StageTimer t_(ST_SORT, s);
          C3DGS_HIP_TRY(run_tile_sort(b.sort_temp, b.sort_temp_bytes, b.keys_unsorted, b.keys_sorted, b.key_bytes, b.values_unsorted,
                                      b.point_list, R, end_bit, s, tclear != 0)); }  // K6, binning stage 2
        C3DGS_STAGE_CHECK(ST_SORT, p.debug, s);
        if (p.debug && onesweep_timed_out(s)) return fail(C3DGS_E_HIP, "tile sort: look-back timed out");
        C3DGS_TIMED_STAGE(ST_RANGES, p.debug, s, launch_identify_ranges(R, b.keys_sorted, b.key_bytes, img.ranges, sort_err, s)); // K8
    }
    // the tiles' compact lists (ids + quadrant masks of the entries that can reach their tile) go to the now idle sort scratch:
    // 5 R bytes, what the backward walks instead of the point list
    C3DGS_TIMED_STAGE(ST_RENDER_FWD, p.debug, s,
                      launch_render_forward(W, H, img, b.point_list, g.splat, p.background, out_color, compact_ptrs(b, R), sort_err, s)); // K9
    return C3DGS_OK;
}

static int backward_impl(const c3dgs_raster_params* pp, bool indexed, const int32_t* radii, const void* geom_buffer,
                         const void* binning_buffer, const void* image_buffer, int32_t R, const float* dL_dout_color,
                         c3dgs_resize_fn ws_resize, void* ws_user, const c3dgs_raster_grads* grads, void* stream_,
                         const float* dL_ddepth = nullptr, const float* dL_dalpha = nullptr,
                         const float* dL_ddistortion = nullptr, const float* moment = nullptr, float near_ = 0.f, float far_ = 0.f,
                         const float* dL_dnormal = nullptr, const float* normals = nullptr, const float* axes_rotations = nullptr,
                         const int64_t* axes_g_indices = nullptr, float* dL_daxes_rotations = nullptr)
{
    // gradients through the maps (render_maps_backward.hip: one blend replay for every map of the call): without a map, exactly
    // the plain backward below. Without the distortion map's gradient the other four distortion arguments are not looked at
    if (dL_ddistortion) {
        if (!moment) return fail(C3DGS_E_INVALID, "backward_distortion: moment is required with dL_ddistortion");
        if (!(far_ <= 0.f) && !(near_ > 0.f && near_ < far_))       // a NaN fails here as well
            return fail(C3DGS_E_INVALID, "backward_distortion: 0 < near < far is required (far <= 0 selects the raw mode)");
    }
    // With the normal map's gradient normal_backward_fold follows backward_preprocess; without it `normals` and the axes are not looked at. The fold chains to the
    // rotations the normals were made from: the call's own (and its dL_drotations), or, where the call blends a precomputed
    // covariance, which has no axes, the rotations given beside it, into a gradient tensor of their own that the caller has zeroed
    if (dL_dnormal) {
        if (!normals) return fail(C3DGS_E_INVALID, "backward_normal: normals is required with dL_dnormal");
        if (axes_rotations && !dL_daxes_rotations)
            return fail(C3DGS_E_INVALID, "backward_normal: dL_daxes_rotations is required with axes_rotations");
        if (pp && pp->cov3D_precomp && !axes_rotations)
            return fail(C3DGS_E_INVALID, "backward_normal: a precomputed covariance has no axes; axes_rotations is required beside it");
    }
    const bool maps = dL_ddepth != nullptr || dL_dalpha != nullptr || dL_ddistortion != nullptr || dL_dnormal != nullptr;
    if (int rc = validate(pp, indexed, true)) return rc;
    if (!grads) return fail(C3DGS_E_INVALID, "grads is NULL");
    c3dgs_raster_params p = *pp;
    if (!indexed) { p.sh_indices = nullptr; p.g_indices = nullptr; p.scale_factors = nullptr; }
    hipStream_t s = (hipStream_t)stream_;
    const int P = p.P, W = p.W, H = p.H;

    // codebook-sized outputs of the indexed variant are scatter-added: zero them here
    void* cb_zero = nullptr;           // one 16-byte aligned span of whole 16-byte words: cleared by the prep kernel below
    size_t cb_zero16 = 0;
    if (indexed) {
        const size_t n_sh = (grads->dL_dsh && p.sh) ? (size_t)p.SHS * p.M * 3 * sizeof(float) : 0;
        const size_t n_rot = (grads->dL_drotations && p.scales) ? (size_t)p.GS * 4 * sizeof(float) : 0;
        const size_t n_sc = (grads->dL_dscales && p.scales) ? (size_t)p.GS * 3 * sizeof(float) : 0;
        char* a_sh = (char*)grads->dL_dsh; char* a_rot = (char*)grads->dL_drotations; char* a_sc = (char*)grads->dL_dscales;
        if (n_sh && n_rot && n_sc && a_rot == a_sh + n_sh && a_sc == a_rot + n_rot) {
            // the three tensors are carved from one allocation (c3dgs_amd/rasterizer.py does that): one fill
            const size_t n = n_sh + n_rot + n_sc;
            if (p.P > 0 && R >= 0 && ((uintptr_t)a_sh & 15u) == 0) {
                cb_zero = a_sh; cb_zero16 = n / 16;
                if (n % 16) C3DGS_HIP_TRY(hipMemsetAsync(a_sh + cb_zero16 * 16, 0, n % 16, s));
            } else {
                C3DGS_HIP_TRY(hipMemsetAsync(a_sh, 0, n, s));
            }
        } else {
            if (n_sh) C3DGS_HIP_TRY(hipMemsetAsync(a_sh, 0, n_sh, s));
            if (n_sc) C3DGS_HIP_TRY(hipMemsetAsync(a_sc, 0, n_sc, s));
            if (n_rot) C3DGS_HIP_TRY(hipMemsetAsync(a_rot, 0, n_rot, s));
        }
    }
    if (P == 0) return C3DGS_OK;
    if (!radii || !geom_buffer || !image_buffer || (!dL_dout_color && !maps) || (R > 0 && !binning_buffer))
        return fail(C3DGS_E_INVALID, "radii, forward buffers and dL_dout_color are required");
    if (!ws_resize) return fail(C3DGS_E_INVALID, "workspace callback is required");
    if (R < 0) return fail(C3DGS_E_INVALID, "R must be >= 0");

    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    const ImgPtrs img = img_ptrs(const_cast<void*>(image_buffer), W, H);
    uint32_t* sort_err = maps ? onesweep_error_word() : nullptr;
    if (maps && !sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    // with maps: the same layout and, behind it, the dL/dz plane
    // with the normal map's gradient: behind that, the dn plane
    void* ws_base = ws_resize(ws_user, dL_dnormal ? normal_backward_layout(P, R).total_bytes
                                       : maps     ? depth_backward_layout(P, R).total_bytes
                                                  : c3dgs_backward_workspace_bytes(P, R));
    if (!ws_base) return fail(C3DGS_E_ALLOC, "backward workspace allocation failed");
    const BwdPtrs w = bwd_ptrs(ws_base, P, R);
    float* dz_plane = maps ? (float*)((char*)ws_base + depth_backward_layout(P, R).dz) : nullptr;
    NormalSlot* dn_plane = dL_dnormal ? (NormalSlot*)((char*)ws_base + normal_backward_layout(P, R).dn) : nullptr;
    // the colour blend launch: always without maps; with maps only where the loss uses the image
    const bool blend = R > 0 && dL_dout_color != nullptr;

    // only the 1-byte "written" flags are cleared (R bytes, not 36 R): the blend kernel never visits the instances
    // behind each tile's saturation point (73 % of them on the bench scene) and the per-Gaussian kernel skips them.
    // one launch: tile schedule of the blend kernel (img.tile_order: scratch of this call) + the flag clear. The codebook-gradient
    // clear (80 MB on the bench view, needed only by the per-Gaussian kernel's scatter-adds) rides in the blend kernel itself, a
    // slice per tile workgroup: that kernel is bound by vector issue and leaves the memory system idle (without a blend launch
    // the clear stays here)
    { StageTimer t_(ST_ZERO_PARTIALS, s);
      launch_backward_prep(blend ? W : 0, H, img, w.touched, w.touched_bytes / 16, blend ? nullptr : cb_zero, blend ? 0 : cb_zero16, s); }
    if (R > 0) {
        const CompactPtrs cl = compact_ptrs(bin_ptrs(const_cast<void*>(binning_buffer), R, W, H), R);
        if (blend)
            C3DGS_TIMED_STAGE(ST_RENDER_BWD, p.debug, s,
                              launch_render_backward(W, H, img, g.splat, g.block_base, p.background, dL_dout_color, w.partials, w.touched,
                                                     cl, cb_zero, cb_zero16, s)); // K10
        if (maps) {
            // one replay for every map of the call; the stage is named after the widest map it serves
            const int stage = dL_dnormal ? ST_RENDER_NORMAL_BWD : dL_ddistortion ? ST_RENDER_DISTORTION_BWD : ST_RENDER_DEPTH_BWD;
            C3DGS_TIMED_STAGE(stage, p.debug, s,
                              launch_render_maps_backward(W, H, img, cl, g, w, dz_plane, dn_plane, normals, dL_ddepth, dL_dalpha,
                                                          dL_dnormal, dL_ddistortion, moment, distortion_map(near_, far_), sort_err, s));
        }
    }
    C3DGS_TIMED_STAGE(ST_BWD_PREPROCESS, p.debug, s, launch_backward_preprocess(p, radii, g, w, *grads, s)); // K11 + K12(i)
    if (maps && R > 0 && grads->dL_dmeans3D)
        C3DGS_TIMED_STAGE(ST_DEPTH_BWD_FOLD, p.debug, s,
                          launch_depth_backward_fold(P, g, w, dz_plane, p.viewmatrix, grads->dL_dmeans3D, sort_err, s));
    if (dL_dnormal && R > 0 && axes_rotations)
        C3DGS_TIMED_STAGE(ST_NORMAL_BWD_FOLD, p.debug, s,
                          launch_normal_backward_fold(P, g, w, dn_plane, normals, axes_rotations, axes_g_indices, p.viewmatrix,
                                                      dL_daxes_rotations, sort_err, s));
    else if (dL_dnormal && R > 0 && grads->dL_drotations)
        C3DGS_TIMED_STAGE(ST_NORMAL_BWD_FOLD, p.debug, s,
                          launch_normal_backward_fold(P, g, w, dn_plane, normals, p.rotations, p.g_indices, p.viewmatrix,
                                                      grads->dL_drotations, sort_err, s));
    return C3DGS_OK;
}

} // namespace c3dgs

using namespace c3dgs;

extern "C" {

const char* c3dgs_last_error(void) { return g_last_error.c_str(); }

int c3dgs_profile_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return C3DGS_OK;
}

int c3dgs_profile_only(const char* stage_name)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_only = -1;
    if (!stage_name || !*stage_name) return C3DGS_OK;
    for (int i = 0; i < ST_COUNT; i++)
        if (std::strcmp(stage_name, kStageNames[i]) == 0) { g_prof_only = i; return C3DGS_OK; }
    return fail(C3DGS_E_INVALID, std::string("profile_only: unknown stage ") + stage_name);
}

int c3dgs_profile_read(c3dgs_stage_time* out, int capacity)
{
    std::vector<ProfRec> recs;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        recs.swap(g_prof_recs);
    }
    double total[ST_COUNT] = { 0 };
    long long count[ST_COUNT] = { 0 };
    for (auto& r : recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            total[r.stage] += (double)ms;
            count[r.stage]++;
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        for (auto& r : recs) { g_prof_pool.push_back(r.a); g_prof_pool.push_back(r.b); }
    }
    int n = 0;
    for (int i = 0; i < ST_COUNT && n < capacity; i++) {
        if (!count[i]) continue;
        std::memset(&out[n], 0, sizeof(out[n]));
        std::strncpy(out[n].name, kStageNames[i], sizeof(out[n].name) - 1);
        out[n].total_ms = total[i];
        out[n].count = count[i];
        n++;
    }
    return n;
}
int c3dgs_abi_version(void) { return C3DGS_ABI_VERSION; }

int c3dgs_get_geom_layout(int32_t P, c3dgs_geom_layout* out)
{
    if (!out || P < 0) return fail(C3DGS_E_INVALID, "bad arguments");
    geom_layout(P, out);
    return C3DGS_OK;
}
int c3dgs_get_binning_layout(int32_t R, int32_t W, int32_t H, c3dgs_binning_layout* out)
{
    if (!out || R < 0 || W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "bad arguments");
    binning_layout(R, W, H, out);
    return C3DGS_OK;
}
int c3dgs_get_image_layout(int32_t W, int32_t H, c3dgs_image_layout* out)
{
    if (!out || W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "bad arguments");
    ImageLayout L; image_layout(W, H, &L);
    *out = L;                                                        // the public fields
    return C3DGS_OK;
}
int c3dgs_get_compact_layout(int32_t R, int32_t W, int32_t H, c3dgs_compact_layout* out)
{
    if (!out || R < 0 || W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "bad arguments");
    c3dgs_binning_layout BL; binning_layout(R, W, H, &BL);
    const CompactBinLayout C = compact_bin_layout(R);
    ImageLayout IL; image_layout(W, H, &IL);
    out->cqm = BL.sort_temp + C.cqm; out->cid = BL.sort_temp + C.cid;
    out->tile_used_c = IL.tile_used_c; out->n_contrib_c = IL.n_contrib_c;
    return C3DGS_OK;
}
int c3dgs_get_backward_layout(int32_t P, int32_t R, c3dgs_backward_layout* out)
{
    if (!out || P < 0 || R < 0) return fail(C3DGS_E_INVALID, "bad arguments");
    backward_layout(P, R, out);
    return C3DGS_OK;
}
size_t c3dgs_backward_workspace_bytes(int32_t P, int32_t R)
{
    c3dgs_backward_layout L; backward_layout(P, R, &L);
    return L.total_bytes;
}

int c3dgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                       void* stream)
{
    (void)projmatrix; // the reference's in_frustum only tests view-space z (auxiliary.h:156)
    if (P < 0) return fail(C3DGS_E_INVALID, "P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!means3D || !viewmatrix || !present) return fail(C3DGS_E_INVALID, "means3D, viewmatrix and present are required");
    C3DGS_TIMED_STAGE(ST_MARK_VISIBLE, 0, (hipStream_t)stream, launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_mark_visible_pose(int32_t P, const float* means3D, const float* extrinsic_vector, uint8_t* present, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!means3D || !extrinsic_vector || !present) return fail(C3DGS_E_INVALID, "means3D, extrinsic_vector and present are required");
    C3DGS_TIMED_STAGE(ST_MARK_VISIBLE, 0, (hipStream_t)stream, launch_mark_visible_pose(P, means3D, extrinsic_vector, present, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_camera_from_pose(const float* extrinsic_vector, float inv_tan_half_fovx, float inv_tan_half_fovy, float* viewmatrix,
                           float* projmatrix, float* campos, void* stream)
{
    if (!extrinsic_vector || !viewmatrix || !projmatrix || !campos) return fail(C3DGS_E_INVALID, "camera_from_pose: NULL pointer");
    launch_camera_from_pose(extrinsic_vector, inv_tan_half_fovx, inv_tan_half_fovy, viewmatrix, projmatrix, campos, (hipStream_t)stream);
    C3DGS_STAGE("camera_from_pose", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_rasterize_gaussians(const c3dgs_raster_params* p, c3dgs_resize_fn geom_resize, void* geom_user,
                              c3dgs_resize_fn binning_resize, void* binning_user, c3dgs_resize_fn image_resize,
                              void* image_user, float* out_color, int32_t* radii, int32_t* num_rendered, void* stream)
{
    return forward_impl(p, false, geom_resize, geom_user, binning_resize, binning_user, image_resize, image_user, out_color,
                        radii, num_rendered, stream);
}

int c3dgs_rasterize_gaussians_indexed(const c3dgs_raster_params* p, c3dgs_resize_fn geom_resize, void* geom_user,
                                      c3dgs_resize_fn binning_resize, void* binning_user, c3dgs_resize_fn image_resize,
                                      void* image_user, float* out_color, int32_t* radii, int32_t* num_rendered, void* stream)
{
    return forward_impl(p, true, geom_resize, geom_user, binning_resize, binning_user, image_resize, image_user, out_color,
                        radii, num_rendered, stream);
}

int c3dgs_rasterize_gaussians_backward(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                       const void* binning_buffer, const void* image_buffer, int32_t R,
                                       const float* dL_dout_color, c3dgs_resize_fn workspace_resize, void* workspace_user,
                                       const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, false, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream);
}

int c3dgs_rasterize_gaussians_backward_indexed(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                               const void* binning_buffer, const void* image_buffer, int32_t R,
                                               const float* dL_dout_color, c3dgs_resize_fn workspace_resize,
                                               void* workspace_user, const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, true, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream);
}

int c3dgs_rasterize_gaussians_backward_depth(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                             const void* binning_buffer, const void* image_buffer, int32_t R,
                                             const float* dL_dout_color, const float* dL_ddepth, const float* dL_dalpha,
                                             c3dgs_resize_fn workspace_resize, void* workspace_user,
                                             const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, false, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream, dL_ddepth, dL_dalpha);
}

int c3dgs_rasterize_gaussians_backward_depth_indexed(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                                     const void* binning_buffer, const void* image_buffer, int32_t R,
                                                     const float* dL_dout_color, const float* dL_ddepth, const float* dL_dalpha,
                                                     c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                     const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, true, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream, dL_ddepth, dL_dalpha);
}

size_t c3dgs_depth_backward_workspace_bytes(int32_t P, int32_t R) { return depth_backward_layout(P, R).total_bytes; }

int c3dgs_rasterize_gaussians_backward_distortion(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                                  const void* binning_buffer, const void* image_buffer, int32_t R,
                                                  const float* dL_dout_color, const float* dL_ddepth, const float* dL_dalpha,
                                                  const float* dL_ddistortion, const float* moment, float near_, float far_,
                                                  c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                  const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, false, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream, dL_ddepth, dL_dalpha, dL_ddistortion, moment, near_, far_);
}

int c3dgs_rasterize_gaussians_backward_distortion_indexed(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                                          const void* binning_buffer, const void* image_buffer, int32_t R,
                                                          const float* dL_dout_color, const float* dL_ddepth, const float* dL_dalpha,
                                                          const float* dL_ddistortion, const float* moment, float near_, float far_,
                                                          c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                          const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, true, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream, dL_ddepth, dL_dalpha, dL_ddistortion, moment, near_, far_);
}

size_t c3dgs_distortion_backward_workspace_bytes(int32_t P, int32_t R) { return depth_backward_layout(P, R).total_bytes; }

int c3dgs_rasterize_gaussians_backward_normal(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                              const void* binning_buffer, const void* image_buffer, int32_t R,
                                              const float* dL_dout_color, const float* dL_ddepth, const float* dL_dalpha,
                                              const float* dL_dnormal, const float* normals, const float* axes_rotations,
                                              const int64_t* axes_g_indices, float* dL_daxes_rotations, const float* dL_ddistortion,
                                              const float* moment, float near_, float far_, c3dgs_resize_fn workspace_resize,
                                              void* workspace_user, const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, false, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream, dL_ddepth, dL_dalpha, dL_ddistortion, moment, near_, far_, dL_dnormal, normals,
                         axes_rotations, axes_g_indices, dL_daxes_rotations);
}

int c3dgs_rasterize_gaussians_backward_normal_indexed(const c3dgs_raster_params* p, const int32_t* radii, const void* geom_buffer,
                                                      const void* binning_buffer, const void* image_buffer, int32_t R,
                                                      const float* dL_dout_color, const float* dL_ddepth, const float* dL_dalpha,
                                                      const float* dL_dnormal, const float* normals, const float* axes_rotations,
                                                      const int64_t* axes_g_indices, float* dL_daxes_rotations,
                                                      const float* dL_ddistortion, const float* moment, float near_, float far_,
                                                      c3dgs_resize_fn workspace_resize, void* workspace_user,
                                                      const c3dgs_raster_grads* grads, void* stream)
{
    return backward_impl(p, true, radii, geom_buffer, binning_buffer, image_buffer, R, dL_dout_color, workspace_resize,
                         workspace_user, grads, stream, dL_ddepth, dL_dalpha, dL_ddistortion, moment, near_, far_, dL_dnormal, normals,
                         axes_rotations, axes_g_indices, dL_daxes_rotations);
}

size_t c3dgs_normal_backward_workspace_bytes(int32_t P, int32_t R) { return normal_backward_layout(P, R).total_bytes; }

int c3dgs_gaussian_normals(int32_t P, const float* means3D, const float* scales, const float* rotations, const int64_t* g_indices,
                           const float* viewmatrix, float* out_normals, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "gaussian_normals: P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!means3D || !scales || !rotations || !viewmatrix || !out_normals)
        return fail(C3DGS_E_INVALID, "gaussian_normals: means3D, scales, rotations, viewmatrix and out_normals are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_GAUSSIAN_NORMALS, 0, s,
                      launch_gaussian_normals(P, means3D, scales, rotations, g_indices, viewmatrix, out_normals, s));
    return C3DGS_OK;
}

int c3dgs_render_normal(int32_t P, int32_t W, int32_t H, int32_t R, const void* geom_buffer, const void* binning_buffer,
                        const void* image_buffer, const float* normals, float* out_normal, void* stream)
{
    if (W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "render_normal: W and H must be positive");
    if (P < 0 || R < 0) return fail(C3DGS_E_INVALID, "render_normal: P and R must be >= 0");
    if (!out_normal) return fail(C3DGS_E_INVALID, "render_normal: out_normal is required");
    if (R > 0 && P == 0) return fail(C3DGS_E_INVALID, "render_normal: R > 0 instances cannot come from P = 0");
    if (R > 0 && (!geom_buffer || !binning_buffer || !image_buffer || !normals))
        return fail(C3DGS_E_INVALID, "render_normal: the forward's geometry, binning and image buffers and the normals are required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || R == 0) {            // nothing was blended anywhere
        C3DGS_HIP_TRY(hipMemsetAsync(out_normal, 0, (size_t)3 * W * H * sizeof(float), s));
        return C3DGS_OK;
    }
    uint32_t* sort_err = onesweep_error_word();
    if (!sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    const ImgPtrs img = img_ptrs(const_cast<void*>(image_buffer), W, H);
    const BinPtrs b = bin_ptrs(const_cast<void*>(binning_buffer), R, W, H);
    C3DGS_TIMED_STAGE(ST_RENDER_NORMAL, 0, s,
                      launch_render_normal(W, H, img, compact_ptrs(b, R), g.splat, normals, out_normal, sort_err, s));
    return C3DGS_OK;
}

static int stencil_args(const char* who, int32_t W, int32_t H, float tan_fovx, float tan_fovy)
{
    if (W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, std::string(who) + ": W and H must be positive");
    if (!(tan_fovx > 0.f) || !(tan_fovy > 0.f)) return fail(C3DGS_E_INVALID, std::string(who) + ": tan_fovx and tan_fovy must be positive");
    return C3DGS_OK;
}

int c3dgs_depth_to_normal(int32_t W, int32_t H, const float* z, float tan_fovx, float tan_fovy, float* out_normal, void* stream)
{
    if (int rc = stencil_args("depth_to_normal", W, H, tan_fovx, tan_fovy)) return rc;
    if (!z || !out_normal) return fail(C3DGS_E_INVALID, "depth_to_normal: z and out_normal are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_DEPTH_TO_NORMAL, 0, s, launch_depth_to_normal(W, H, z, tan_fovx, tan_fovy, out_normal, s));
    return C3DGS_OK;
}

int c3dgs_depth_to_normal_backward(int32_t W, int32_t H, const float* z, const float* dL_dnormal, float tan_fovx, float tan_fovy,
                                   float* dL_dz, void* stream)
{
    if (int rc = stencil_args("depth_to_normal_backward", W, H, tan_fovx, tan_fovy)) return rc;
    if (!z || !dL_dnormal || !dL_dz) return fail(C3DGS_E_INVALID, "depth_to_normal_backward: z, dL_dnormal and dL_dz are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_DEPTH_TO_NORMAL_BWD, 0, s,
                      launch_depth_to_normal_backward(W, H, z, dL_dnormal, tan_fovx, tan_fovy, dL_dz, s));
    return C3DGS_OK;
}

int c3dgs_render_distortion(int32_t P, int32_t W, int32_t H, int32_t R, const void* geom_buffer, const void* binning_buffer,
                            const void* image_buffer, float near_, float far_, float* out_distortion, float* out_moment, void* stream)
{
    if (W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "render_distortion: W and H must be positive");
    if (P < 0 || R < 0) return fail(C3DGS_E_INVALID, "render_distortion: P and R must be >= 0");
    if (!out_distortion) return fail(C3DGS_E_INVALID, "render_distortion: out_distortion is required");
    if (!(far_ <= 0.f) && !(near_ > 0.f && near_ < far_))
        return fail(C3DGS_E_INVALID, "render_distortion: 0 < near < far is required (far <= 0 selects the raw mode)");
    if (R > 0 && P == 0) return fail(C3DGS_E_INVALID, "render_distortion: R > 0 instances cannot come from P = 0");
    if (R > 0 && (!geom_buffer || !binning_buffer || !image_buffer))
        return fail(C3DGS_E_INVALID, "render_distortion: the forward's geometry, binning and image buffers are required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || R == 0) {            // nothing was blended anywhere
        const size_t bytes = (size_t)W * H * sizeof(float);
        for (float* o : { out_distortion, out_moment })
            if (o) C3DGS_HIP_TRY(hipMemsetAsync(o, 0, bytes, s));
        return C3DGS_OK;
    }
    uint32_t* sort_err = onesweep_error_word();
    if (!sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    const ImgPtrs img = img_ptrs(const_cast<void*>(image_buffer), W, H);
    const BinPtrs b = bin_ptrs(const_cast<void*>(binning_buffer), R, W, H);
    C3DGS_TIMED_STAGE(ST_RENDER_DISTORTION, 0, s,
                      launch_render_distortion(W, H, img, compact_ptrs(b, R), g.splat, g.depth_keys, distortion_map(near_, far_),
                                               out_distortion, out_moment, sort_err, s));
    return C3DGS_OK;
}

int c3dgs_render_depth(int32_t P, int32_t W, int32_t H, int32_t R, const void* geom_buffer, const void* binning_buffer,
                       const void* image_buffer, float* out_depth, float* out_alpha, float* out_median, void* stream)
{
    if (W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "render_depth: W and H must be positive");
    if (P < 0 || R < 0) return fail(C3DGS_E_INVALID, "render_depth: P and R must be >= 0");
    if (!out_depth && !out_alpha && !out_median) return fail(C3DGS_E_INVALID, "render_depth: at least one output is required");
    if (R > 0 && P == 0) return fail(C3DGS_E_INVALID, "render_depth: R > 0 instances cannot come from P = 0");
    if (R > 0 && (!geom_buffer || !binning_buffer || !image_buffer))
        return fail(C3DGS_E_INVALID, "render_depth: the forward's geometry, binning and image buffers are required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || R == 0) {            // nothing was blended anywhere: T stays 1
        const size_t bytes = (size_t)W * H * sizeof(float);
        for (float* o : { out_depth, out_alpha, out_median })
            if (o) C3DGS_HIP_TRY(hipMemsetAsync(o, 0, bytes, s));
        return C3DGS_OK;
    }
    uint32_t* sort_err = onesweep_error_word();
    if (!sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    const ImgPtrs img = img_ptrs(const_cast<void*>(image_buffer), W, H);
    const BinPtrs b = bin_ptrs(const_cast<void*>(binning_buffer), R, W, H);
    C3DGS_TIMED_STAGE(ST_RENDER_DEPTH, 0, s,
                      launch_render_depth(W, H, img, compact_ptrs(b, R), g.splat, g.depth_keys, out_depth, out_alpha, out_median,
                                          sort_err, s));
    return C3DGS_OK;
}

size_t c3dgs_contrib_workspace_bytes(int32_t P, int32_t R) { return contrib_layout(P, R).total_bytes; }

int c3dgs_render_contrib(int32_t P, int32_t W, int32_t H, int32_t R, const void* geom_buffer, const void* binning_buffer,
                         const void* image_buffer, void* workspace, float* out_weight_sum, float* out_weight_max,
                         uint32_t* out_hits, void* stream)
{
    if (W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "render_contrib: W and H must be positive");
    if (P < 0 || R < 0) return fail(C3DGS_E_INVALID, "render_contrib: P and R must be >= 0");
    if (!out_weight_sum && !out_weight_max && !out_hits) return fail(C3DGS_E_INVALID, "render_contrib: at least one output is required");
    if (R > 0 && P == 0) return fail(C3DGS_E_INVALID, "render_contrib: R > 0 instances cannot come from P = 0");
    if (R > 0 && (!geom_buffer || !binning_buffer || !image_buffer || !workspace))
        return fail(C3DGS_E_INVALID, "render_contrib: the forward's geometry, binning and image buffers and a workspace are required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || R == 0) {            // nothing was blended anywhere
        if (P > 0) {
            if (out_weight_sum) C3DGS_HIP_TRY(hipMemsetAsync(out_weight_sum, 0, (size_t)P * sizeof(float), s));
            if (out_weight_max) C3DGS_HIP_TRY(hipMemsetAsync(out_weight_max, 0, (size_t)P * sizeof(float), s));
            if (out_hits) C3DGS_HIP_TRY(hipMemsetAsync(out_hits, 0, (size_t)P * sizeof(uint32_t), s));
        }
        return C3DGS_OK;
    }
    uint32_t* sort_err = onesweep_error_word();
    if (!sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    const ImgPtrs img = img_ptrs(const_cast<void*>(image_buffer), W, H);
    const BinPtrs b = bin_ptrs(const_cast<void*>(binning_buffer), R, W, H);
    const ContribPtrs w = contrib_ptrs(workspace, P, R);
    {
        StageTimer t_(ST_RENDER_CONTRIB, s);
        // only the 1-byte "written" flags are cleared, by the fill workgroups of the backward's prep kernel (no tiles: nothing is
        // ordered, img.tile_order stays as it is)
        launch_backward_prep(0, H, img, w.touched, w.touched_bytes / 16, nullptr, 0, s);
        { StageTimer a_(ST_RENDER_CONTRIB_BLEND, s); launch_render_contrib(W, H, img, compact_ptrs(b, R), g, w, sort_err, s); }
        { StageTimer b_(ST_RENDER_CONTRIB_SUM, s); launch_contrib_sum(P, g, w, out_weight_sum, out_weight_max, out_hits, sort_err, s); }
    }
    C3DGS_STAGE_CHECK(ST_RENDER_CONTRIB, 0, s);
    return C3DGS_OK;
}

int c3dgs_contrib_accumulate(int32_t P_model, int32_t P_rows, const uint8_t* visible, const int32_t* rank, const float* weight_sum,
                             const float* weight_max, const uint32_t* hits, float* acc_sum, float* acc_max, int64_t* acc_hits,
                             uint32_t* acc_views, void* stream)
{
    if (P_model < 0 || P_rows < 0) return fail(C3DGS_E_INVALID, "contrib_accumulate: P_model and P_rows must be >= 0");
    if ((visible == nullptr) != (rank == nullptr)) return fail(C3DGS_E_INVALID, "contrib_accumulate: visible and rank come as a pair");
    if (!visible && P_rows != P_model) return fail(C3DGS_E_INVALID, "contrib_accumulate: without visible / rank the rows are the model's");
    if (P_model == 0 || P_rows == 0) return C3DGS_OK;
    if (!weight_sum || !weight_max || !hits || !acc_sum || !acc_max || !acc_hits || !acc_views)
        return fail(C3DGS_E_INVALID, "contrib_accumulate: the three rows and the four accumulators are required");
    launch_contrib_accumulate(P_model, P_rows, visible, rank, weight_sum, weight_max, hits, acc_sum, acc_max, acc_hits, acc_views,
                              (hipStream_t)stream);
    C3DGS_STAGE("contrib_accumulate", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

size_t c3dgs_error_workspace_bytes(int32_t P, int32_t R) { return error_layout(P, R).total_bytes; }

int c3dgs_render_error(int32_t P, int32_t W, int32_t H, int32_t R, const void* geom_buffer, const void* binning_buffer,
                       const void* image_buffer, void* workspace, const float* pixel_map, float* out_err_sum, void* stream)
{
    if (W <= 0 || H <= 0) return fail(C3DGS_E_INVALID, "render_error: W and H must be positive");
    if (P < 0 || R < 0) return fail(C3DGS_E_INVALID, "render_error: P and R must be >= 0");
    if (!out_err_sum) return fail(C3DGS_E_INVALID, "render_error: the output is required");
    if (!pixel_map) return fail(C3DGS_E_INVALID, "render_error: the pixel map is required");
    if (R > 0 && P == 0) return fail(C3DGS_E_INVALID, "render_error: R > 0 instances cannot come from P = 0");
    if (R > 0 && (!geom_buffer || !binning_buffer || !image_buffer || !workspace))
        return fail(C3DGS_E_INVALID, "render_error: the forward's geometry, binning and image buffers and a workspace are required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || R == 0) {            // nothing was blended anywhere
        if (P > 0) C3DGS_HIP_TRY(hipMemsetAsync(out_err_sum, 0, (size_t)P * sizeof(float), s));
        return C3DGS_OK;
    }
    uint32_t* sort_err = onesweep_error_word();
    if (!sort_err) return fail(C3DGS_E_HIP, "cannot resolve the sort error word");
    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    const ImgPtrs img = img_ptrs(const_cast<void*>(image_buffer), W, H);
    const BinPtrs b = bin_ptrs(const_cast<void*>(binning_buffer), R, W, H);
    const ErrorPtrs w = error_ptrs(workspace, P, R);
    {
        StageTimer t_(ST_RENDER_ERROR, s);
        // only the 1-byte "written" flags are cleared, as c3dgs_render_contrib clears its own
        launch_backward_prep(0, H, img, w.touched, w.touched_bytes / 16, nullptr, 0, s);
        { StageTimer a_(ST_RENDER_ERROR_BLEND, s); launch_render_error(W, H, img, compact_ptrs(b, R), g, w, pixel_map, sort_err, s); }
        { StageTimer b_(ST_RENDER_ERROR_SUM, s); launch_error_sum(P, g, w, out_err_sum, sort_err, s); }
    }
    C3DGS_STAGE_CHECK(ST_RENDER_ERROR, 0, s);
    return C3DGS_OK;
}

size_t c3dgs_pose_grad_workspace_bytes(int32_t P) { return pose_grad_workspace_bytes(P); }

int c3dgs_pose_grad(int32_t P, int32_t D, int32_t M, float scale_modifier, const float* means3D, const float* dL_dmeans3D,
                    const float* dL_dcov3D, const float* dL_dcolors, const float* sh, const int64_t* sh_indices,
                    const float* cov3D_precomp, const float* scales, const float* rotations, const float* scale_factors,
                    const int64_t* g_indices, const void* geom_buffer, const int32_t* radii, const float* pose, void* workspace,
                    float* out, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "pose_grad: P must be >= 0");
    if (D < 0 || D > 3 || M < 0) return fail(C3DGS_E_INVALID, "pose_grad: the SH degree must be 0..3 and M >= 0");
    if (!pose || !out) return fail(C3DGS_E_INVALID, "pose_grad: the pose and the output are required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {                      // nothing to sum
        C3DGS_HIP_TRY(hipMemsetAsync(out, 0, 7 * sizeof(float), s));
        return C3DGS_OK;
    }
    if (!means3D || !dL_dmeans3D || !dL_dcov3D || !radii)
        return fail(C3DGS_E_INVALID, "pose_grad: means3D, dL_dmeans3D, dL_dcov3D and radii are required");
    if (!geom_buffer || !workspace) return fail(C3DGS_E_INVALID, "pose_grad: the forward's geometry buffer and a workspace are required");
    if ((scales == nullptr) != (rotations == nullptr)) return fail(C3DGS_E_INVALID, "pose_grad: scales and rotations come as a pair");
    if ((cov3D_precomp != nullptr) == (scales != nullptr))
        return fail(C3DGS_E_INVALID, "pose_grad: exactly one of cov3D_precomp and the scale / rotation pair is required");
    if ((g_indices == nullptr) != (scale_factors == nullptr))
        return fail(C3DGS_E_INVALID, "pose_grad: g_indices and scale_factors come as a pair");
    if (g_indices && !scales) return fail(C3DGS_E_INVALID, "pose_grad: g_indices need the scale / rotation codebooks");
    if (sh_indices && !sh) return fail(C3DGS_E_INVALID, "pose_grad: sh_indices need sh");
    if (sh && !dL_dcolors) return fail(C3DGS_E_INVALID, "pose_grad: with sh, dL_dcolors is required");
    if (sh && M < (D + 1) * (D + 1)) return fail(C3DGS_E_INVALID, "pose_grad: M must hold the (D + 1)^2 coefficients of degree D");
    const GeomPtrs g = geom_ptrs(const_cast<void*>(geom_buffer), P);
    PoseGradIn in;
    in.P = P; in.D = D; in.M = M; in.scale_modifier = scale_modifier;
    in.means3D = means3D; in.dL_dmeans3D = dL_dmeans3D; in.dL_dcov3D = dL_dcov3D; in.dL_dcolors = dL_dcolors;
    in.sh = sh; in.sh_indices = sh_indices; in.cov3D_precomp = cov3D_precomp; in.scales = scales; in.rotations = rotations;
    in.scale_factors = scale_factors; in.g_indices = g_indices; in.clamped = g.clamped; in.radii = radii; in.pose = pose;
    {
        StageTimer t_(ST_POSE_GRAD, s);
        { StageTimer a_(ST_POSE_GRAD_SUMS, s); launch_pose_sums(in, (float*)workspace, s); }
        { StageTimer b_(ST_POSE_GRAD_FOLD, s); launch_pose_fold(P, (const float*)workspace, pose, out, s); }
    }
    C3DGS_STAGE_CHECK(ST_POSE_GRAD, 0, s);
    return C3DGS_OK;
}

// what c3dgs_aa_opacity and c3dgs_aa_opacity_backward both ask of the params: the per-Gaussian projection's inputs
static int aa_validate(const char* who, const c3dgs_raster_params* p)
{
    const std::string w(who);
    if (!p) return fail(C3DGS_E_INVALID, w + ": params is NULL");
    if (p->P < 0) return fail(C3DGS_E_INVALID, w + ": P must be >= 0");
    const bool has_sr = p->scales != nullptr && p->rotations != nullptr;
    if ((p->scales != nullptr) != (p->rotations != nullptr) || has_sr == (p->cov3D_precomp != nullptr))
        return fail(C3DGS_E_INVALID, w + ": exactly one of the scale / rotation pair and cov3D_precomp is required");
    if (p->g_indices && !p->scale_factors) return fail(C3DGS_E_INVALID, w + ": g_indices need scale_factors");
    if (p->P == 0) return C3DGS_OK;
    if (p->W <= 0 || p->H <= 0) return fail(C3DGS_E_INVALID, w + ": W and H must be positive");
    if (!p->means3D || !p->opacities || !p->viewmatrix)
        return fail(C3DGS_E_INVALID, w + ": means3D, opacities (the raw ones) and viewmatrix are required");
    return C3DGS_OK;
}

int c3dgs_aa_opacity(const c3dgs_raster_params* p, float* opacity_out, float* rho, void* stream)
{
    if (int rc = aa_validate("aa_opacity", p)) return rc;
    if (!opacity_out) return fail(C3DGS_E_INVALID, "aa_opacity: opacity_out is required");
    if (p->P == 0) return C3DGS_OK;
    C3DGS_TIMED_STAGE(ST_AA_OPACITY, p->debug, (hipStream_t)stream, launch_aa_opacity(*p, opacity_out, rho, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_aa_opacity_backward(const c3dgs_raster_params* p, const int32_t* radii, const c3dgs_raster_grads* grads, void* stream)
{
    if (int rc = aa_validate("aa_opacity_backward", p)) return rc;
    if (!grads) return fail(C3DGS_E_INVALID, "aa_opacity_backward: grads is NULL");
    if (!grads->dL_dopacity) return fail(C3DGS_E_INVALID, "aa_opacity_backward: grads->dL_dopacity is required");
    if (p->cov3D_precomp && !grads->dL_dcov3D)
        return fail(C3DGS_E_INVALID, "aa_opacity_backward: with cov3D_precomp, grads->dL_dcov3D is required");
    if (p->P == 0) return C3DGS_OK;
    if (!radii) return fail(C3DGS_E_INVALID, "aa_opacity_backward: radii is required");
    C3DGS_TIMED_STAGE(ST_AA_OPACITY_BWD, p->debug, (hipStream_t)stream,
                      launch_aa_opacity_backward(*p, radii, *grads, (hipStream_t)stream));
    return C3DGS_OK;
}

size_t c3dgs_filter3d_workspace_bytes(int32_t) { return 256; }    // {bits of the largest seen dist, bits of the focal}

int c3dgs_filter3d_compute(int32_t P, int32_t C, const float* xyz, const float* cameras, float* filter_3D, uint8_t* seen,
                           void* workspace, size_t workspace_bytes, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "filter3d_compute: P must be >= 0");
    if (C <= 0) return fail(C3DGS_E_INVALID, "filter3d_compute: C must be positive (a filter needs at least one camera)");
    if (P == 0) return C3DGS_OK;
    if (!xyz || !cameras || !filter_3D) return fail(C3DGS_E_INVALID, "filter3d_compute: xyz, cameras and filter_3D are required");
    if (!workspace || workspace_bytes < c3dgs_filter3d_workspace_bytes(P) || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return fail(C3DGS_E_INVALID, "filter3d_compute: workspace must hold c3dgs_filter3d_workspace_bytes(P) bytes, 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    {
        StageTimer t_(ST_FILTER3D_COMPUTE, s);
        hipError_t e = hipMemsetAsync(workspace, 0, 8, s);
        if (e != hipSuccess) return fail(C3DGS_E_HIP, std::string("filter3d_compute: hipMemsetAsync: ") + hipGetErrorString(e));
        launch_filter3d_dist(P, C, xyz, cameras, filter_3D, (uint32_t*)workspace, s);
        launch_filter3d_finish(P, (const uint32_t*)workspace, filter_3D, seen, s);
    }
    C3DGS_STAGE_CHECK(ST_FILTER3D_COMPUTE, 0, s);
    return C3DGS_OK;
}

// what c3dgs_filter3d_apply and c3dgs_filter3d_apply_backward both ask of the rows
static int filter3d_validate(const char* who, const c3dgs_filter3d_rows* r)
{
    const std::string w(who);
    if (!r) return fail(C3DGS_E_INVALID, w + ": rows is NULL");
    if (r->n < 0) return fail(C3DGS_E_INVALID, w + ": n must be >= 0");
    if (r->g_indices && !r->scale_factors) return fail(C3DGS_E_INVALID, w + ": g_indices need scale_factors");
    if (r->visible && (!r->rank || r->P_model < 0)) return fail(C3DGS_E_INVALID, w + ": visible needs rank and P_model >= 0");
    if (r->n == 0) return C3DGS_OK;
    if (!r->opacities || !r->scales || !r->filter_3D || (!r->rotations && !r->cov3D_precomp))
        return fail(C3DGS_E_INVALID, w + ": opacities, scales, rotations (unless cov3D_precomp is given) and filter_3D are required");
    if (reinterpret_cast<uintptr_t>(r->rotations) & 15u)
        return fail(C3DGS_E_INVALID, w + ": rotations must be 16-byte aligned");
    return C3DGS_OK;
}

int c3dgs_filter3d_apply(const c3dgs_filter3d_rows* r, float* cov3D_out, float* opacity_out, void* stream)
{
    if (int rc = filter3d_validate("filter3d_apply", r)) return rc;
    if (r->n == 0) return C3DGS_OK;
    if (!cov3D_out || !opacity_out) return fail(C3DGS_E_INVALID, "filter3d_apply: cov3D_out and opacity_out are required");
    C3DGS_TIMED_STAGE(ST_FILTER3D_APPLY, 0, (hipStream_t)stream, launch_filter3d_apply(*r, cov3D_out, opacity_out, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_filter3d_apply_backward(const c3dgs_filter3d_rows* r, const c3dgs_filter3d_grads* g, void* stream)
{
    if (int rc = filter3d_validate("filter3d_apply_backward", r)) return rc;
    if (!g) return fail(C3DGS_E_INVALID, "filter3d_apply_backward: grads is NULL");
    if (r->n == 0) return C3DGS_OK;
    if (!g->dL_dopacity && !g->dL_dscales && !g->dL_drotations && !g->dL_dscale_factors)
        return fail(C3DGS_E_INVALID, "filter3d_apply_backward: at least one output gradient is required");
    if (reinterpret_cast<uintptr_t>(g->dL_drotations) & 15u)
        return fail(C3DGS_E_INVALID, "filter3d_apply_backward: dL_drotations must be 16-byte aligned");
    C3DGS_TIMED_STAGE(ST_FILTER3D_APPLY_BWD, 0, (hipStream_t)stream, launch_filter3d_apply_backward(*r, *g, (hipStream_t)stream));
    return C3DGS_OK;
}

// what every mesh entry asks of the lattice and the two planes
static int mesh_validate(const char* who, const c3dgs_lattice* l, const float* tsdf, const float* weight)
{
    const std::string w(who);
    if (!l) return fail(C3DGS_E_INVALID, w + ": lattice is NULL");
    if (l->Nx < 1 || l->Ny < 1 || l->Nz < 1) return fail(C3DGS_E_INVALID, w + ": Nx, Ny and Nz must be positive");
    if ((uint64_t)l->Nx * (uint64_t)l->Ny > (uint64_t)INT32_MAX || (uint64_t)l->Nx * (uint64_t)l->Ny * (uint64_t)l->Nz > (uint64_t)INT32_MAX)
        return fail(C3DGS_E_INVALID, w + ": Nx Ny Nz must be at most 2^31 - 1");
    if (!(l->voxel_size > 0.f)) return fail(C3DGS_E_INVALID, w + ": voxel_size must be positive");
    if (!tsdf || !weight) return fail(C3DGS_E_INVALID, w + ": the tsdf and weight planes are required");
    return C3DGS_OK;
}

static int mesh_workspace(const char* who, const c3dgs_lattice* l, const void* workspace, size_t workspace_bytes)
{
    if (!workspace || workspace_bytes < mesh_extract_workspace_bytes(l->Nx, l->Ny, l->Nz) || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(C3DGS_E_INVALID, std::string(who) + ": workspace must hold c3dgs_mesh_extract_workspace_bytes(Nx, Ny, Nz) bytes, "
                                                        "256-byte aligned");
    return C3DGS_OK;
}

int c3dgs_tsdf_integrate(const c3dgs_lattice* l, int32_t K, int32_t W, int32_t H, const float* depth, const float* color,
                         const float* cameras, float sdf_trunc, float depth_min, float depth_max, float* tsdf, float* weight,
                         float* vol_color, void* stream)
{
    if (int rc = mesh_validate("tsdf_integrate", l, tsdf, weight)) return rc;
    if (K < 1) return fail(C3DGS_E_INVALID, "tsdf_integrate: K must be at least 1");
    if (W < 1 || H < 1) return fail(C3DGS_E_INVALID, "tsdf_integrate: W and H must be positive");
    if (!(sdf_trunc > 0.f)) return fail(C3DGS_E_INVALID, "tsdf_integrate: sdf_trunc must be positive");
    if (!(depth_min < depth_max)) return fail(C3DGS_E_INVALID, "tsdf_integrate: depth_min < depth_max is required");
    if (!depth || !cameras) return fail(C3DGS_E_INVALID, "tsdf_integrate: depth and cameras are required");
    if ((color != nullptr) != (vol_color != nullptr))
        return fail(C3DGS_E_INVALID, "tsdf_integrate: color and vol_color come as a pair");
    C3DGS_TIMED_STAGE(ST_TSDF_INTEGRATE, 0, (hipStream_t)stream,
                      launch_tsdf_integrate(*l, K, W, H, depth, color, cameras, sdf_trunc, depth_min, depth_max, tsdf, weight, vol_color,
                                            (hipStream_t)stream));
    return C3DGS_OK;
}

size_t c3dgs_mesh_extract_workspace_bytes(int32_t Nx, int32_t Ny, int32_t Nz)
{
    if (Nx < 1 || Ny < 1 || Nz < 1 || (uint64_t)Nx * (uint64_t)Ny > (uint64_t)INT32_MAX ||
        (uint64_t)Nx * (uint64_t)Ny * (uint64_t)Nz > (uint64_t)INT32_MAX) return 0;
    return mesh_extract_workspace_bytes(Nx, Ny, Nz);
}

int c3dgs_mesh_extract_count(const c3dgs_lattice* l, const float* tsdf, const float* weight, void* workspace, size_t workspace_bytes,
                             int64_t* counts, void* stream)
{
    if (int rc = mesh_validate("mesh_extract_count", l, tsdf, weight)) return rc;
    if (int rc = mesh_workspace("mesh_extract_count", l, workspace, workspace_bytes)) return rc;
    if (!counts) return fail(C3DGS_E_INVALID, "mesh_extract_count: counts is NULL");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_MESH_CLASSIFY, 0, s, launch_mesh_classify(*l, tsdf, weight, workspace, s));
    const uint32_t* totals = nullptr;
    C3DGS_TIMED_STAGE(ST_MESH_SCAN, 0, s, totals = launch_mesh_scan(*l, workspace, s));
    uint32_t host[2] = { 0u, 0u };
    C3DGS_HIP_TRY(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, s));
    C3DGS_HIP_TRY(hipStreamSynchronize(s));
    if (host[0] > (uint32_t)INT32_MAX || host[1] > (uint32_t)INT32_MAX)
        return fail(C3DGS_E_INVALID, "mesh_extract_count: more than 2^31 - 1 vertices or faces; extract a coarser or smaller volume");
    counts[0] = host[0]; counts[1] = host[1];
    return C3DGS_OK;
}

int c3dgs_mesh_extract_emit(const c3dgs_lattice* l, const float* tsdf, const float* weight, const float* vol_color, void* workspace,
                            size_t workspace_bytes, int64_t V, int64_t F, float* vertices, float* colors, int32_t* faces, void* stream)
{
    if (int rc = mesh_validate("mesh_extract_emit", l, tsdf, weight)) return rc;
    if (int rc = mesh_workspace("mesh_extract_emit", l, workspace, workspace_bytes)) return rc;
    if (V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX) return fail(C3DGS_E_INVALID, "mesh_extract_emit: V and F must be in [0, 2^31 - 1]");
    if (V == 0) return C3DGS_OK;                            // no vertex, no face: the outputs are empty, whatever their pointers
    if ((vol_color != nullptr) != (colors != nullptr))
        return fail(C3DGS_E_INVALID, "mesh_extract_emit: vol_color and colors come as a pair");
    if (!vertices || (F > 0 && !faces)) return fail(C3DGS_E_INVALID, "mesh_extract_emit: vertices and faces are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_MESH_EMIT_VERTICES, 0, s, launch_mesh_vertices(*l, tsdf, vol_color, workspace, (uint32_t)V, vertices, colors, s));
    if (F > 0) C3DGS_TIMED_STAGE(ST_MESH_EMIT_FACES, 0, s, launch_mesh_faces(*l, tsdf, workspace, (uint32_t)F, faces, s));
    return C3DGS_OK;
}

int c3dgs_error_map_l1(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, float* out, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0) return fail(C3DGS_E_INVALID, "error_map_l1: C, H and W must be positive");
    if (!img || !gt || !out) return fail(C3DGS_E_INVALID, "error_map_l1: both images and the output are required");
    {
        StageTimer t_(ST_ERROR_MAP_L1, (hipStream_t)stream);
        launch_error_map_l1(C, H, W, img, gt, out, (hipStream_t)stream);
    }
    C3DGS_STAGE_CHECK(ST_ERROR_MAP_L1, 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_error_accumulate(int32_t P_model, int32_t P_rows, const uint8_t* visible, const int32_t* rank, const float* err_sum,
                           float* acc_max, float* acc_sum, void* stream)
{
    if (P_model < 0 || P_rows < 0) return fail(C3DGS_E_INVALID, "error_accumulate: P_model and P_rows must be >= 0");
    if ((visible == nullptr) != (rank == nullptr)) return fail(C3DGS_E_INVALID, "error_accumulate: visible and rank come as a pair");
    if (!visible && P_rows != P_model) return fail(C3DGS_E_INVALID, "error_accumulate: without visible / rank the rows are the model's");
    if (P_model == 0 || P_rows == 0) return C3DGS_OK;
    if (!err_sum || !acc_max || !acc_sum) return fail(C3DGS_E_INVALID, "error_accumulate: the row and the two accumulators are required");
    launch_error_accumulate(P_model, P_rows, visible, rank, err_sum, acc_max, acc_sum, (hipStream_t)stream);
    C3DGS_STAGE("error_accumulate", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_weighted_distance(int64_t N, int32_t C, int32_t K, const float* coefs, const int64_t* gather,
                            const float* codebook, float* out_dist, int64_t* out_idx, void* stream)
{
    if (N < 0 || C < 0 || K <= 0) return fail(C3DGS_E_INVALID, "coefs and codebook must have same number of channels");
    if (N == 0) return C3DGS_OK;
    if (!coefs || !codebook || !out_dist || !out_idx) return fail(C3DGS_E_INVALID, "ceofs and codebook must have dimension 2");
    {
        StageTimer t_(ST_WDIST, (hipStream_t)stream);
        if (launch_weighted_distance(N, C, K, coefs, gather, codebook, out_dist, out_idx, (hipStream_t)stream))
            return fail(C3DGS_E_INVALID, "unsupported channel count");
    }
    C3DGS_STAGE_CHECK(ST_WDIST, 0, (hipStream_t)stream);
    return C3DGS_OK;
}

size_t c3dgs_weighted_distance_ws_bytes(int64_t N, int32_t C, int32_t K) { return wd_ws_bytes(N, C, K); }

int c3dgs_weighted_distance_ws(int64_t N, int32_t C, int32_t K, const float* coefs, const int64_t* gather, const float* codebook,
                               float* out_dist, int64_t* out_idx, void* ws, size_t ws_bytes, void* stream)
{
    if (N < 0 || C < 0 || K <= 0) return fail(C3DGS_E_INVALID, "coefs and codebook must have same number of channels");
    if (N == 0) return C3DGS_OK;
    if (!coefs || !codebook || !out_dist || !out_idx) return fail(C3DGS_E_INVALID, "ceofs and codebook must have dimension 2");
    {
        StageTimer t_(ST_WDIST, (hipStream_t)stream);
        if (launch_weighted_distance(N, C, K, coefs, gather, codebook, out_dist, out_idx, (hipStream_t)stream, ws, ws ? ws_bytes : 0))
            return fail(C3DGS_E_INVALID, "unsupported channel count");
    }
    C3DGS_STAGE_CHECK(ST_WDIST, 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_vq_accumulate(int64_t B, int32_t K, int32_t D, const float* x, const float* w, const int64_t* gather,
                        const int64_t* idx, const float* dist, float* S, double* dist_sum, void* stream)
{
    if (B < 0 || K <= 0 || D <= 0) return fail(C3DGS_E_INVALID, "bad sizes");
    if (B == 0) return C3DGS_OK;
    if (!x || !w || !idx || !S) return fail(C3DGS_E_INVALID, "x, w, idx and S are required");
    C3DGS_TIMED_STAGE(ST_VQ_ACC, 0, (hipStream_t)stream, launch_vq_accumulate(B, K, D, x, w, gather, idx, dist, S, dist_sum, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_vq_sums(int64_t B, int32_t K, int32_t D, const float* x, const float* w, const int64_t* gather,
                  const float* codebook, float* dist, int64_t* idx, float* S, double* dist_sum, void* ws, size_t ws_bytes,
                  void* stream)
{
    if (B < 0 || K <= 0 || D <= 0) return fail(C3DGS_E_INVALID, "bad sizes");
    if (!S || !dist_sum) return fail(C3DGS_E_INVALID, "S and dist_sum are required");
    C3DGS_HIP_TRY(hipMemsetAsync(S, 0, (size_t)K * (D + 1) * sizeof(float), (hipStream_t)stream));
    C3DGS_HIP_TRY(hipMemsetAsync(dist_sum, 0, sizeof(double), (hipStream_t)stream));
    if (B == 0) return C3DGS_OK;
    if (!x || !w || !codebook || !dist || !idx) return fail(C3DGS_E_INVALID, "x, w, codebook, dist and idx are required");
    {
        StageTimer t_(ST_WDIST, (hipStream_t)stream);
        if (launch_weighted_distance(B, K, D, x, gather, codebook, dist, idx, (hipStream_t)stream, ws, ws ? ws_bytes : 0))
            return fail(C3DGS_E_INVALID, "unsupported channel count");
    }
    C3DGS_STAGE_CHECK(ST_WDIST, 0, (hipStream_t)stream);
    return c3dgs_vq_accumulate(B, K, D, x, w, gather, idx, dist, S, dist_sum, stream);
}

int c3dgs_vq_step_supported(int32_t K, int32_t D, const float* x, const float* codebook, const void* ws, size_t ws_bytes)
{
    return (K > 0 && D > 0 && wd_presplit_supported(K, D, x, codebook, ws, ws_bytes)) ? 1 : 0;
}

int c3dgs_vq_step_sums(int32_t step, int64_t B, int32_t K, int32_t D, const float* x, const float* w, const int64_t* gather,
                       const float* codebook, float* dist, int64_t* idx, float* S, double* dist_sum, void* ws, size_t ws_bytes,
                       void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (step < 0 || B <= 0 || K <= 0 || D <= 0) return fail(C3DGS_E_INVALID, "vq_step_sums: bad sizes");
    if (!x || !w || !codebook || !dist || !idx || !S || !dist_sum) return fail(C3DGS_E_INVALID, "vq_step_sums: NULL argument");
    if (!wd_presplit_supported(K, D, x, codebook, ws, ws_bytes))
        return fail(C3DGS_E_INVALID, "vq_step_sums: shape / scratch not served by the fused step (see c3dgs_vq_step_supported)");
    if (step == 0) {            // nothing is prepared yet: the classic first half, then arm the scratch for c3dgs_vq_step_apply
        C3DGS_HIP_TRY(hipMemsetAsync(S, 0, (size_t)K * (D + 1) * sizeof(float), s));
        C3DGS_HIP_TRY(hipMemsetAsync(dist_sum, 0, sizeof(double), s));
    }
    {
        StageTimer t_(ST_WDIST, s);
        if (launch_weighted_distance(B, K, D, x, gather, codebook, dist, idx, s, ws, ws_bytes, step == 0 ? -1 : (step & 1)))
            return fail(C3DGS_E_INVALID, "vq_step_sums: unsupported shape");
        if (step == 0) launch_vq_seed_words(K, D, ws, s);
    }
    C3DGS_STAGE_CHECK(ST_WDIST, 0, s);
    C3DGS_TIMED_STAGE(ST_VQ_ACC, 0, s,
                      launch_vq_accumulate(B, K, D, x, w, gather, idx, dist, S, dist_sum, s, vq_next_absmax_word(K, D, ws, step & 1)));
    return C3DGS_OK;
}

int c3dgs_vq_step_apply(int32_t step, int32_t K, int32_t D, float* S, float* codebook, float* entry_importance, float decay,
                        float alpha, float eps, int32_t scale_normalize, void* ws, size_t ws_bytes, void* stream)
{
    if (step < 0 || K <= 0 || D <= 0 || !S || !codebook || !entry_importance) return fail(C3DGS_E_INVALID, "vq_step_apply: bad arguments");
    { StageTimer t_(ST_VQ_APPLY, (hipStream_t)stream);
      if (launch_vq_apply_split(K, D, S, codebook, entry_importance, decay, alpha, eps, scale_normalize, ws, ws_bytes, step & 1, (hipStream_t)stream))
          return fail(C3DGS_E_INVALID, "vq_step_apply: shape / scratch not served by the fused step (see c3dgs_vq_step_supported)"); }
    C3DGS_STAGE_CHECK(ST_VQ_APPLY, 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_vq_apply(int32_t K, int32_t D, const float* S, float* codebook, float* entry_importance, float decay,
                   float alpha, float eps, int32_t scale_normalize, void* stream)
{
    if (K <= 0 || D <= 0 || !S || !codebook || !entry_importance) return fail(C3DGS_E_INVALID, "bad arguments");
    C3DGS_TIMED_STAGE(ST_VQ_APPLY, 0, (hipStream_t)stream,
                      launch_vq_apply(K, D, S, codebook, entry_importance, decay, alpha, eps, scale_normalize, (hipStream_t)stream));
    return C3DGS_OK;
}

size_t c3dgs_morton_workspace_bytes(int32_t P) { return morton_workspace_bytes(P); }

int c3dgs_morton_order(int32_t P, const float* xyz, int64_t* codes, int64_t* order, void* workspace, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!xyz || !codes || !order || !workspace) return fail(C3DGS_E_INVALID, "morton_order: bad arguments");
    if (run_morton_order(P, xyz, codes, order, workspace, (hipStream_t)stream)) return fail(C3DGS_E_HIP, "morton_order failed");
    C3DGS_STAGE("morton_order", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

size_t c3dgs_knn_workspace_bytes(int32_t P) { return knn_workspace_bytes(P); }

int c3dgs_knn_mean_dist2(int32_t P, const float* xyz, float* out, void* workspace, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "knn_mean_dist2: P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!xyz || !out || !workspace) return fail(C3DGS_E_INVALID, "knn_mean_dist2: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    { StageTimer t_(ST_KNN_SORT, s);
      if (run_knn_sort(P, xyz, workspace, s)) return fail(C3DGS_E_HIP, "knn_mean_dist2: sort failed"); }
    C3DGS_STAGE_CHECK(ST_KNN_SORT, 0, s);
    C3DGS_TIMED_STAGE(ST_KNN_BOUNDS, 0, s, launch_knn_bounds(P, workspace, s));
    C3DGS_TIMED_STAGE(ST_KNN_QUERY, 0, s, launch_knn_query(P, workspace, out, s));
    return C3DGS_OK;
}

int c3dgs_knn_neighbours(int32_t P, const float* xyz, int32_t* idx, float* d2, void* workspace, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "knn_neighbours: P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!xyz || !idx || !d2 || !workspace) return fail(C3DGS_E_INVALID, "knn_neighbours: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    { StageTimer t_(ST_KNN_SORT, s);
      if (run_knn_sort(P, xyz, workspace, s)) return fail(C3DGS_E_HIP, "knn_neighbours: sort failed"); }
    C3DGS_STAGE_CHECK(ST_KNN_SORT, 0, s);
    C3DGS_TIMED_STAGE(ST_KNN_BOUNDS, 0, s, launch_knn_bounds(P, workspace, s));
    C3DGS_TIMED_STAGE(ST_KNN_QUERY, 0, s, launch_knn_query_neighbours(P, workspace, idx, d2, s));
    return C3DGS_OK;
}

// ---- geometry evaluation (nn_query.hip, mesh_sample.hip, geometry_metrics.hip) ----
static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

size_t c3dgs_nn_index_bytes(int32_t P) { return P < 0 ? 0 : knn_workspace_bytes(P); }

int c3dgs_nn_build(int32_t P, const float* xyz, void* index, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "nn_build: P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!xyz || !index) return fail(C3DGS_E_INVALID, "nn_build: xyz and index are required");
    if (misaligned(index, 256)) return fail(C3DGS_E_INVALID, "nn_build: index must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    { StageTimer t_(ST_KNN_SORT, s);
      if (run_knn_sort(P, xyz, index, s)) return fail(C3DGS_E_HIP, "nn_build: sort failed"); }
    C3DGS_STAGE_CHECK(ST_KNN_SORT, 0, s);
    C3DGS_TIMED_STAGE(ST_KNN_BOUNDS, 0, s, launch_knn_bounds(P, index, s));
    return C3DGS_OK;
}

size_t c3dgs_nn_query_workspace_bytes(int32_t Q) { return Q < 0 ? 0 : nn_query_workspace_bytes(Q); }

int c3dgs_nn_query(int32_t P, const void* index, int32_t Q, const float* queries, int32_t sort_queries, int32_t* idx, float* d2,
                   uint32_t* leaves, void* workspace, void* stream)
{
    if (P < 0 || Q < 0) return fail(C3DGS_E_INVALID, "nn_query: P and Q must be >= 0");
    if (Q == 0) return C3DGS_OK;
    if (P > 0 && !index) return fail(C3DGS_E_INVALID, "nn_query: index is NULL");
    const bool sorted = sort_queries != 0 && P > 0;          // without a reference set nothing is walked: nothing to order
    if (!queries || !idx || !d2) return fail(C3DGS_E_INVALID, "nn_query: queries, idx and d2 are required");
    if (sorted && !workspace) return fail(C3DGS_E_INVALID, "nn_query: sorted queries need the workspace");
    if (misaligned(index, 256) || (sorted && misaligned(workspace, 256)))
        return fail(C3DGS_E_INVALID, "nn_query: index and workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (sorted) {
        { StageTimer t_(ST_NN_QUERY_SORT, s);
          if (run_nn_query_sort(P, index, Q, queries, workspace, s)) return fail(C3DGS_E_HIP, "nn_query: sort failed"); }
        C3DGS_STAGE_CHECK(ST_NN_QUERY_SORT, 0, s);
    }
    C3DGS_TIMED_STAGE(ST_NN_QUERY, 0, s, launch_nn_query(P, index, Q, queries, sorted, workspace, idx, d2, leaves, s));
    return C3DGS_OK;
}

size_t c3dgs_mesh_sample_workspace_bytes(int32_t F) { return F < 0 ? 0 : mesh_sample_workspace_bytes(F); }

static int mesh_sample_validate(const char* who, int32_t V, const float* vertices, int32_t F, const int32_t* faces, const void* workspace,
                                size_t workspace_bytes)
{
    const std::string w(who);
    if (V < 0 || F < 0) return fail(C3DGS_E_INVALID, w + ": V and F must be >= 0");
    if (F == 0) return C3DGS_OK;
    if (!vertices || !faces) return fail(C3DGS_E_INVALID, w + ": vertices and faces are required");
    if (!workspace || workspace_bytes < mesh_sample_workspace_bytes(F) || misaligned(workspace, 256))
        return fail(C3DGS_E_INVALID, w + ": workspace must hold c3dgs_mesh_sample_workspace_bytes(F) bytes, 256-byte aligned");
    return C3DGS_OK;
}

int c3dgs_mesh_sample_count(int32_t V, const float* vertices, int32_t F, const int32_t* faces, float density, uint32_t seed,
                            void* workspace, size_t workspace_bytes, uint64_t* total, void* stream)
{
    if (int rc = mesh_sample_validate("mesh_sample_count", V, vertices, F, faces, workspace, workspace_bytes)) return rc;
    if (!(density > 0.f) || !(density <= FLT_MAX)) return fail(C3DGS_E_INVALID, "mesh_sample_count: density must be finite and positive");
    if (!total) return fail(C3DGS_E_INVALID, "mesh_sample_count: total is NULL");
    *total = 0;
    if (F == 0) return C3DGS_OK;
    hipStream_t s = (hipStream_t)stream;
    C3DGS_HIP_TRY(mesh_sample_clear(F, workspace, s));
    C3DGS_TIMED_STAGE(ST_MESH_SAMPLE_COUNT, 0, s, launch_mesh_sample_count(V, vertices, F, faces, density, seed, workspace, s));
    const uint32_t* words = nullptr;
    C3DGS_TIMED_STAGE(ST_MESH_SAMPLE_SCAN, 0, s, words = launch_mesh_sample_scan(F, workspace, s));
    uint32_t host[3] = { 0u, 0u, 0u };
    C3DGS_HIP_TRY(hipMemcpyAsync(host, words, sizeof(host), hipMemcpyDeviceToHost, s));
    C3DGS_HIP_TRY(hipStreamSynchronize(s));
    if (host[2] & 1u) return fail(C3DGS_E_INVALID, "mesh_sample_count: a face has a vertex index outside [0, V)");
    if (host[2] & 2u)
        return fail(C3DGS_E_INVALID, "mesh_sample_count: a face would get 2^24 or more samples (area * density); lower the density");
    const uint64_t n = (uint64_t)host[0] | ((uint64_t)host[1] << 32);
    if ((host[2] & 4u) || n > (uint64_t)INT32_MAX)
        return fail(C3DGS_E_INVALID, "mesh_sample_count: more than 2^31 - 1 samples; lower the density");
    *total = n;
    return C3DGS_OK;
}

int c3dgs_mesh_sample_emit(int32_t V, const float* vertices, int32_t F, const int32_t* faces, uint32_t seed, const void* workspace,
                           size_t workspace_bytes, int64_t S, float* points, int32_t* face, void* stream)
{
    if (int rc = mesh_sample_validate("mesh_sample_emit", V, vertices, F, faces, workspace, workspace_bytes)) return rc;
    if (S < 0 || S > INT32_MAX) return fail(C3DGS_E_INVALID, "mesh_sample_emit: S must be in [0, 2^31 - 1]");
    if (S == 0) return C3DGS_OK;
    if (F == 0) return fail(C3DGS_E_INVALID, "mesh_sample_emit: a mesh without faces has no samples");
    if (!points || !face) return fail(C3DGS_E_INVALID, "mesh_sample_emit: points and face are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_MESH_SAMPLE_EMIT, 0, s, launch_mesh_sample_emit(V, vertices, F, faces, seed, workspace, (uint32_t)S, points, face, s));
    return C3DGS_OK;
}

size_t c3dgs_geometry_reduce_workspace_bytes(int64_t N) { return N < 0 ? 0 : geometry_reduce_workspace_bytes(N); }

int c3dgs_geometry_reduce(int64_t N, const float* d2, const float* points, const float* bounds, float max_dist, int32_t T,
                          const float* thresholds, void* workspace, size_t workspace_bytes, double* out, void* stream)
{
    if (N < 0) return fail(C3DGS_E_INVALID, "geometry_reduce: N must be >= 0");
    if (T < 0 || T > C3DGS_GEOMETRY_MAX_THRESHOLDS) return fail(C3DGS_E_INVALID, "geometry_reduce: T must be in [0, 8]");
    if (T > 0 && !thresholds) return fail(C3DGS_E_INVALID, "geometry_reduce: thresholds is NULL");
    if (N > 0 && (points != nullptr) != (bounds != nullptr)) return fail(C3DGS_E_INVALID, "geometry_reduce: points and bounds come as a pair");
    if (!out || (N > 0 && !d2)) return fail(C3DGS_E_INVALID, "geometry_reduce: d2 and out are required");
    if (!workspace || workspace_bytes < geometry_reduce_workspace_bytes(N) || misaligned(workspace, 8) || misaligned(out, 8))
        return fail(C3DGS_E_INVALID, "geometry_reduce: workspace must hold c3dgs_geometry_reduce_workspace_bytes(N) bytes, 8-byte aligned");
    C3DGS_TIMED_STAGE(ST_GEOMETRY_REDUCE, 0, (hipStream_t)stream,
                      launch_geometry_reduce(N, d2, points, bounds, max_dist, T, thresholds, workspace, out, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_abs_accumulate(int64_t n, const float* g, float* acc, void* stream)
{
    if (n < 0 || (n > 0 && (!g || !acc))) return fail(C3DGS_E_INVALID, "abs_accumulate: bad arguments");
    launch_abs_accumulate(n, g, acc, (hipStream_t)stream);
    C3DGS_STAGE("abs_accumulate", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_adam_step(int32_t n_tensors, const c3dgs_adam_tensor* tensors, double beta1, double beta2, double eps, void* stream)
{
    if (n_tensors < 0 || n_tensors > C3DGS_ADAM_MAX_TENSORS) return fail(C3DGS_E_INVALID, "adam_step: between 0 and 16 tensors per call");
    if (n_tensors == 0) return C3DGS_OK;
    if (!tensors) return fail(C3DGS_E_INVALID, "adam_step: tensors is NULL");
    for (int k = 0; k < n_tensors; k++)
        if (tensors[k].n > 0 && (!tensors[k].param || !tensors[k].grad || !tensors[k].exp_avg || !tensors[k].exp_avg_sq))
            return fail(C3DGS_E_INVALID, "adam_step: NULL tensor pointer");
    C3DGS_TIMED_STAGE(ST_ADAM, 0, (hipStream_t)stream, launch_adam(n_tensors, tensors, beta1, beta2, eps, (hipStream_t)stream));
    return C3DGS_OK;
}

// ---- what the entries of sparse Adam, density control and MCMC check alike; each returns the message behind the entry's name
static const char* bad_row_count(int64_t P)
{
    if (P < 0) return "P must be >= 0";
    if (P >= (int64_t(1) << 31)) return "P must be below 2^31 (row ids are 32-bit)";
    return nullptr;
}
static const char* bad_workspace(const void* w)
{
    return !w || (reinterpret_cast<uintptr_t>(w) & 255u) ? "the workspace must be non-NULL and 256-byte aligned" : nullptr;
}
// the c3dgs_rows_tensor table of c3dgs_rows_apply / c3dgs_mcmc_apply. `rows`: how many rows the call writes; a call that
// writes none returns before it reads the table, so only the count is checked then.
static const char* bad_rows_table(int32_t n_tensors, const c3dgs_rows_tensor* tensors, int64_t rows)
{
    if (n_tensors < 0 || n_tensors > C3DGS_ROWS_MAX_TENSORS) return "between 0 and 16 tensors per call";
    if (rows == 0 || n_tensors == 0) return nullptr;
    if (!tensors) return "NULL buffer";
    for (int k = 0; k < n_tensors; k++)
        if (tensors[k].row_floats < 1 || tensors[k].row_floats > 4096) return "row_floats must be between 1 and 4096";
    return nullptr;
}

// ---- sparse Adam (sparse_adam.hip)

int c3dgs_sparse_adam_workspace_bytes(int64_t P, size_t* bytes)
{
    if (!bytes) return fail(C3DGS_E_INVALID, "sparse_adam_workspace_bytes: bytes is NULL");
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("sparse_adam_workspace_bytes: ") + bad);
    *bytes = sparse_adam_layout(P).total_bytes;
    return C3DGS_OK;
}

int c3dgs_sparse_adam_select(int64_t P, const void* mask, int32_t mask_kind, void* workspace, void* stream)
{
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("sparse_adam_select: ") + bad);
    if (mask_kind != 0 && mask_kind != 1) return fail(C3DGS_E_INVALID, "sparse_adam_select: mask_kind must be 0 (uint8 != 0) or 1 (int32 > 0)");
    if (P == 0) return C3DGS_OK;
    if (!mask) return fail(C3DGS_E_INVALID, "sparse_adam_select: mask is NULL");
    if (const char* bad = bad_workspace(workspace)) return fail(C3DGS_E_INVALID, std::string("sparse_adam_select: ") + bad);
    C3DGS_TIMED_STAGE(ST_SPARSE_ADAM_SELECT, 0, (hipStream_t)stream, launch_sparse_adam_select(P, mask, mask_kind, workspace, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_sparse_adam_step(int32_t n_tensors, const c3dgs_sparse_adam_tensor* tensors, int64_t P, const void* workspace, double beta1,
                           double beta2, double eps, void* stream)
{
    if (n_tensors < 0 || n_tensors > C3DGS_ADAM_MAX_TENSORS)
        return fail(C3DGS_E_INVALID, "sparse_adam_step: between 0 and 16 tensors per call");
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("sparse_adam_step: ") + bad);
    if (n_tensors == 0) return C3DGS_OK;
    if (!tensors) return fail(C3DGS_E_INVALID, "sparse_adam_step: tensors is NULL");
    for (int k = 0; k < n_tensors; k++) {
        const c3dgs_sparse_adam_tensor& t = tensors[k];
        if (t.row_len <= 0) return fail(C3DGS_E_INVALID, "sparse_adam_step: row_len must be > 0");
        if (t.n != P * (int64_t)t.row_len) return fail(C3DGS_E_INVALID, "sparse_adam_step: n must be P * row_len");
        if (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))
            return fail(C3DGS_E_INVALID, "sparse_adam_step: NULL tensor pointer");
    }
    if (P == 0) return C3DGS_OK;
    if (const char* bad = bad_workspace(workspace)) return fail(C3DGS_E_INVALID, std::string("sparse_adam_step: ") + bad);
    C3DGS_TIMED_STAGE(ST_SPARSE_ADAM_STEP, 0, (hipStream_t)stream,
                      launch_sparse_adam_step(n_tensors, tensors, P, workspace, beta1, beta2, eps, (hipStream_t)stream));
    return C3DGS_OK;
}

// ---- adaptive density control (densify.hip)
static const int kRowsMaxCopies = 250;     // kind is a byte: 2 + k

int c3dgs_densify_classify(int32_t P, const float* accum, const float* denom, const float* scale_clone, const float* scale_split,
                           const float* scale_prune_self, const float* scale_prune_child, const float* opacity, float max_grad,
                           float dense_extent, float min_opacity, float big_extent, uint8_t* code, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "densify_classify: P must be >= 0");
    if (!(max_grad > 0.f)) return fail(C3DGS_E_INVALID, "densify_classify: max_grad must be > 0 (see include/c3dgs_hip.h)");
    if (P == 0) return C3DGS_OK;
    if (!accum || !denom || !scale_clone || !scale_split || !opacity || !code)
        return fail(C3DGS_E_INVALID, "densify_classify: NULL buffer");
    if ((scale_prune_self == nullptr) != (scale_prune_child == nullptr))
        return fail(C3DGS_E_INVALID, "densify_classify: scale_prune_self and scale_prune_child go together");
    launch_densify_classify(P, accum, denom, scale_clone, scale_split, scale_prune_self, scale_prune_child, opacity, max_grad,
                            dense_extent, min_opacity, big_extent, code, (hipStream_t)stream);
    C3DGS_STAGE("densify_classify", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

size_t c3dgs_rows_plan_workspace_bytes(int32_t P) { return rows_plan_workspace_bytes(P); }

int c3dgs_rows_plan(int32_t P, const uint8_t* code, int32_t N, int64_t capacity, int32_t* src, uint8_t* kind, int32_t* draw_row,
                    int32_t* totals, void* workspace, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "rows_plan: P must be >= 0");
    if (N < 1 || N > kRowsMaxCopies) return fail(C3DGS_E_INVALID, "rows_plan: N must be between 1 and 250");
    if (capacity < 0) return fail(C3DGS_E_INVALID, "rows_plan: capacity must be >= 0");
    if ((int64_t)P * (2 + N) >= ((int64_t)1 << 31)) return fail(C3DGS_E_INVALID, "rows_plan: P * (2 + N) must fit 31 bits");
    if (!totals) return fail(C3DGS_E_INVALID, "rows_plan: totals is required");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) { C3DGS_HIP_TRY(hipMemsetAsync(totals, 0, 4 * sizeof(int32_t), s)); return C3DGS_OK; }
    if (!code || !workspace) return fail(C3DGS_E_INVALID, "rows_plan: NULL buffer");
    if (src && (!kind || !draw_row)) return fail(C3DGS_E_INVALID, "rows_plan: src, kind and draw_row go together");
    C3DGS_HIP_TRY(run_rows_plan(P, code, N, capacity, src, kind, draw_row, totals, workspace, s));
    C3DGS_STAGE("rows_plan", 0, s);
    return C3DGS_OK;
}

int c3dgs_rows_apply(int32_t P, int64_t P_new, const int32_t* src, const uint8_t* kind, const int32_t* draw_row, int32_t n_tensors,
                     const c3dgs_rows_tensor* tensors, int32_t N, int64_t n_draws, const float* rotation_raw, const float* std,
                     const float* z, int32_t log_scaling, int32_t half_xyz, void* stream)
{
    if (P < 0 || P_new < 0 || n_draws < 0) return fail(C3DGS_E_INVALID, "rows_apply: sizes must be >= 0");
    if (N < 1 || N > kRowsMaxCopies) return fail(C3DGS_E_INVALID, "rows_apply: N must be between 1 and 250");
    if (const char* bad = bad_rows_table(n_tensors, tensors, P_new)) return fail(C3DGS_E_INVALID, std::string("rows_apply: ") + bad);
    if (P_new >= ((int64_t)1 << 31)) return fail(C3DGS_E_INVALID, "rows_apply: P_new must fit 31 bits");
    if (P_new == 0 || n_tensors == 0) return C3DGS_OK;
    if (P == 0) return fail(C3DGS_E_INVALID, "rows_apply: P_new > 0 rows cannot come from P = 0");
    if (!src || !kind || !draw_row) return fail(C3DGS_E_INVALID, "rows_apply: NULL buffer");
    for (int k = 0; k < n_tensors; k++) {
        const c3dgs_rows_tensor& t = tensors[k];
        if (!t.in_param || !t.out_param) return fail(C3DGS_E_INVALID, "rows_apply: NULL tensor pointer");
        const int nm = (t.in_exp_avg != nullptr) + (t.in_exp_avg_sq != nullptr) + (t.out_exp_avg != nullptr) + (t.out_exp_avg_sq != nullptr);
        if (nm != 0 && nm != 4) return fail(C3DGS_E_INVALID, "rows_apply: the four moment pointers go together");
        if (t.role != C3DGS_ROLE_COPY && t.role != C3DGS_ROLE_XYZ && t.role != C3DGS_ROLE_SCALING)
            return fail(C3DGS_E_INVALID, "rows_apply: unknown role");
        if (t.role != C3DGS_ROLE_COPY && t.row_floats != 3) return fail(C3DGS_E_INVALID, "rows_apply: xyz / scaling rows have 3 floats");
        if (t.role != C3DGS_ROLE_COPY && n_draws > 0 && (!std || !z || (t.role == C3DGS_ROLE_XYZ && !rotation_raw)))
            return fail(C3DGS_E_INVALID, "rows_apply: children need rotation_raw, std and z");
    }
    launch_rows_apply(P, P_new, src, kind, draw_row, n_tensors, tensors, N, n_draws, rotation_raw, std, z, log_scaling, half_xyz, (hipStream_t)stream);
    C3DGS_STAGE("rows_apply", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_densify_stats(int32_t P, const float* grad, const uint8_t* filter, const int32_t* radii, float* accum, float* denom,
                        float* max_radii, void* stream)
{
    if (P < 0) return fail(C3DGS_E_INVALID, "densify_stats: P must be >= 0");
    if (P == 0) return C3DGS_OK;
    if (!grad || !filter || !accum || !denom) return fail(C3DGS_E_INVALID, "densify_stats: NULL buffer");
    if ((radii == nullptr) != (max_radii == nullptr)) return fail(C3DGS_E_INVALID, "densify_stats: radii and max_radii go together");
    launch_densify_stats(P, grad, filter, radii, accum, denom, max_radii, (hipStream_t)stream);
    C3DGS_STAGE("densify_stats", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

// ---- MCMC density control (mcmc.hip)
int c3dgs_mcmc_workspace_bytes(int64_t P, size_t* bytes)
{
    if (!bytes) return fail(C3DGS_E_INVALID, "mcmc_workspace_bytes: bytes is NULL");
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("mcmc_workspace_bytes: ") + bad);
    *bytes = mcmc_layout(P).total_bytes;
    return C3DGS_OK;
}

int c3dgs_mcmc_sample(int64_t P, const float* raw_opacity, const uint8_t* dead, int32_t derive_dead, float min_opacity,
                      uint8_t* dead_out, int64_t n, const double* draws, int32_t reuse_weights, uint32_t* q, int32_t* sources,
                      int32_t* counts, uint64_t* T, void* workspace, void* stream)
{
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("mcmc_sample: ") + bad);
    if (n < 0) return fail(C3DGS_E_INVALID, "mcmc_sample: n must be >= 0");
    if (n >= (int64_t(1) << 31)) return fail(C3DGS_E_INVALID, "mcmc_sample: n must be below 2^31");
    if (dead && derive_dead) return fail(C3DGS_E_INVALID, "mcmc_sample: a dead mask and derive_dead exclude each other");
    if (P == 0) return C3DGS_OK;
    if (!counts) return fail(C3DGS_E_INVALID, "mcmc_sample: counts is NULL");
    if (!reuse_weights) {
        if (!raw_opacity || !q || !T) return fail(C3DGS_E_INVALID, "mcmc_sample: raw_opacity, q and T are required");
        if (derive_dead && !dead_out) return fail(C3DGS_E_INVALID, "mcmc_sample: derive_dead needs dead_out");
        if (derive_dead && !(min_opacity >= 0.f)) return fail(C3DGS_E_INVALID, "mcmc_sample: min_opacity must be >= 0");
    }
    if (n > 0 && (!draws || !sources)) return fail(C3DGS_E_INVALID, "mcmc_sample: n > 0 needs draws and sources");
    if (const char* bad = bad_workspace(workspace)) return fail(C3DGS_E_INVALID, std::string("mcmc_sample: ") + bad);
    hipStream_t s = (hipStream_t)stream;
    if (reuse_weights) C3DGS_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)P * sizeof(int32_t), s));
    else
        C3DGS_TIMED_STAGE(ST_MCMC_WEIGHTS, 0, s, launch_mcmc_weights(P, raw_opacity, dead, derive_dead, min_opacity, dead_out, q, counts,
                                                                     (unsigned long long*)T, workspace, s));
    if (n > 0) C3DGS_TIMED_STAGE(ST_MCMC_SEARCH, 0, s, launch_mcmc_search(P, n, draws, sources, counts, workspace, s));
    return C3DGS_OK;
}

int c3dgs_mcmc_apply(int64_t P, int64_t n, const int32_t* dst, int64_t dst_base, const int32_t* sources, const int32_t* counts,
                     int32_t n_tensors, const c3dgs_rows_tensor* tensors, int32_t copy_rows, float min_opacity, void* workspace,
                     void* stream)
{
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("mcmc_apply: ") + bad);
    if (n < 0) return fail(C3DGS_E_INVALID, "mcmc_apply: n must be >= 0");
    if (n >= (int64_t(1) << 31)) return fail(C3DGS_E_INVALID, "mcmc_apply: n must be below 2^31");
    if (const char* bad = bad_rows_table(n_tensors, tensors, P ? n : 0)) return fail(C3DGS_E_INVALID, std::string("mcmc_apply: ") + bad);
    if (!(min_opacity >= 0.f && min_opacity < 1.f)) return fail(C3DGS_E_INVALID, "mcmc_apply: min_opacity must be in [0, 1)");
    if (P == 0 || n == 0) return C3DGS_OK;
    if (!sources || !counts) return fail(C3DGS_E_INVALID, "mcmc_apply: NULL buffer");
    if (!dst && (dst_base < 0 || dst_base + n > P)) return fail(C3DGS_E_INVALID, "mcmc_apply: dst_base + n must lie inside [0, P]");
    const c3dgs_rows_tensor* opacity = nullptr;
    const c3dgs_rows_tensor* scale = nullptr;
    for (int k = 0; k < n_tensors; k++) {
        const c3dgs_rows_tensor& t = tensors[k];
        if (!t.out_param || t.in_param != t.out_param) return fail(C3DGS_E_INVALID, "mcmc_apply: the step is in place (in_param == out_param, not NULL)");
        if (t.in_exp_avg != t.out_exp_avg || t.in_exp_avg_sq != t.out_exp_avg_sq || (t.out_exp_avg == nullptr) != (t.out_exp_avg_sq == nullptr))
            return fail(C3DGS_E_INVALID, "mcmc_apply: the moment pointers go together and are in place");
        if (t.role == C3DGS_MCMC_ROLE_OPACITY) {
            if (opacity || t.row_floats != 1) return fail(C3DGS_E_INVALID, "mcmc_apply: one opacity tensor of 1 float per row");
            opacity = &t;
        } else if (t.role == C3DGS_MCMC_ROLE_SCALE) {
            if (scale || t.row_floats > 3) return fail(C3DGS_E_INVALID, "mcmc_apply: one scale tensor of 1 to 3 floats per row");
            scale = &t;
        } else if (t.role != C3DGS_ROLE_COPY) return fail(C3DGS_E_INVALID, "mcmc_apply: unknown role");
    }
    if (!opacity || !scale) return fail(C3DGS_E_INVALID, "mcmc_apply: the table needs the opacity and the scale tensor");
    if (const char* bad = bad_workspace(workspace)) return fail(C3DGS_E_INVALID, std::string("mcmc_apply: ") + bad);
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_MCMC_VALUES, 0, s, launch_mcmc_values(P, counts, opacity->in_param, scale->in_param, scale->row_floats, min_opacity, workspace, s));
    C3DGS_TIMED_STAGE(ST_MCMC_APPLY, 0, s, launch_mcmc_apply(P, n, dst, dst_base, sources, n_tensors, tensors, copy_rows, workspace, s));
    return C3DGS_OK;
}

int c3dgs_mcmc_noise(int64_t P, float* xyz, const float* rotation, const float* scaling, const float* scaling_factor,
                     const float* raw_opacity, const float* xi, float noise_lr, float xyz_lr, void* stream)
{
    if (const char* bad = bad_row_count(P)) return fail(C3DGS_E_INVALID, std::string("mcmc_noise: ") + bad);
    if (P == 0) return C3DGS_OK;
    if (!xyz || !rotation || !scaling || !raw_opacity || !xi) return fail(C3DGS_E_INVALID, "mcmc_noise: NULL buffer");
    C3DGS_TIMED_STAGE(ST_MCMC_NOISE, 0, (hipStream_t)stream,
                      launch_mcmc_noise(P, xyz, rotation, scaling, scaling_factor, raw_opacity, xi, noise_lr, xyz_lr, (hipStream_t)stream));
    return C3DGS_OK;
}

// ---- per-image colour correction: bilateral grids (bilagrid.hip)
// the sizes every bilagrid entry takes; H = W = 1 where there is no image. -> the message, or null
static const char* bilagrid_bad_sizes(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg)
{
    if (H <= 0 || W <= 0 || L <= 0 || Hg <= 0 || Wg <= 0) return "every size must be positive";
    const int64_t lim = int64_t(1) << 31;
    const int64_t lh = (int64_t)L * Hg;
    if (lh >= lim || lh * Wg >= lim || 12 * lh * Wg >= lim) return "12 * L * Hg * Wg must be below 2^31";
    if (3 * (int64_t)H * W >= lim) return "3 * H * W must be below 2^31";
    return nullptr;
}
// the launch limits of the gather: vertices x slabs workgroups along x, level chunks along y
static const char* bilagrid_bad_plan(const BilagridPlan& plan)
{
    if (plan.groups >= (int64_t(1) << 31) || plan.chunks > 65535) return "the gather's launch does not fit (vertices x slabs >= 2^31 or L > 524280)";
    return nullptr;
}

size_t c3dgs_bilagrid_workspace_bytes(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg)
{
    if (const char* bad = bilagrid_bad_sizes(H, W, L, Hg, Wg)) { set_error(std::string("bilagrid_workspace_bytes: ") + bad); return 0; }
    return bilagrid_plan(H, W, L, Hg, Wg).total_bytes;
}

int c3dgs_bilagrid_slice(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg, const float* grid, const float* rgb, float* out,
                         void* stream)
{
    if (const char* bad = bilagrid_bad_sizes(H, W, L, Hg, Wg)) return fail(C3DGS_E_INVALID, std::string("bilagrid_slice: ") + bad);
    if (!grid || !rgb || !out) return fail(C3DGS_E_INVALID, "bilagrid_slice: grid, rgb and out are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_BILAGRID_SLICE, 0, s, launch_bilagrid_slice(H, W, L, Hg, Wg, grid, rgb, out, s));
    return C3DGS_OK;
}

int c3dgs_bilagrid_slice_backward(int32_t H, int32_t W, int32_t L, int32_t Hg, int32_t Wg, const float* grid, const float* rgb,
                                  const float* dL_dout, float* dL_dgrid, float* dL_drgb, void* workspace, void* stream)
{
    if (const char* bad = bilagrid_bad_sizes(H, W, L, Hg, Wg)) return fail(C3DGS_E_INVALID, std::string("bilagrid_slice_backward: ") + bad);
    if (!grid || !rgb || !dL_dout || !dL_dgrid)
        return fail(C3DGS_E_INVALID, "bilagrid_slice_backward: grid, rgb, dL_dout and dL_dgrid are required");
    if (!workspace) return fail(C3DGS_E_INVALID, "bilagrid_slice_backward: the workspace is NULL (c3dgs_bilagrid_workspace_bytes)");
    const BilagridPlan plan = bilagrid_plan(H, W, L, Hg, Wg);
    if (const char* bad = bilagrid_bad_plan(plan)) return fail(C3DGS_E_INVALID, std::string("bilagrid_slice_backward: ") + bad);
    hipStream_t s = (hipStream_t)stream;
    {
        StageTimer t_(ST_BILAGRID_SLICE_BWD, s);
        { StageTimer a_(ST_BILAGRID_GATHER, s); launch_bilagrid_gather(H, W, L, Hg, Wg, plan, rgb, dL_dout, (float*)workspace, s); }
        { StageTimer b_(ST_BILAGRID_FOLD, s); launch_bilagrid_fold(L, Hg, Wg, plan, (const float*)workspace, dL_dgrid, s); }
        if (dL_drgb) { StageTimer c_(ST_BILAGRID_RGB_BWD, s); launch_bilagrid_rgb_backward(H, W, L, Hg, Wg, grid, rgb, dL_dout, dL_drgb, s); }
    }
    C3DGS_STAGE_CHECK(ST_BILAGRID_SLICE_BWD, 0, s);
    return C3DGS_OK;
}

// what the two total-variation entries ask of their sizes
static const char* bilagrid_bad_tv_sizes(int32_t C, int32_t L, int32_t Hg, int32_t Wg)
{
    if (C <= 0) return "every size must be positive";
    if (const char* bad = bilagrid_bad_sizes(1, 1, L, Hg, Wg)) return bad;
    if ((int64_t)C * 12 * L * Hg * Wg >= (int64_t(1) << 31)) return "C * 12 * L * Hg * Wg must be below 2^31";
    return nullptr;
}

int c3dgs_bilagrid_tv(int32_t C, int32_t L, int32_t Hg, int32_t Wg, const float* grids, void* workspace, float* out, void* stream)
{
    if (const char* bad = bilagrid_bad_tv_sizes(C, L, Hg, Wg)) return fail(C3DGS_E_INVALID, std::string("bilagrid_tv: ") + bad);
    if (!grids || !out) return fail(C3DGS_E_INVALID, "bilagrid_tv: grids and out are required");
    if (!workspace) return fail(C3DGS_E_INVALID, "bilagrid_tv: the workspace is NULL (c3dgs_bilagrid_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_BILAGRID_TV, 0, s, launch_bilagrid_tv(C, L, Hg, Wg, grids, (double*)workspace, out, s));
    return C3DGS_OK;
}

int c3dgs_bilagrid_tv_backward(int32_t C, int32_t L, int32_t Hg, int32_t Wg, const float* grids, const float* dL_dtv,
                               float* dL_dgrids, void* stream)
{
    if (const char* bad = bilagrid_bad_tv_sizes(C, L, Hg, Wg)) return fail(C3DGS_E_INVALID, std::string("bilagrid_tv_backward: ") + bad);
    if (!grids || !dL_dtv || !dL_dgrids) return fail(C3DGS_E_INVALID, "bilagrid_tv_backward: grids, dL_dtv and dL_dgrids are required");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_TIMED_STAGE(ST_BILAGRID_TV_BWD, 0, s, launch_bilagrid_tv_backward(C, L, Hg, Wg, grids, dL_dtv, dL_dgrids, s));
    return C3DGS_OK;
}

// ---- initial densification (ray_fill.hip)
size_t c3dgs_ray_fill_plan_workspace_bytes(int32_t P, int64_t rows) { return ray_fill_plan_workspace_bytes(P, rows); }

int c3dgs_ray_fill_plan(int32_t P, const float* d2, float step, int64_t capacity, int32_t* src, uint8_t* slot, int32_t* level,
                        int32_t* totals, void* workspace, size_t workspace_bytes, void* stream)
{
    if (P < 0 || capacity < 0) return fail(C3DGS_E_INVALID, "ray_fill_plan: P and capacity must be >= 0");
    if (P > INT32_MAX - 255) return fail(C3DGS_E_INVALID, "ray_fill_plan: P must be at most INT32_MAX - 255");
    if (!(step > 0.f) || !(step <= FLT_MAX)) return fail(C3DGS_E_INVALID, "ray_fill_plan: step must be a positive finite number");
    if (!totals) return fail(C3DGS_E_INVALID, "ray_fill_plan: totals is required");
    if (src && (!slot || !level)) return fail(C3DGS_E_INVALID, "ray_fill_plan: src, slot and level go together");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) { C3DGS_HIP_TRY(hipMemsetAsync(totals, 0, 4 * sizeof(int32_t), s)); return C3DGS_OK; }
    if (!d2 || !workspace) return fail(C3DGS_E_INVALID, "ray_fill_plan: NULL buffer");
    std::string problem;
    C3DGS_HIP_TRY(run_ray_fill_plan(P, d2, step, capacity, src, slot, level, totals, workspace, workspace_bytes, s, &problem));
    if (!problem.empty()) return fail(C3DGS_E_INVALID, "ray_fill_plan: " + problem);
    C3DGS_STAGE("ray_fill_plan", 0, s);
    return C3DGS_OK;
}

int c3dgs_ray_fill_xyz(int32_t P, const float* xyz, const int32_t* idx, const float* d2, float step, int64_t n_new,
                       const int32_t* src, const uint8_t* slot, const int32_t* level, float* out, void* stream)
{
    if (P < 0 || n_new < 0) return fail(C3DGS_E_INVALID, "ray_fill_xyz: sizes must be >= 0");
    if (n_new > INT32_MAX - 255) return fail(C3DGS_E_INVALID, "ray_fill_xyz: n_new must be at most INT32_MAX - 255");
    if (!(step > 0.f) || !(step <= FLT_MAX)) return fail(C3DGS_E_INVALID, "ray_fill_xyz: step must be a positive finite number");
    if (n_new == 0) return C3DGS_OK;
    if (!xyz || !idx || !d2 || !src || !slot || !level || !out) return fail(C3DGS_E_INVALID, "ray_fill_xyz: NULL buffer");
    launch_ray_fill_xyz(P, xyz, idx, d2, step, n_new, src, slot, level, out, (hipStream_t)stream);
    C3DGS_STAGE("ray_fill_xyz", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

// ---- ground-truth image of a camera (image_io.hip)
int c3dgs_image_from_u8(int32_t Hs, int32_t Ws, int32_t C, const uint8_t* src, int32_t flip, const float* bg, int32_t Hd, int32_t Wd,
                        float* out, void* stream)
{
    const int32_t kMax = 32768;
    if (Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1 || Hs > kMax || Ws > kMax || Hd > kMax || Wd > kMax)
        return fail(C3DGS_E_INVALID, "image_from_u8: every dimension must be in [1, 32768]");
    if (C != 3 && C != 4) return fail(C3DGS_E_INVALID, "image_from_u8: C must be 3 or 4");
    if (bg && C == 3) return fail(C3DGS_E_INVALID, "image_from_u8: a background needs an alpha channel (C == 4)");
    if (!src || !out) return fail(C3DGS_E_INVALID, "image_from_u8: NULL buffer");
    launch_image_from_u8(Hs, Ws, C, src, flip != 0, bg, Hd, Wd, out, (hipStream_t)stream);
    C3DGS_STAGE("image_from_u8", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

// ---- prune / codebook compaction of an indexed model (index_plan.hip)
static const int32_t kIndexPlanMaxRows = INT32_MAX - 255;     // one lane per row in 256-lane workgroups, int arithmetic

size_t c3dgs_index_plan_workspace_bytes(int32_t P, int32_t K0, int32_t K1) { return index_plan_workspace_bytes(P, K0, K1); }

int c3dgs_index_plan(int32_t P, const uint8_t* keep, const int64_t* idx0, int32_t K0, const int64_t* idx1, int32_t K1, int64_t cap_rows,
                     int64_t cap_cb0, int64_t cap_cb1, int32_t* src, int64_t* new_idx0, int64_t* new_idx1, int32_t* cb_src0,
                     int32_t* cb_src1, int32_t* totals, void* workspace, void* stream)
{
    if (P < 0 || K0 < 0 || K1 < 0) return fail(C3DGS_E_INVALID, "index_plan: P, K0 and K1 must be >= 0");
    if (P > kIndexPlanMaxRows || K0 > kIndexPlanMaxRows || K1 > kIndexPlanMaxRows)
        return fail(C3DGS_E_INVALID, "index_plan: P, K0 and K1 must be at most INT32_MAX - 255");
    if (cap_rows < 0 || cap_cb0 < 0 || cap_cb1 < 0) return fail(C3DGS_E_INVALID, "index_plan: capacities must be >= 0");
    if ((idx0 && K0 <= 0) || (idx1 && K1 <= 0)) return fail(C3DGS_E_INVALID, "index_plan: an index array needs a codebook of K > 0 rows");
    if (!totals) return fail(C3DGS_E_INVALID, "index_plan: totals is required");
    if (!workspace) return fail(C3DGS_E_INVALID, "index_plan: workspace is required");
    if (src && ((idx0 && (!new_idx0 || !cb_src0)) || (idx1 && (!new_idx1 || !cb_src1))))
        return fail(C3DGS_E_INVALID, "index_plan: src, and new_idx and cb_src of every index space given, go together");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) { C3DGS_HIP_TRY(hipMemsetAsync(totals, 0, 4 * sizeof(int32_t), s)); return C3DGS_OK; }
    C3DGS_HIP_TRY(run_index_plan(P, keep, idx0, K0, idx1, K1, cap_rows, cap_cb0, cap_cb1, src, new_idx0, new_idx1, cb_src0, cb_src1,
                                 totals, workspace, s));
    C3DGS_STAGE("index_plan", 0, s);
    return C3DGS_OK;
}

int c3dgs_extract_rot_scale(int32_t n, const float* cov6, float* rot, float* scale, void* stream)
{
    if (n < 0) return fail(C3DGS_E_INVALID, "extract_rot_scale: n must be >= 0");
    if (n == 0) return C3DGS_OK;
    if (!cov6 || !rot || !scale || (reinterpret_cast<uintptr_t>(rot) & 15)) return fail(C3DGS_E_INVALID, "extract_rot_scale: bad arguments");
    launch_extract_rot_scale(n, cov6, rot, scale, (hipStream_t)stream);
    C3DGS_STAGE("extract_rot_scale", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, float* dmaps, double* sums,
                          void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !sums) return fail(C3DGS_E_INVALID, "l1_ssim_forward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    C3DGS_HIP_TRY(hipMemsetAsync(sums, 0, 128 * sizeof(double), s));
    const size_t n = (size_t)C * H * W;
    C3DGS_TIMED_STAGE(ST_LOSS_FWD, 0, s,
                      launch_l1_ssim_forward(C, H, W, img, gt, dmaps, dmaps ? dmaps + n : nullptr, dmaps ? dmaps + 2 * n : nullptr, sums, s));
    return C3DGS_OK;
}

int c3dgs_l1_ssim_value(const double* sums, double l1_scale, double ssim_scale, double constant, float* out, void* stream)
{
    if (!sums || !out) return fail(C3DGS_E_INVALID, "l1_ssim_value: bad arguments");
    launch_l1_ssim_value(sums, l1_scale, ssim_scale, constant, out, (hipStream_t)stream);
    C3DGS_STAGE("l1_ssim_value", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, const float* dmaps,
                           const float* grad_loss, float l1_coeff, float ssim_coeff, float* dL_dimg, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !dmaps || !grad_loss || !dL_dimg)
        return fail(C3DGS_E_INVALID, "l1_ssim_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)C * H * W;
    C3DGS_TIMED_STAGE(ST_LOSS_BWD, 0, s,
                      launch_l1_ssim_backward(C, H, W, img, gt, dmaps, dmaps + n, dmaps + 2 * n, grad_loss, l1_coeff, ssim_coeff, dL_dimg, s));
    return C3DGS_OK;
}

// ---- image metrics of the evaluation pass (metrics.hip) ----
size_t c3dgs_image_metrics_ws_bytes(int32_t N, int32_t C, int32_t H, int32_t W) { return image_metrics_ws_bytes(N, C, H, W); }

int c3dgs_image_metrics(int32_t N, int32_t C, int32_t H, int32_t W, const float* img, const float* gt, void* ws, size_t ws_bytes,
                        double* out, void* stream)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(C3DGS_E_INVALID, "image_metrics: N, C, H and W must be positive");
    if (image_metrics_workgroups(N, C, H, W) > IMAGE_METRICS_MAX_WORKGROUPS)
        return fail(C3DGS_E_INVALID, "image_metrics: size overflow (N * C * H * W too large for one call; split the batch)");
    if (!img || !gt || !ws || !out) return fail(C3DGS_E_INVALID, "image_metrics: img, gt, ws and out are required");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(C3DGS_E_INVALID, "image_metrics: ws must be 8-byte aligned");
    const size_t need = image_metrics_ws_bytes(N, C, H, W);
    if (ws_bytes < need)
        return fail(C3DGS_E_INVALID, "image_metrics: ws too small (" + std::to_string(ws_bytes) + " bytes, need " +
                                         std::to_string(need) + ")");
    launch_image_metrics(N, C, H, W, img, gt, (double*)ws, out, (hipStream_t)stream);
    C3DGS_STAGE("image_metrics", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

// ---- QAT getters ----
static int qat_validate(const c3dgs_qat_params* q, const char* who)
{
    if (!q) return fail(C3DGS_E_INVALID, std::string(who) + ": params is NULL");
    if (q->P < 0 || q->GS < 0 || q->SHS < 0 || q->M < 1) return fail(C3DGS_E_INVALID, std::string(who) + ": bad sizes");
    if (!q->state) return fail(C3DGS_E_INVALID, std::string(who) + ": state is required");
    if (q->features_dc && q->M > 1 && !q->features_rest)
        return fail(C3DGS_E_INVALID, std::string(who) + ": features_rest is required with features_dc when M > 1");
    if (reinterpret_cast<uintptr_t>(q->rotation) & 15) return fail(C3DGS_E_INVALID, std::string(who) + ": rotation must be 16-byte aligned");
    return C3DGS_OK;
}
static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

size_t c3dgs_qat_workspace_bytes(void) { return qat_workspace_bytes(); }
size_t c3dgs_qat_scan_bytes(int32_t P) { return qat_scan_bytes(P); }

int c3dgs_qat_observe(const c3dgs_qat_params* q, void* workspace, void* stream)
{
    if (int rc = qat_validate(q, "qat_observe")) return rc;
    if (!workspace) return fail(C3DGS_E_INVALID, "qat_observe: workspace is required");
    C3DGS_TIMED_STAGE(ST_QAT_OBSERVE, 0, (hipStream_t)stream, launch_qat_observe(*q, workspace, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_qat_codebooks(const c3dgs_qat_params* q, float* scales_n, float* rotations, float* shs, void* stream)
{
    if (int rc = qat_validate(q, "qat_codebooks")) return rc;
    if (misaligned16(rotations) || misaligned16(shs)) return fail(C3DGS_E_INVALID, "qat_codebooks: outputs must be 16-byte aligned");
    C3DGS_TIMED_STAGE(ST_QAT_CODEBOOKS, 0, (hipStream_t)stream, launch_qat_codebooks(*q, scales_n, rotations, shs, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_qat_codebooks_backward(const c3dgs_qat_params* q, const float* dL_dscales_n, const float* dL_drotations,
                                 const float* dL_dshs, float* dL_dscaling, float* dL_drotation, float* dL_dfeatures_dc,
                                 float* dL_dfeatures_rest, void* stream)
{
    if (int rc = qat_validate(q, "qat_codebooks_backward")) return rc;
    if (misaligned16(dL_drotations) || misaligned16(dL_drotation) || misaligned16(dL_dshs))
        return fail(C3DGS_E_INVALID, "qat_codebooks_backward: rotation / sh gradients must be 16-byte aligned");
    if (dL_dshs && q->features_dc && (!dL_dfeatures_dc || (q->M > 1 && !dL_dfeatures_rest)))
        return fail(C3DGS_E_INVALID, "qat_codebooks_backward: dL_dfeatures_dc / dL_dfeatures_rest are required with dL_dshs");
    C3DGS_TIMED_STAGE(ST_QAT_CODEBOOKS_BWD, 0, (hipStream_t)stream,
                      launch_qat_codebooks_backward(*q, dL_dscales_n, dL_drotations, dL_dshs, dL_dscaling, dL_drotation, dL_dfeatures_dc,
                                                    dL_dfeatures_rest, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_qat_visible(const c3dgs_qat_params* q, const float* viewmatrix, uint8_t* visible, int32_t* rank, int32_t* count,
                      void* scan_workspace, void* stream)
{
    if (int rc = qat_validate(q, "qat_visible")) return rc;
    if (!count) return fail(C3DGS_E_INVALID, "qat_visible: count is required");
    hipStream_t s = (hipStream_t)stream;
    if (q->P == 0) { C3DGS_HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t), s)); return C3DGS_OK; }
    if (!q->xyz || !viewmatrix || !visible || !rank || !scan_workspace) return fail(C3DGS_E_INVALID, "qat_visible: bad arguments");
    { StageTimer t_(ST_QAT_VISIBLE, s); C3DGS_HIP_TRY(run_qat_visible(*q, viewmatrix, visible, rank, count, scan_workspace, s)); }
    C3DGS_STAGE_CHECK(ST_QAT_VISIBLE, 0, s);
    return C3DGS_OK;
}

int c3dgs_qat_points(const c3dgs_qat_params* q, const uint8_t* visible, const int32_t* rank, const int64_t* sh_indices,
                     const int64_t* g_indices, float* means3D, float* opacities, float* scale_factors, int64_t* sh_indices_out,
                     int64_t* g_indices_out, void* stream)
{
    if (int rc = qat_validate(q, "qat_points")) return rc;
    if ((visible == nullptr) != (rank == nullptr)) return fail(C3DGS_E_INVALID, "qat_points: visible and rank go together");
    C3DGS_TIMED_STAGE(ST_QAT_POINTS, 0, (hipStream_t)stream,
                      launch_qat_points(*q, visible, rank, sh_indices, g_indices, means3D, opacities, scale_factors, sh_indices_out,
                                        g_indices_out, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_qat_points_backward(const c3dgs_qat_params* q, const uint8_t* visible, const int32_t* rank, const float* dL_dmeans3D,
                              const float* dL_dmeans2D, const float* dL_dopacities, const float* dL_dscale_factors,
                              float* dL_dxyz, float* dL_dscreenspace, float* dL_dopacity, float* dL_dscaling_factor, void* stream)
{
    if (int rc = qat_validate(q, "qat_points_backward")) return rc;
    if ((visible == nullptr) != (rank == nullptr)) return fail(C3DGS_E_INVALID, "qat_points_backward: visible and rank go together");
    if ((dL_dopacity && dL_dopacities && !q->opacity) || (dL_dscaling_factor && dL_dscale_factors && !q->scaling_factor))
        return fail(C3DGS_E_INVALID, "qat_points_backward: the raw opacity / scaling_factor are needed to recompute the masks");
    C3DGS_TIMED_STAGE(ST_QAT_POINTS_BWD, 0, (hipStream_t)stream,
                      launch_qat_points_backward(*q, visible, rank, dL_dmeans3D, dL_dmeans2D, dL_dopacities, dL_dscale_factors, dL_dxyz,
                                                 dL_dscreenspace, dL_dopacity, dL_dscaling_factor, (hipStream_t)stream));
    return C3DGS_OK;
}

int c3dgs_qat_quantize(const c3dgs_qat_params* q, int32_t scaling_is_exp, int8_t* opacity, int8_t* scaling, int8_t* scaling_factor,
                       int8_t* rotation, int8_t* features_dc, int8_t* features_rest, void* stream)
{
    if (int rc = qat_validate(q, "qat_quantize")) return rc;
    if (rotation && (reinterpret_cast<uintptr_t>(rotation) & 3)) return fail(C3DGS_E_INVALID, "qat_quantize: rotation output must be 4-byte aligned");
    launch_qat_quantize(*q, scaling_is_exp, opacity, scaling, scaling_factor, rotation, features_dc, features_rest, (hipStream_t)stream);
    C3DGS_STAGE("qat_quantize", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_fake_quantize(int64_t n, const float* x, c3dgs_fq_state* state, int32_t observe, int32_t enabled,
                        float averaging_constant, float* out, void* workspace, void* stream)
{
    if (n < 0) return fail(C3DGS_E_INVALID, "fake_quantize: n must be >= 0");
    if (n == 0) return C3DGS_OK;
    if (!x || !state || !out || (observe && !workspace)) return fail(C3DGS_E_INVALID, "fake_quantize: bad arguments");
    launch_fake_quantize(n, x, state, observe, enabled, averaging_constant, out, workspace, (hipStream_t)stream);
    C3DGS_STAGE("fake_quantize", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

int c3dgs_fake_quantize_backward(int64_t n, const float* x, const c3dgs_fq_state* state, int32_t enabled, const float* g,
                                 float* dx, void* stream)
{
    if (n < 0) return fail(C3DGS_E_INVALID, "fake_quantize_backward: n must be >= 0");
    if (n == 0) return C3DGS_OK;
    if (!x || !state || !g || !dx) return fail(C3DGS_E_INVALID, "fake_quantize_backward: bad arguments");
    launch_fake_quantize_backward(n, x, state, enabled, g, dx, (hipStream_t)stream);
    C3DGS_STAGE("fake_quantize_backward", 0, (hipStream_t)stream);
    return C3DGS_OK;
}

} // extern "C"
