"""Build c3dgs_amd/libc3dgs_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m c3dgs_amd.build [--force] [--verbose] [--variants] [--diag]

Per-file flags matter: preprocess.hip / backward_preprocess.hip are compiled with -ffp-contract=off
because radii, tile rectangles and depth bits feed bit-exact integer tile keys (see csrc/gsmath.hpp); knn.hip
because its distances are a bit-exact contract.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libc3dgs_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
          "-fno-gpu-rdc", "-DNDEBUG"]
SOURCES = {
    "c_abi.hip": [],
    "c_abi_debug.hip": [],      # test hooks (include/c3dgs_hip_debug.h, c3dgs_hip_depth_sort_debug.h)
    "preprocess.hip": ["-ffp-contract=off"],
    "backward_preprocess.hip": ["-ffp-contract=off"] + os.environ.get("C3DGS_BWDPRE_FLAGS", "").split(),
    "binning.hip": [],
    "radix_sort.hip": os.environ.get("C3DGS_SORT_FLAGS", "").split(),
    # SLP packing into v_pk_*_f32 costs register shuffles in the blend loops and keeps DPP adds from fusing
    "render.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    # the depth / alpha / median replay of the forward's blend: render.hip's flags, so that the shared alpha expression compiles alike
    "render_depth.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    # the gradients through every map: the same replay, walked back to front with render.hip's backward recurrences
    "render_maps_backward.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    # the distortion and normal maps: siblings of render_depth.hip, render.hip's flags for the same reason
    "render_distortion.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    "render_normal.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    # the per-Gaussian normals, their fold and the depth -> normal stencil: single fp32 operations that tests/normal_ref.py
    # restates, and the chains of csrc/gsgrad.hpp
    "normals.hip": ["-ffp-contract=off"],
    # the per-Gaussian blend statistics: the same replay, the same flags
    "render_contrib.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    # the per-Gaussian error scores: the same replay and the same reduction network, the same flags
    "render_error.hip": os.environ.get("C3DGS_RENDER_FLAGS", "-fno-slp-vectorize").split(),
    # MFMA accumulators in VGPRs (no v_accvgpr_read per value in the top-2 update of the search kernel)
    "vq.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"] + os.environ.get("C3DGS_VQ_FLAGS", "").split(),
    # the exact pose gradient rebuilds Sigma as preprocess does (csrc/gsmath.hpp) and the SH direction term with the function
    # backward_preprocess calls (csrc/gsgrad.hpp)
    "pose_grad.hip": ["-ffp-contract=off"],
    # the opacity compensation of the antialiased mode forms the 2D covariance with preprocess's expressions (csrc/gsmath.hpp) and
    # chains its gradient with the functions of csrc/gsgrad.hpp
    "aa_opacity.hip": ["-ffp-contract=off"],
    # the 3D smoothing filter: its projections are single fp32 operations a NumPy restatement repeats bit for bit, and its
    # covariance is preprocess's (csrc/gsmath.hpp); its backward is the covariance chain of csrc/gsgrad.hpp, which must round as
    # backward_preprocess's does (tests/test_gsgrad_gpu.py)
    "filter3d.hip": ["-ffp-contract=off"],
    # mesh extraction: the projections of the TSDF fusion and the edge interpolation of the marching tetrahedra are single fp32
    # operations that tests/mesh_ref.py restates bit for bit
    "mesh.hip": ["-ffp-contract=off"],
    "draws.hip": [],
    "loss.hip": [],
    "metrics.hip": [],
    "encode.hip": [],
    "knn.hip": ["-ffp-contract=off"],       # the distances and box bounds are bit-exact fp32 expressions (csrc/knn.hip)
    # geometry evaluation: the same distances and bounds for external queries (csrc/knn_tree.hpp), the sampler's areas and
    # positions, and the reduction's sqrt are single fp32 operations that tests/geometry_ref.py restates bit for bit
    "nn_query.hip": ["-ffp-contract=off"],
    "mesh_sample.hip": ["-ffp-contract=off"],
    "geometry_metrics.hip": ["-ffp-contract=off"],
    "adam.hip": ["-ffp-contract=off"],
    "sparse_adam.hip": ["-ffp-contract=off"],   # adam.hip's arithmetic (csrc/adam_common.hpp), rounded as adam.hip rounds it
    "qat.hip": ["-ffp-contract=off"],
    "densify.hip": ["-ffp-contract=off"],   # sqrt(gx*gx + gy*gy) of the densification stats is torch's two-rounding sum
    # MCMC density control: t = floor(u * T) of the sampler is one IEEE multiply that the host restatement repeats (csrc/mcmc.hip)
    "mcmc.hip": ["-ffp-contract=off"],
    # per-image colour correction (bilateral grids): no test needs separately rounded operations, so contraction stays on
    "bilagrid.hip": [],
    "index_plan.hip": [],
    "ray_fill.hip": ["-ffp-contract=off"],  # x * (1 - a) + a * y of the new positions is four separately rounded operations
    "image_io.hip": ["-ffp-contract=off"],  # t0 * (1 - f) + t1 * f of the bilinear taps is separately rounded (csrc/image_io.hip)
}
HEADERS = [os.path.join(CSRC, "common.hpp"), os.path.join(CSRC, "gsmath.hpp"), os.path.join(CSRC, "gsgrad.hpp"),
           os.path.join(CSRC, "render_diag.hpp"),
           os.path.join(CSRC, "render_common.hpp"), os.path.join(CSRC, "replay.hpp"), os.path.join(CSRC, "scan_blocks.hpp"), os.path.join(CSRC, "adam_common.hpp"), os.path.join(CSRC, "mcmc.hpp"), os.path.join(CSRC, "jobs.hpp"),
           os.path.join(CSRC, "bilagrid.hpp"), os.path.join(CSRC, "knn_tree.hpp"),
           os.path.join(HERE, "..", "include", "c3dgs_hip.h"), os.path.join(HERE, "..", "include", "c3dgs_hip_debug.h"),
           os.path.join(HERE, "..", "include", "c3dgs_hip_depth_sort_debug.h")]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(name, extra, verbose):
    src = os.path.join(CSRC, name)
    obj = os.path.join(OBJ, name.replace(".hip", ".o"))
    cmd = [HIPCC] + COMMON + extra + ["-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return obj


# Variants of the library: same sources, extra flags for some files; objects of untouched files are shared with the product build.
# VARIANTS are what tests need. "spin1": every look-back of the radix sorts gives up after ONE poll, which forces the time-out
# path that tests/test_sort_gpu.py::test_sort_timeout_is_not_silent exercises (loaded through C3DGS_LIB_PATH in a child process).
VARIANTS = {"spin1": {"radix_sort.hip": ["-DC3DGS_OS_SPIN_LIMIT=1u"]}}
# DIAG_VARIANTS are measurement builds (python -m c3dgs_amd.build --diag): the two instrumented files are compiled with
# -DC3DGS_DIAG plus the variant's mode flag and diag.hip, which is no product source, is linked in, so every one of them exports
# the measurement entries of include/c3dgs_hip_debug.h (zeros for the kinds of data its mode does not collect).
#   "lanes":   the blend kernels count how many pixel lanes use each (wave, Gaussian) pair (tools/lane_efficiency.py)
#   "bwdtime": render_backward sums the shader clock per phase (tools/bwd_phases.py)
#   "ostime":  the digit passes of the onesweep sorts stamp the shader clock at their phase boundaries (tools/sort_phases.py)
def _diag(mode):
    return {src: ["-DC3DGS_DIAG", mode] for src in ("render.hip", "radix_sort.hip", "diag.hip")}


DIAG_VARIANTS = {"lanes": _diag("-DC3DGS_COUNT_LANES"), "bwdtime": _diag("-DC3DGS_BWD_TIMING"), "ostime": _diag("-DC3DGS_OS_TIMING")}


def build_variant(name, verbose=False):
    build(verbose=verbose)
    flags = {**VARIANTS, **DIAG_VARIANTS}[name]
    odir = os.path.join(HERE, "build", "variant_" + name)
    os.makedirs(odir, exist_ok=True)
    lib = os.path.join(HERE, f"libc3dgs_hip_{name}.so")
    objs, rebuilt = [], False
    for src in list(SOURCES) + [f for f in flags if f not in SOURCES]:
        extra = SOURCES.get(src, [])
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        if src in flags:
            obj = os.path.join(odir, src.replace(".hip", ".o"))
            if _stale(obj, [os.path.join(CSRC, src)] + HEADERS + [os.path.abspath(__file__)]):
                cmd = [HIPCC] + COMMON + extra + flags[src] + ["-c", os.path.join(CSRC, src), "-o", obj]
                if verbose:
                    print(" ".join(cmd), flush=True)
                subprocess.check_call(cmd)
                rebuilt = True
        objs.append(obj)
    if rebuilt or _stale(lib, objs):
        subprocess.check_call([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs)
    return lib


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    deps_common = HEADERS + [os.path.abspath(__file__)]
    todo, objs = [], []
    for name, extra in SOURCES.items():
        obj = os.path.join(OBJ, name.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [os.path.join(CSRC, name)] + deps_common):
            todo.append((name, extra))
    if todo:
        with ThreadPoolExecutor(max_workers=min(4, len(todo))) as ex:
            list(ex.map(lambda t: _compile(t[0], t[1], verbose), todo))
    if force or todo or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv or "-v" in sys.argv))
    for flag, table in (("--variants", VARIANTS), ("--diag", DIAG_VARIANTS)):
        for v in table if flag in sys.argv else ():
            print(build_variant(v, verbose="--verbose" in sys.argv or "-v" in sys.argv))
