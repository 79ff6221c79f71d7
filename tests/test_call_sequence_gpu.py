"""-m gpu: state that outlives a call. Nine configurations of the rasterizer, all through the autograd modules (so that the cached
workspaces, the mapped host pad with its sequence numbers and the sticky sort time-out word take part), are first run once each
and recorded -- every record checked against the oracle with the checkers of the parity tests --, then run in a fixed, seeded
order in which every ordered pair X -> Y of different configurations occurs (tests/call_sequence.py), and every call must give
its record again: bit for bit where the project declares the output reproducible, within the parity bar for the scatter-added
codebook gradients of the indexed path. The order is run on the default stream, once more on a second stream, and once more with
every uninitialised allocation filled with 0xFF between guard bands (tests/poison.py). At the end no call may have raised the
sort's time-out word.

  A   37,001 Gaussians (three depth-sort tiles and a ragged tail) on 64 x 64, depths below 512: the three-pass depth sort
  B   A with one Gaussian at depth 600: the four-pass fallback
  C   prefiltered, 4,097 Gaussians: the four raw passes
  D   63 Gaussians on 33 x 17
  E   2,000 Gaussians on 4,112 x 16: 257 tile columns, the gather variant; a far larger image buffer under a small scene
  F   indexed, 12,289 Gaussians, depth_grad (with a loss on both maps), contrib and error_target
  F'  F at 257 Gaussians: the same layouts, smaller, over what F left
  G   everything behind the camera (R = 0)
  H   no Gaussians (P = 0)"""
import numpy as np
import pytest
import torch

from tests import call_sequence, gpu_util, poison, synth
from tests import test_scratch_poison_gpu as sp

pytestmark = pytest.mark.gpu

NAMES = ("A", "B", "C", "D", "E", "F", "F'", "G", "H")
SEED = 20240
LEAF_KEYS = ("means3D", "opacities", "shs", "colors_precomp", "scales", "scale_factors", "rotations", "cov3D_precomp")
GRAD_OF = {"means3D": "dL_dmeans3D", "means2D": "dL_dmeans2D", "opacities": "dL_dopacity", "shs": "dL_dsh", "scales": "dL_dscales",
           "rotations": "dL_drotations", "scale_factors": "dL_dscale_factors", "colors_precomp": "dL_dcolors", "cov3D_precomp": "dL_dcov3D"}
EXTRAS = ("depth", "alpha", "median", "weight_sum", "weight_max", "hits", "err_sum")


class Config:
    """one configuration: the case and its oracle reference (computed once, shared, not to be modified), its inputs on the device"""

    def __init__(self, hip, name):
        variant, P, image, route = {"A": ("base", sp.SIZES[-1], "64x64", "plain"), "B": ("base", sp.SIZES[-1], "64x64", "far"),
                                    "C": ("base", 4097, "64x64", "prefiltered"), "D": ("base", 63, "33x17", "plain"),
                                    "E": ("base", 2000, "64x64", "wide"), "F": ("indexed", sp.TILE + 1, "64x64", "plain"),
                                    "F'": ("indexed", 257, "64x64", "plain"), "G": ("all_behind", 257, "64x64", "plain"),
                                    "H": ("empty", 257, "64x64", "plain")}[name]
        self.name, self.full = name, name in ("F", "F'")
        self.inp, self.cam, self.indexed, self.st, dL, self.ref = sp._raster_reference(variant, P, image, route)
        inp, W, H = self.inp, self.cam["W"], self.cam["H"]
        self.W, self.H = W, H
        identity = route == "wide"
        focal = 2000.0 if identity else sp.IMAGES[image]["focal"]
        intr, ev = synth.camera(W, H, focal, **({} if identity else dict(extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))))
        self.ev = ev.cuda()
        self.dL = torch.from_numpy(dL).cuda()
        self.dev = {k: inp[k].cuda() for k in LEAF_KEYS + ("sh_indices", "g_indices") if inp.get(k) is not None}
        skw = {}
        if self.full:
            from tests.test_depth_grad_gpu import _maps
            self.gD, self.gA = (torch.from_numpy(m).cuda() for m in _maps(W, H))
            self.target = synth.grad_image(W, H, seed=5).abs().clamp(0, 1).cuda().contiguous()
            skw = dict(depth_grad=True, contrib=True, error_target=self.target)
        self.rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=self.ev, bg=inp["bg"].cuda(),
                                                    scale_modifier=float(inp["scale_modifier"]), sh_degree=int(inp["degree"]),
                                                    prefiltered=bool(inp["prefiltered"]), debug=False, clamp_color=bool(inp["clamp_color"]), **skw)
        self.rast = (hip.GaussianRasterizerIndexed if self.indexed else hip.GaussianRasterizer)(self.rs)

    def call(self):
        """one forward and backward through the module -> {name: numpy}: the forward's arrays (gpu_util.unpack), the extras, the
        gradients of the image loss (`dL_*`) and, with maps, those of the image + maps loss (`full.dL_*`)"""
        d = self.dev
        leaves = {k: d[k].detach().requires_grad_() for k in LEAF_KEYS if k in d}
        leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
        kw = dict(means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacities"], shs=leaves.get("shs"),
                  colors_precomp=leaves.get("colors_precomp"), scales=leaves.get("scales"), rotations=leaves.get("rotations"),
                  cov3D_precomp=leaves.get("cov3D_precomp"), extrinsic_vector=self.ev)
        if self.indexed:
            kw.update(sh_indices=d["sh_indices"], g_indices=d["g_indices"], scale_factors=leaves.get("scale_factors"))
        out = self.rast(**kw)
        fn = out[0].grad_fn                                  # the Function's ctx: the three buffers are among what it saved
        geom, binning, img = fn.saved_tensors[9:12]
        fw = dict(radii=out[1], color=out[0].detach(), geom=geom, binning=binning, img=img, num_rendered=fn.num_rendered, W=self.W, H=self.H)
        rec = sp._forward_outputs(fw)
        rec.update(zip(EXTRAS, (t.detach() for t in out[2:])))

        def grads(loss, prefix, **kw):
            for v in leaves.values():
                v.grad = None
            loss.backward(**kw)
            for k, v in leaves.items():
                rec[prefix + GRAD_OF[k]] = (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy()
        image_loss = (out[0] * self.dL).sum()
        grads(image_loss, "", retain_graph=self.full)
        if self.full:
            grads(image_loss + (out[2] * self.gD).sum() + (out[3] * self.gA).sum(), "full.")
        torch.cuda.synchronize()
        return {k: poison._np(v) for k, v in rec.items()}

    def check_record(self, rec):
        """the record against the oracle: the forward and the gradients with the checkers of tests/test_raster_gpu.py, the extras
        with those of their own tests"""
        from tests import fullsize
        from tests.test_raster_gpu import GRAD_TOL, _check_forward
        st = self.st
        u = {k: v for k, v in rec.items() if "dL_" not in k and k not in EXTRAS}
        u["num_rendered"] = int(u["num_rendered"])
        _check_forward(u, st)
        got = {k: v.reshape(self.ref[k].shape) for k, v in rec.items() if k.startswith("dL_") and k in self.ref and v.size == self.ref[k].size}
        assert set(got) == {GRAD_OF[k] for k in list(self.dev) + ["means2D"] if k in GRAD_OF}, sorted(got)
        fullsize.check_grads(st, u, got, self.ref, GRAD_TOL, "record " + self.name)
        assert np.isfinite(rec["out_color"]).all()
        if self.full:
            from tests import contrib_ref, depth_ref, error_ref
            from tests.test_render_contrib_gpu import check_against_walk
            from tests.test_render_depth_gpu import check_maps
            from tests.test_render_error_gpu import check_scores
            from c3dgs_amd import rasterizer as rz
            label = "record " + self.name
            check_maps(label, self.inp, self.cam, self.indexed, st, u, rec["depth"], rec["alpha"], rec["median"],
                       walk=depth_ref.walk(st, st.W, st.H))
            hits = rec["hits"].view(np.uint32)
            check_against_walk(label, u, rec["weight_sum"], rec["weight_max"], hits, ref=contrib_ref.walk(st, st.W, st.H))
            emap = rz._C.error_map_l1(torch.from_numpy(rec["out_color"]).cuda(), self.target).cpu().numpy()
            check_scores(label, u, rec["err_sum"], hits, ref=error_ref.walk(st, st.W, st.H, emap))
            for k in ("dL_dmeans3D", "dL_dopacity"):        # the maps' loss reaches them
                assert gpu_util.rel_inf(rec["full." + k], rec[k]) > 1e-3, k

    def same_as_record(self, got, rec, where):
        from tests.test_raster_gpu import GRAD_TOL
        assert got.keys() == rec.keys(), where
        for k, v in got.items():
            if self.indexed and k.split(".")[-1] in sp.SCATTERED:        # float atomics: the order of the adds is not fixed
                assert gpu_util.rel_inf(v, rec[k]) <= GRAD_TOL, (where, k, gpu_util.rel_inf(v, rec[k]))
            else:
                assert v.shape == rec[k].shape and v.dtype == rec[k].dtype, (where, k)
                assert poison._bits(v).tobytes() == poison._bits(rec[k]).tobytes(), f"{where}: {k} differs from its record"


@pytest.fixture(scope="module")
def recorded(hip, orc):
    """each configuration run once, in order, recorded and checked against the oracle"""
    configs = {n: Config(hip, n) for n in NAMES}
    records = {}
    for n in NAMES:
        records[n] = configs[n].call()
        configs[n].check_record(records[n])
    st = {n: configs[n].st for n in NAMES}
    assert st["A"].num_rendered > 8192 and st["G"].num_rendered == 0 and st["G"].P > 0 and st["H"].P == 0
    assert int(st["B"].depths.view(np.uint32)[7]) >= sp.LIMIT3 and st["B"].radii[7] > 0
    assert int(st["A"].depths.view(np.uint32)[st["A"].radii > 0].max()) < sp.LIMIT3
    assert (configs["E"].W + 15) // 16 > 255
    return configs, records


def _run_sequence(configs, records, label):
    seq = call_sequence.sequence(NAMES, SEED)
    assert call_sequence.covers_every_ordered_pair(seq, NAMES)          # the condition, on the sequence that is run
    for i, n in enumerate(seq):
        got = configs[n].call()
        configs[n].same_as_record(got, records[n], f"{label}, call {i} ({seq[i - 1] if i else '-'} -> {n})")


def _no_timeout_was_raised(configs):
    """a forward fails if an earlier call raised the sort's sticky time-out word, and clears it: one more, then nothing is pending"""
    rec = configs["D"].call()
    assert np.isfinite(rec["out_color"]).all()


def test_every_ordered_pair_on_the_default_stream(recorded):
    configs, records = recorded
    _run_sequence(configs, records, "default stream")
    _no_timeout_was_raised(configs)


def test_every_ordered_pair_on_a_second_stream(recorded):
    configs, records = recorded
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _run_sequence(configs, records, "second stream")
        _no_timeout_was_raised(configs)
    torch.cuda.synchronize()


def test_every_ordered_pair_under_poison(recorded):
    configs, records = recorded
    with poison.poisoned(0xFF) as p:
        _run_sequence(configs, records, "poisoned 0xFF")
        _no_timeout_was_raised(configs)
    frames = {r.frame.split(":")[1] for r in p.records if r.nbytes}
    assert {"_resize", "_forward", "_backward", "get", "_c_render_depth"} <= frames, frames      # scratch, outputs and the cached workspaces
