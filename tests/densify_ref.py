"""Torch restatement of the reference's STAGED adaptive density control -- TEST INFRASTRUCTURE, NOT THE PRODUCT.

Device-agnostic (CPU for tests/test_densify_ref_cpu.py, the GPU for tests/test_densify_gpu.py and tools/time_densify.py):
what scene/gaussian_model.py does for a non-indexed model, in its order and with its torch ops,
    densification_postfix / cat_tensors_to_optimizer   :1161-1211      -> Staged.extend
    prune_points / _prune_optimizer                      :1081-1158      -> Staged.prune_points
    densify_and_clone, densify_and_split                 :1213-1330
    densify_and_prune                                    :1336-1349
    reset_opacity                                        :1391-1397
with real torch.ao.quantization.FakeQuantize modules as the reference builds them (:109-134). Two extra per-row tensors
ride along (`src`: the row of the scene the call started from, `kind`: 0 original, 1 clone, 2 + k child copy k), so the
result carries its provenance. tests/golden/densify.npz pins this file against the reference itself.

classify_ref / plan_ref restate the fused decision (csrc/densify.hip) on explicit activated inputs.
"""
import torch

PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "scaling_factor")
KEEP, CLONE, SPLIT, CHILD_KEPT = 1, 2, 4, 8


def make_qa(quantization, device):
    """The three modules the density control touches. quantization=False switches the scaling pair off; opacity_qa stays on."""
    qa = {k: torch.ao.quantization.FakeQuantize(dtype=torch.qint8).to(device) for k in ("opacity", "scaling", "scaling_factor")}
    if not quantization:
        for k in ("scaling", "scaling_factor"):
            qa[k].disable_fake_quant()
            qa[k].disable_observer()
    return qa


def qa_state(mod):
    """(min_val, max_val, scale, zero_point) as Python floats / int."""
    o = mod.activation_post_process
    return float(o.min_val), float(o.max_val), float(mod.scale), int(mod.zero_point)


def set_qa_state(mod, min_val, max_val, scale, zero_point):
    o = mod.activation_post_process
    dev = mod.scale.device
    o.min_val = torch.tensor(float(min_val), device=dev)
    o.max_val = torch.tensor(float(max_val), device=dev)
    mod.scale.fill_(float(scale))
    mod.zero_point.fill_(int(zero_point))


def build_rotation(r):
    """Rotation matrices of RAW quaternions (r, x, y, z), normalised first: utils/general_utils.py:84-107, entry by entry."""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


class Staged:
    """The scene of the staged sequence: `p[name]` parameters, `m[name]` = (exp_avg, exp_avg_sq) or None, the three
    accumulators, the modules, and the provenance rows."""

    def __init__(self, params, moments=None, accum=None, denom=None, max_radii2D=None, qa=None, quantization=True,
                 use_factor_scaling=True, percent_dense=0.01):
        self.p = {k: v for k, v in params.items() if v is not None}
        self.m = {k: (moments[k] if moments and moments.get(k) is not None else None) for k in self.p}
        dev = self.p["xyz"].device
        n = self.p["xyz"].shape[0]
        self.device = dev
        self.accum = accum if accum is not None else torch.zeros(n, 1, device=dev)
        self.denom = denom if denom is not None else torch.zeros(n, 1, device=dev)
        self.max_radii2D = max_radii2D if max_radii2D is not None else torch.zeros(n, device=dev)
        self.qa = qa if qa is not None else make_qa(quantization, dev)
        self.use_factor_scaling = use_factor_scaling
        self.quantization = quantization
        self.percent_dense = percent_dense
        self.src = torch.arange(n, device=dev)
        self.kind = torch.zeros(n, dtype=torch.long, device=dev)
        self.draws_used = None

    # getters, :213-267
    @property
    def get_scaling(self):
        if self.use_factor_scaling:
            scaling_n = self.qa["scaling"](torch.nn.functional.normalize(torch.nn.functional.relu(self.p["scaling"])))
            return torch.exp(self.qa["scaling_factor"](self.p["scaling_factor"])) * scaling_n
        return self.qa["scaling"](torch.exp(self.p["scaling"]))

    @property
    def get_xyz(self):                                           # xyz_qa: FakeQuantizationHalf when quantisation aware
        return self.p["xyz"].half().float() if self.quantization else self.p["xyz"]

    @property
    def get_opacity(self):
        return self.qa["opacity"](torch.sigmoid(self.p["opacity"]))

    def extend(self, new, src, kind):                            # densification_postfix
        for k in self.p:
            ext = new[k]
            if self.m[k] is not None:
                self.m[k] = (torch.cat((self.m[k][0], torch.zeros_like(ext)), dim=0),
                             torch.cat((self.m[k][1], torch.zeros_like(ext)), dim=0))
            self.p[k] = torch.cat((self.p[k], ext), dim=0)
        self.src = torch.cat((self.src, src))
        self.kind = torch.cat((self.kind, kind))
        n = self.p["xyz"].shape[0]
        self.accum = torch.zeros((n, 1), device=self.device)
        self.denom = torch.zeros((n, 1), device=self.device)
        self.max_radii2D = torch.zeros((n,), device=self.device)

    def prune_points(self, mask):
        valid = ~mask
        for k in self.p:
            if self.m[k] is not None:
                self.m[k] = (self.m[k][0][valid], self.m[k][1][valid])
            self.p[k] = self.p[k][valid]
        self.src, self.kind = self.src[valid], self.kind[valid]
        self.accum, self.denom, self.max_radii2D = self.accum[valid], self.denom[valid], self.max_radii2D[valid]

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        mask = torch.where(torch.norm(grads, dim=-1) >= grad_threshold, True, False)
        mask = torch.logical_and(mask, torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        new = {k: v[mask] for k, v in self.p.items()}
        self.extend(new, self.src[mask], torch.ones_like(self.kind[mask]))

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, draws=None):
        n_init = self.p["xyz"].shape[0]
        scaling = self.get_scaling
        rotation = self.p["rotation"]
        padded = torch.zeros((n_init), device=self.device)
        padded[:grads.shape[0]] = grads.squeeze()
        mask = torch.where(padded >= grad_threshold, True, False)
        mask = torch.logical_and(mask, torch.max(scaling, dim=1).values > self.percent_dense * scene_extent)
        stds = scaling[mask].repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=self.device)
        z = draws if draws is not None else torch.randn(stds.shape, device=self.device)
        self.draws_used = z
        samples = z * stds + means                              # torch.normal(mean=means, std=stds)
        rots = build_rotation(rotation[mask]).repeat(N, 1, 1)
        new = {k: v[mask].repeat(N, *([1] * (v.dim() - 1))) for k, v in self.p.items()}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.get_xyz[mask].repeat(N, 1)
        new["scaling"] = stds / (0.8 * N) if self.use_factor_scaling else torch.log(stds / (0.8 * N))
        S = int(mask.sum())
        kinds = torch.arange(N, device=self.device).repeat_interleave(S) + 2
        self.extend(new, self.src[mask].repeat(N), kinds)
        self.prune_points(torch.cat((mask, torch.zeros(N * S, device=self.device, dtype=bool))))

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, draws=None, N=2):
        grads = self.accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent, N, draws)
        prune_mask = (self.get_opacity < min_opacity).squeeze(-1)
        if max_screen_size:
            big_points_vs = self.max_radii2D > max_screen_size  # dead: the postfix has zeroed max_radii2D
            big_points_ws = self.get_scaling.max(dim=1).values > 0.1 * extent
            prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
        self.prune_points(prune_mask)

    def reset_opacity(self):
        new = torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01)   # two accesses: the observer moves twice
        self.p["opacity"] = torch.log(new / (1 - new))
        if self.m["opacity"] is not None:
            self.m["opacity"] = (torch.zeros_like(self.p["opacity"]), torch.zeros_like(self.p["opacity"]))


# ---- the fused decision on explicit activated inputs
def classify_ref(accum, denom, scale_clone, scale_split, scale_prune_self, scale_prune_child, opacity, max_grad, dense_extent,
                 min_opacity, big_extent):
    """The reference's predicates with torch's own tensor-vs-Python-scalar comparisons -> uint8 codes."""
    g = accum.reshape(-1, 1) / denom.reshape(-1, 1)
    g[g.isnan()] = 0.0
    clone = (torch.norm(g, dim=-1) >= max_grad) & (torch.max(scale_clone, dim=1).values <= dense_extent)
    split = (g.squeeze(-1) >= max_grad) & (torch.max(scale_split, dim=1).values > dense_extent)
    low = opacity.reshape(-1) < min_opacity
    prune_self, prune_child = low, low
    if scale_prune_self is not None:
        prune_self = low | (scale_prune_self.max(dim=1).values > big_extent)
        prune_child = low | (scale_prune_child.max(dim=1).values > big_extent)
    code = (~split & ~prune_self).long() * KEEP + (clone & ~prune_self).long() * CLONE + split.long() * SPLIT + \
        (split & ~prune_child).long() * CHILD_KEPT
    return code.to(torch.uint8)


def plan_ref(code, N=2):
    """-> src, kind, draw_row (int64), (kept, clones, S, parents whose children survive) in the reference's row order."""
    code = code.long()
    idx = torch.arange(code.shape[0], device=code.device)
    keep, clone = (code & KEEP) != 0, (code & CLONE) != 0
    split = (code & SPLIT) != 0
    ck = split & ((code & CHILD_KEPT) != 0)
    S = int(split.sum())
    rank = torch.cumsum(split.long(), 0) - 1                    # rank among all S selected parents
    parts_src = [idx[keep], idx[clone]] + [idx[ck]] * N
    parts_kind = [torch.zeros_like(idx[keep]), torch.ones_like(idx[clone])] + [torch.full_like(idx[ck], 2 + k) for k in range(N)]
    parts_draw = [torch.full_like(idx[keep], -1), torch.full_like(idx[clone], -1)] + [k * S + rank[ck] for k in range(N)]
    return torch.cat(parts_src), torch.cat(parts_kind), torch.cat(parts_draw), (int(keep.sum()), int(clone.sum()), S, int(ck.sum()))


def fused_codes(scene, max_grad, min_opacity, extent, max_screen_size, N=2):
    """The decision GaussianModel.densify_and_prune takes, restated with the torch.ao modules of `scene` (a Staged, left
    untouched except for its observers): three or four observer accesses on P-row (and one 2P-row) batches instead of the
    staged scenes -> (code uint8[P], std [P,3]). Duplicated rows do not move a batch's min / max, so the observers end
    where the staged sequence leaves them."""
    raw_s, raw_f = scene.p["scaling"], scene.p.get("scaling_factor")

    def activated(raw, factor):
        if scene.use_factor_scaling:
            scaling_n = scene.qa["scaling"](torch.nn.functional.normalize(torch.nn.functional.relu(raw)))
            return torch.exp(scene.qa["scaling_factor"](factor)) * scaling_n
        return scene.qa["scaling"](torch.exp(raw))

    dense_extent, big_extent = scene.percent_dense * extent, 0.1 * extent
    s1 = activated(raw_s, raw_f)
    s2 = activated(raw_s, raw_f)
    opacity = scene.get_opacity
    sp_self = sp_child = None
    if max_screen_size:
        raw = classify_ref(scene.accum, scene.denom, s1, s2, None, None, opacity, max_grad, dense_extent, float("-inf"), big_extent)
        split = ((raw & SPLIT) != 0)[:, None]
        pure_parent = split & ((raw & CLONE) == 0)[:, None]
        child_raw = s2 / (0.8 * N)
        if not scene.use_factor_scaling:
            child_raw = torch.log(child_raw)
        batch = torch.cat([torch.where(pure_parent, child_raw, raw_s), torch.where(split, child_raw, raw_s)])
        s3 = activated(batch, torch.cat([raw_f, raw_f]) if raw_f is not None else None)
        P = raw_s.shape[0]
        sp_self, sp_child = s3[:P], s3[P:]
    code = classify_ref(scene.accum, scene.denom, s1, s2, sp_self, sp_child, opacity, max_grad, dense_extent, min_opacity,
                        big_extent)
    return code, s2


# ---- tests/golden/densify.npz (tests/golden/make_golden_densify.py)
def load_fixture():
    import os
    import numpy as np
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify.npz"), allow_pickle=False)
    cases = {}
    for name in d["cases"]:
        name = str(name)
        cases[name] = {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(name + "/")}
    return cases


def case_tensors(case, device):
    """Parameters and moments of a fixture case: the decision-relevant rows from the file, colours and every moment filled
    with unique values (they are copy-only)."""
    P = int(case["P"][0])
    t = lambda a: torch.from_numpy(a.copy()).to(device)         # noqa: E731
    uniq = lambda shape, base: (torch.arange(int(torch.Size(shape).numel()), dtype=torch.float32).reshape(shape) * 0.25 + base).to(device)  # noqa: E731
    params = {"xyz": t(case["in_xyz"]), "f_dc": uniq((P, 1, 3), 1000.0), "f_rest": uniq((P, 15, 3), 5000.0),
              "opacity": t(case["in_opacity"]), "scaling": t(case["in_scaling"]), "rotation": t(case["in_rotation"]),
              "scaling_factor": t(case["in_scaling_factor"]) if "in_scaling_factor" in case else None}
    moments = {k: (uniq(v.shape, 1e5 * (i + 1)), uniq(v.shape, 1e6 * (i + 1)))
               for i, (k, v) in enumerate(params.items()) if v is not None}
    return params, moments


def staged_from_case(case, device):
    params, moments = case_tensors(case, device)
    quant, factor = bool(case["quantization"][0]), bool(case["use_factor_scaling"][0])
    s = Staged(params, moments, torch.from_numpy(case["accum"].copy()).to(device), torch.from_numpy(case["denom"].copy()).to(device),
               torch.from_numpy(case["max_radii2D"].copy()).to(device), quantization=quant, use_factor_scaling=factor,
               percent_dense=float(case["percent_dense"][0]))
    for k in s.qa:
        if "qa_before_" + k in case:
            lo, hi, scale = case["qa_before_" + k]
            set_qa_state(s.qa[k], lo, hi, scale, int(case["qa_before_" + k + "_zp"][0]))
    return s


def run_case_method(scene, case, name, draws):
    """Call on `scene` (a Staged or a c3dgs_amd GaussianModel: same method names) what the fixture case `name` records."""
    max_grad, extent = float(case["max_grad"][0]), float(case["extent"][0])
    N = int(case["N"][0])
    accum, denom = scene.xyz_gradient_accum if hasattr(scene, "xyz_gradient_accum") else scene.accum, scene.denom
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    if name == "clone":
        return scene.densify_and_clone(grads, max_grad, extent)
    if name == "split":
        return scene.densify_and_split(grads, max_grad, extent, N, draws=draws)
    if name == "prune":
        return scene.prune_points(torch.from_numpy(case["prune_mask"].copy()).to(denom.device))
    return scene.densify_and_prune(max_grad, float(case["min_opacity"][0]), extent, int(case["max_screen_size"][0]) or None,
                                   draws=draws)
