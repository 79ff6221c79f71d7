"""The QAT getters and render glue of the reference's GaussianModel, fused on the device.

Mirrors of scene/gaussian_model.py:
    setup_functions / activations                 :54-77
    the FakeQuantize(dtype=qint8) module set      :109-134
    get_scaling ... get_opacity                   :213-267
    GaussianModel.render                          :766-886
    FakeQuantizationHalf                          :1405-1414
    save_ply / load / load_ply                    :324-503  (PLY IO in ply.py; distCUDA2 scales in knn.py)
    adaptive density control (non-indexed)        :288-290, :1061-1403  (csrc/densify.hip)
    densify_initial                               :1352-1389  (csrc/ray_fill.hip, knn.py)

The reference evaluates every getter with torch ops and seven torch.ao FakeQuantize modules: about a hundred small
launches and twenty host syncs per view (aminmax + float(scale) / int(zero_point) per module, one nonzero per
boolean-mask gather). Here the module state (min, max, scale, zero_point) lives in ONE device tensor that is never
read back, and an indexed QAT render is: visible flags + scan, ONE observe pass, ONE codebook launch, ONE compaction
launch, the rasterizer, and two backward launches (csrc/qat.hip). A single 4-byte device->host read (the visible count)
remains; it overlaps the observe / codebook kernels.
"""
import ctypes as C
import math

import torch

from . import _lib
from . import rasterizer as _rz
from . import rows as _rows
from ._lib import ptr as _ptr, stream as _stream
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, GaussianRasterizerIndexed

SLOTS = ("opacity", "scaling", "scaling_factor", "rotation", "features_dc", "features_rest")
_SLOT = {k: i for i, k in enumerate(SLOTS)}
AVERAGING_CONSTANT = 0.01       # MovingAverageMinMaxObserver default


class ColorMode:                # scene/gaussian_model.py:49-51
    NOT_INDEXED = 0
    ALL_INDEXED = 1


def new_fq_state(device, n=1):
    """[n,4] float32 rows {min_val=+inf, max_val=-inf, scale=1, zero_point=0 (int32 bits)} -- c3dgs_fq_state."""
    s = torch.zeros(n, 4, dtype=torch.float32, device=device)
    s[:, 0] = float("inf")
    s[:, 1] = float("-inf")
    s[:, 2] = 1.0
    return s


_WS = {}


def _workspace(device):
    dev = torch.device(device)
    ws = _WS.get(dev)
    if ws is None:
        ws = torch.empty(_lib.lib().c3dgs_qat_workspace_bytes(), dtype=torch.uint8, device=dev)
        _WS[dev] = ws
    return ws


class _Observer:
    """`module.activation_post_process` look-alike: min_val / max_val views of the device state."""

    def __init__(self, row):
        self._row = row

    @property
    def min_val(self):
        return self._row[0]

    @property
    def max_val(self):
        return self._row[1]

    averaging_constant = AVERAGING_CONSTANT
    quant_min, quant_max = -128, 127


class _FakeQuantizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module):
        xc = _lib.gpu_tensor(x, "FakeQuantize input")
        out = torch.empty_like(xc)
        row = module._row
        _lib.check(_lib.lib().c3dgs_fake_quantize(xc.numel(), xc.data_ptr(), row.data_ptr(), int(module.observer_enabled),
                                                  int(module.fake_quant_enabled), AVERAGING_CONSTANT, out.data_ptr(),
                                                  _workspace(xc.device).data_ptr(), _stream(xc.device)))
        ctx.enabled = int(module.fake_quant_enabled)
        ctx.save_for_backward(xc, row.clone())
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        x, row = ctx.saved_tensors
        gc = g.contiguous()
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().c3dgs_fake_quantize_backward(x.numel(), x.data_ptr(), row.data_ptr(), ctx.enabled, gc.data_ptr(),
                                                           dx.data_ptr(), _stream(x.device)))
        return dx, None


class FakeQuantize:
    """Device-resident stand-in for torch.ao.quantization.FakeQuantize(dtype=torch.qint8) as the reference builds it
    (scene/gaussian_model.py:109-118): MovingAverageMinMaxObserver, per-tensor affine, [-128, 127]. Same call and the
    same attribute names the reference touches; the state is one 16-byte row on the device."""

    quant_min, quant_max = -128, 127
    dtype = torch.qint8

    def __init__(self, dtype=torch.qint8, device="cuda", _row=None):
        if dtype != torch.qint8:
            raise RuntimeError("c3dgs_amd.model.FakeQuantize mirrors the reference's dtype=torch.qint8 modules only")
        self._row = _row if _row is not None else new_fq_state(device)[0]
        self.observer_enabled = True
        self.fake_quant_enabled = True
        self.activation_post_process = _Observer(self._row)

    def to(self, device):
        if torch.device(device) != self._row.device:
            self._row = self._row.to(device)
            self.activation_post_process = _Observer(self._row)
        return self

    @property
    def scale(self):
        return self._row[2:3]

    @property
    def zero_point(self):
        return self._row[3:4].view(torch.int32)

    def calculate_qparams(self):
        return self.scale, self.zero_point

    def enable_fake_quant(self, enabled=True):
        self.fake_quant_enabled = bool(enabled)
        return self

    def disable_fake_quant(self):
        return self.enable_fake_quant(False)

    def enable_observer(self, enabled=True):
        self.observer_enabled = bool(enabled)
        return self

    def disable_observer(self):
        return self.enable_observer(False)

    def __call__(self, x):
        if x.numel() == 0:
            return x
        return _FakeQuantizeFn.apply(x, self)

    forward = __call__


class FakeQuantizationHalf(torch.autograd.Function):
    """scene/gaussian_model.py:1405-1414: round through fp16, identity gradient."""

    @staticmethod
    def forward(_, x):
        return x.half().float()

    @staticmethod
    def backward(_, grad_output):
        return grad_output


# ----------------------------------------------------------------------------- fused getters
def _qat_params(model, state, *, xyz=None, opacity=None, scaling_factor=None, scaling=None, rotation=None, fdc=None,
                frest=None):
    q = _lib.QatParams()
    q.P = int((xyz if xyz is not None else opacity if opacity is not None else scaling_factor).shape[0]) \
        if (xyz is not None or opacity is not None or scaling_factor is not None) else 0
    q.GS = int((scaling if scaling is not None else rotation).shape[0]) if (scaling is not None or rotation is not None) else 0
    q.SHS = int(fdc.shape[0]) if fdc is not None else 0
    q.M = 1 + (int(frest.shape[1]) if frest is not None else 0)
    q.xyz, q.opacity, q.scaling_factor = _ptr(xyz), _ptr(opacity), _ptr(scaling_factor)
    q.scaling, q.rotation = _ptr(scaling), _ptr(rotation)
    q.features_dc = _ptr(fdc)
    q.features_rest = _ptr(frest) if (frest is not None and frest.numel() > 0) else None
    q.state = state.data_ptr()
    for i, k in enumerate(SLOTS):
        m = model._modules_qa[k]
        q.observer_enabled[i] = int(m.observer_enabled)
        q.fake_quant_enabled[i] = int(m.fake_quant_enabled)
    q.half_xyz = int(model.quantization)
    q.averaging_constant = AVERAGING_CONSTANT
    return q


class _QatGetters(torch.autograd.Function):
    """All getters of one render in one autograd node. Inputs that are None are skipped; `vis` is None (plain getters,
    every row) or (visible u8[P], rank i32[P], V)."""

    @staticmethod
    def forward(ctx, model, vis, sh_indices, g_indices, xyz, screenspace, opacity, scaling_factor, scaling, rotation, fdc,
                frest):
        lib = _lib.lib()
        raw = dict(xyz=xyz, opacity=opacity, scaling_factor=scaling_factor, scaling=scaling, rotation=rotation, fdc=fdc,
                   frest=frest)
        raw = {k: (None if v is None else _lib.gpu_tensor(v, k)) for k, v in raw.items()}
        anyt = next(v for v in raw.values() if v is not None)
        dev = anyt.device
        s = _stream(dev)
        q = _qat_params(model, model._fq_state, **raw)
        _lib.check(lib.c3dgs_qat_observe(C.byref(q), _workspace(dev).data_ptr(), s))
        state = model._fq_state.clone()                       # what the backward must see (the next view moves it)
        f32 = dict(dtype=torch.float32, device=dev)
        scales_n = torch.empty(q.GS, 3, **f32) if raw["scaling"] is not None else None
        rotations = torch.empty(q.GS, 4, **f32) if raw["rotation"] is not None else None
        shs = torch.empty(q.SHS, q.M, 3, **f32) if raw["fdc"] is not None else None
        if scales_n is not None or rotations is not None or shs is not None:
            _lib.check(lib.c3dgs_qat_codebooks(C.byref(q), _ptr(scales_n), _ptr(rotations), _ptr(shs), s))
        visible = rank = None
        V = q.P
        if vis is not None:
            visible, rank, V = vis
            V = int(V() if callable(V) else V)                # the one host read, deferred until here
        means3D = torch.empty(V, 3, **f32) if raw["xyz"] is not None else None
        # means2D only exists to carry a gradient back to `screenspace`: the rasterizer never reads its values
        means2D = torch.empty(V, 3, **f32) if screenspace is not None else None
        opac = torch.empty(V, 1, **f32) if raw["opacity"] is not None else None
        sfac = torch.empty(V, 1, **f32) if raw["scaling_factor"] is not None else None
        sh_out = torch.empty(V, dtype=torch.int64, device=dev) if (sh_indices is not None and vis is not None) else None
        g_out = torch.empty(V, dtype=torch.int64, device=dev) if (g_indices is not None and vis is not None) else None
        if q.P > 0 and (means3D is not None or opac is not None or sfac is not None or sh_out is not None):
            _lib.check(lib.c3dgs_qat_points(C.byref(q), _ptr(visible), _ptr(rank),
                                            _ptr(sh_indices) if sh_out is not None else None,
                                            _ptr(g_indices) if g_out is not None else None,
                                            _ptr(means3D), _ptr(opac), _ptr(sfac), _ptr(sh_out), _ptr(g_out), s))
        if vis is None:
            sh_out, g_out = sh_indices, g_indices
        ctx.model, ctx.P, ctx.has_screen = model, q.P, screenspace is not None
        ctx.flags = ([int(v) for v in q.observer_enabled], [int(v) for v in q.fake_quant_enabled], int(q.half_xyz))
        ctx.save_for_backward(state, visible, rank, *[raw[k] for k in ("xyz", "opacity", "scaling_factor", "scaling",
                                                                       "rotation", "fdc", "frest")])
        outs = (means3D, means2D, opac, sfac, scales_n, rotations, shs, sh_out, g_out)
        ctx.mark_non_differentiable(*[t for t in (sh_out, g_out) if t is not None and vis is not None])
        # without this, autograd hands backward zero-filled int64[V] "gradients" for the two index outputs on every call
        # (2 x 24 MB of fills at V = 3M); a differentiable output nobody used arrives as None and is filled below
        ctx.set_materialize_grads(False)
        ctx.V = V
        return outs

    @staticmethod
    def backward(ctx, g_m3, g_m2, g_op, g_sf, g_scales, g_rot, g_shs, _a, _b):
        lib = _lib.lib()
        state, visible, rank, xyz, opacity, sfac, scaling, rotation, fdc, frest = ctx.saved_tensors
        raw = dict(xyz=xyz, opacity=opacity, scaling_factor=sfac, scaling=scaling, rotation=rotation, fdc=fdc, frest=frest)
        q = _qat_params(ctx.model, state, **raw)
        for i in range(6):                                    # the flags as they were at forward time
            q.observer_enabled[i], q.fake_quant_enabled[i] = ctx.flags[0][i], ctx.flags[1][i]
        q.half_xyz = ctx.flags[2]
        anyt = next(v for v in raw.values() if v is not None)
        dev = anyt.device
        s = _stream(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad                           # (model, vis, sh_idx, g_idx, xyz, screen, op, sf, scal, rot, dc, rest)
        c = lambda t: None if t is None else t.contiguous()
        g_m3, g_m2, g_op, g_sf, g_scales, g_rot, g_shs = map(c, (g_m3, g_m2, g_op, g_sf, g_scales, g_rot, g_shs))
        P = ctx.P
        if g_m3 is None and xyz is not None and need[4]:
            g_m3 = torch.zeros(ctx.V, 3, **f32)
        if g_m2 is None and ctx.has_screen and need[5]:
            g_m2 = torch.zeros(ctx.V, 3, **f32)
        if g_op is None and opacity is not None and need[6]:
            g_op = torch.zeros(ctx.V, 1, **f32)
        if g_sf is None and sfac is not None and need[7]:
            g_sf = torch.zeros(ctx.V, 1, **f32)
        d_xyz = torch.empty(P, 3, **f32) if (xyz is not None and need[4]) else None
        d_screen = torch.empty(P, 3, **f32) if (ctx.has_screen and need[5]) else None
        d_op = torch.empty(P, 1, **f32) if (opacity is not None and need[6]) else None
        d_sf = torch.empty(P, 1, **f32) if (sfac is not None and need[7]) else None
        if P > 0 and any(t is not None for t in (d_xyz, d_screen, d_op, d_sf)):
            _lib.check(lib.c3dgs_qat_points_backward(C.byref(q), _ptr(visible), _ptr(rank), _ptr(g_m3), _ptr(g_m2), _ptr(g_op),
                                                     _ptr(g_sf), _ptr(d_xyz), _ptr(d_screen), _ptr(d_op), _ptr(d_sf), s))
        d_scaling = torch.empty_like(scaling) if (scaling is not None and need[8]) else None
        d_rot = torch.empty_like(rotation) if (rotation is not None and need[9]) else None
        want_sh = fdc is not None and (need[10] or need[11])
        d_dc = torch.empty_like(fdc) if want_sh else None
        d_rest = torch.empty_like(frest) if (want_sh and frest is not None) else None
        zeros = lambda like: torch.zeros_like(like)
        if d_scaling is not None and g_scales is None:
            d_scaling = zeros(scaling)
        if d_rot is not None and g_rot is None:
            d_rot = zeros(rotation)
        if want_sh and g_shs is None:
            d_dc, d_rest = zeros(fdc), (zeros(frest) if frest is not None else None)
        if (d_scaling is not None and g_scales is not None) or (d_rot is not None and g_rot is not None) or \
                (want_sh and g_shs is not None):
            _lib.check(lib.c3dgs_qat_codebooks_backward(
                C.byref(q), _ptr(g_scales) if d_scaling is not None else None, _ptr(g_rot) if d_rot is not None else None,
                _ptr(g_shs) if want_sh else None, _ptr(d_scaling), _ptr(d_rot), _ptr(d_dc), _ptr(d_rest), s))
        return (None, None, None, None, d_xyz, d_screen, d_op, d_sf, d_scaling, d_rot,
                d_dc if need[10] else None, d_rest if need[11] else None)


class PipelineParams:
    """The three switches GaussianModel.render reads from the reference's arguments.PipelineParams, and `antialiasing`."""

    def __init__(self, convert_SHs_python=False, compute_cov3D_python=False, debug=False, antialiasing=False):
        self.convert_SHs_python = convert_SHs_python
        self.compute_cov3D_python = compute_cov3D_python
        self.debug = debug
        self.antialiasing = antialiasing      # upstream 3DGS's switch (not in the reference): render(antialiasing=None) reads it


class GaussianModel:
    """Render-path mirror of scene/gaussian_model.py:GaussianModel (same constructor arguments, parameter attribute
    names, getters and render()). Parameters come from `load` (a trained .ply, a point cloud .ply, or a compressed .npz)
    or are plain tensors the caller assigns (`set_tensors`)."""

    def __init__(self, sh_degree, quantization=True, use_factor_scaling=True, device="cuda", is_splitted=True):
        self.is_splitted = is_splitted
        self.device = torch.device(device)
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self.quantization = quantization
        self.use_factor_scaling = use_factor_scaling
        self.color_index_mode = ColorMode.NOT_INDEXED
        self._xyz = self._features_dc = self._features_rest = self._scaling = self._rotation = self._opacity = None
        self._scaling_factor = None
        self._feature_indices = self._gaussian_indices = None
        self._fq_state = new_fq_state(self.device, len(SLOTS))
        self._modules_qa = {k: FakeQuantize(_row=self._fq_state[i]) for i, k in enumerate(SLOTS)}
        self.opacity_qa = self._modules_qa["opacity"]
        self.scaling_qa = self._modules_qa["scaling"]
        self.scaling_factor_qa = self._modules_qa["scaling_factor"]
        self.rotation_qa = self._modules_qa["rotation"]
        self.features_dc_qa = self._modules_qa["features_dc"]
        self.features_rest_qa = self._modules_qa["features_rest"]
        self.xyz_qa = FakeQuantizationHalf.apply
        if not quantization:                                    # gaussian_model.py:120-134
            for k in ("features_dc", "features_rest", "scaling", "scaling_factor", "rotation"):
                self._modules_qa[k].disable_fake_quant()
                self._modules_qa[k].disable_observer()
            self.xyz_qa = lambda x: x
        self._count_host = None
        # the 3D smoothing filter (compute_3D_filter): f32 [P] or None; stale: the model had one and rows were created since
        self.filter_3D = None
        self._filter_3D_stale = False
        self.spatial_lr_scale = 0.0                             # set by the scene loader in the reference (gaussian_model.py:286)
        self.optimizer = None
        self.xyz_scheduler_args = None
        # activations, gaussian_model.py:54-77
        if use_factor_scaling:
            self.scaling_activation = lambda x: torch.nn.functional.normalize(torch.nn.functional.relu(x))
            self.scaling_factor_activation = torch.exp
        else:
            self.scaling_activation = torch.exp
        self.opacity_activation = torch.sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    # ---- parameters
    def set_tensors(self, *, xyz, features_dc, features_rest, scaling, rotation, opacity, scaling_factor=None,
                    feature_indices=None, gaussian_indices=None, active_sh_degree=None, requires_grad=True):
        """Install the learnable tensors (shapes as in the reference: xyz [P,3], features_dc [S,1,3], features_rest
        [S,M-1,3], scaling [G,3], rotation [G,4], opacity [P,1], scaling_factor [P,1]; S = G = P when not indexed)."""
        def param(t):
            return None if t is None else t.detach().to(self.device, torch.float32).contiguous().requires_grad_(requires_grad)
        self._xyz, self._features_dc, self._features_rest = param(xyz), param(features_dc), param(features_rest)
        self._scaling, self._rotation, self._opacity = param(scaling), param(rotation), param(opacity)
        self._scaling_factor = param(scaling_factor) if self.use_factor_scaling else None
        if self.use_factor_scaling and self._scaling_factor is None:
            raise RuntimeError("use_factor_scaling=True needs scaling_factor")
        self._feature_indices = None if feature_indices is None else feature_indices.to(self.device, torch.int64).contiguous()
        self._gaussian_indices = None if gaussian_indices is None else gaussian_indices.to(self.device, torch.int64).contiguous()
        self.color_index_mode = ColorMode.ALL_INDEXED if feature_indices is not None else ColorMode.NOT_INDEXED
        self.active_sh_degree = self.max_sh_degree if active_sh_degree is None else active_sh_degree
        self.filter_3D, self._filter_3D_stale = None, False
        return self

    def parameters(self):
        return [t for t in (self._xyz, self._features_dc, self._features_rest, self._scaling, self._scaling_factor,
                            self._rotation, self._opacity) if t is not None]

    @property
    def is_gaussian_indexed(self):
        return self._gaussian_indices is not None

    @property
    def is_color_indexed(self):
        return self._feature_indices is not None

    # ---- getters (gaussian_model.py:213-267). Each access runs its module's observer once, as in the reference.
    def _get(self, **raw):
        return _QatGetters.apply(self, None, None, None, raw.get("xyz"), None, raw.get("opacity"), raw.get("scaling_factor"),
                                 raw.get("scaling"), raw.get("rotation"), raw.get("fdc"), raw.get("frest"))

    @property
    def get_xyz(self):
        return self.xyz_qa(self._xyz)

    @property
    def get_opacity(self):
        return self._get(opacity=self._opacity)[2]

    @property
    def get_scaling_normalized(self):
        if self.use_factor_scaling:
            return self._get(scaling=self._scaling)[4]
        return self.scaling_qa(self.scaling_activation(self._scaling))

    @property
    def get_scaling_factor(self):
        if self._scaling_factor is None:
            return 1.0
        return self._get(scaling_factor=self._scaling_factor)[3]

    @property
    def get_scaling(self):
        scaling_n = self.get_scaling_normalized
        if self._scaling_factor is None:
            return scaling_n
        factor = self.get_scaling_factor
        return factor * (scaling_n[self._gaussian_indices] if self.is_gaussian_indexed else scaling_n)

    @property
    def _rotation_post_activation(self):
        return self._get(rotation=self._rotation)[5]

    @property
    def get_rotation(self):
        r = self._rotation_post_activation
        return r[self._gaussian_indices] if self.is_gaussian_indexed else r

    @property
    def _get_features_raw(self):
        return self._get(fdc=self._features_dc, frest=self._features_rest)[6]

    @property
    def get_features(self):
        f = self._get_features_raw
        return f[self._feature_indices] if self.color_index_mode == ColorMode.ALL_INDEXED else f

    def get_covariance(self, scaling_modifier=1, strip_sym=True):
        return _covariance(self.get_scaling, scaling_modifier, self.get_rotation, strip_sym)

    def get_normalized_covariance(self, scaling_modifier=1, strip_sym=True):
        return _covariance(self.get_scaling_normalized, scaling_modifier, self.get_rotation, strip_sym)

    # ---- the 3D smoothing filter (Mip-Splatting; csrc/filter3d.hip, c3dgs_amd/filter3d.py; not in the reference)
    def compute_3D_filter(self, cameras, table=None):
        """Sets `filter_3D` (f32 [P], no grad) over `cameras`: per Gaussian sqrt(0.2) x its smallest depth among the cameras that
        see it / the largest focal length (filter3d.compute; the nearest seen distance stands in for a Gaussian no camera sees).
        From then on render() draws every Gaussian with Sigma + f^2 I and the matching opacity (filter3d.apply), until
        clear_3D_filter(). -> the `seen` flags (bool [P]). Building the camera table reads every camera's pose on the host (one
        device -> host copy per camera); a caller that recomputes over the same cameras passes the `table` of
        filter3d.camera_table(cameras, device) instead and the call is then stream-ordered, without a host read."""
        from . import filter3d
        with torch.no_grad():
            if table is None:
                table = filter3d.camera_table(cameras, self.device)
            self.filter_3D, seen = filter3d.compute(self._xyz.detach(), table)
        self._filter_3D_stale = False
        return seen

    def clear_3D_filter(self):
        self.filter_3D, self._filter_3D_stale = None, False

    def _carry_3D_filter(self, rows):
        """a pure selection or permutation of the rows (a mask or an index tensor) takes the filter along"""
        if self.filter_3D is not None:
            rows = rows.to(self.device)
            rows = rows.bool() if rows.dtype in (torch.bool, torch.uint8) else rows.long()
            self.filter_3D = self.filter_3D[rows].contiguous()

    def _drop_3D_filter(self):
        """rows were created: their filter values do not exist, so render() refuses until compute_3D_filter has run again"""
        if self.filter_3D is not None:
            self.filter_3D, self._filter_3D_stale = None, True

    def _checked_3D_filter(self, pipe, cov3d, viewpoint_camera):
        """render()'s filter, or None without one; raises for what the filtered path does not cover"""
        if self._filter_3D_stale:
            raise RuntimeError("render(): rows were added since the 3D filter was computed; call compute_3D_filter(cameras) again "
                               "(or clear_3D_filter())")
        if self.filter_3D is None:
            return None
        if pipe.compute_cov3D_python:
            raise NotImplementedError("render() with a 3D filter: compute_cov3D_python is not covered")
        if viewpoint_camera.extrinsic_vector.requires_grad:
            raise ValueError("render() with a 3D filter: the gradient to a camera pose that requires grad is not covered")
        if self.filter_3D.shape[0] != self._xyz.shape[0]:
            raise RuntimeError(f"render(): filter_3D has {self.filter_3D.shape[0]} rows for {self._xyz.shape[0]} Gaussians; call "
                               "compute_3D_filter(cameras) again")
        return self.filter_3D

    @property
    def get_scaling_with_3D_filter(self):
        """sqrt(s^2 + f^2) of the activated scales, for inspection (torch ops; render() uses filter3d.apply)"""
        s = self.get_scaling
        return s if self.filter_3D is None else torch.sqrt(s * s + (self.filter_3D * self.filter_3D)[:, None])

    @property
    def get_opacity_with_3D_filter(self):
        """o x sqrt(prod_k s_k^2 / (s_k^2 + f^2)), for inspection (torch ops; render() uses filter3d.apply)"""
        o = self.get_opacity
        if self.filter_3D is None:
            return o
        s2, f2 = self.get_scaling ** 2, (self.filter_3D * self.filter_3D)[:, None]
        r = torch.where(f2 == 0, torch.ones_like(s2), s2 / (s2 + f2))
        return o * torch.sqrt(r[:, 0] * r[:, 1] * r[:, 2])[:, None]

    # ---- what compress_gaussians needs (gaussian_model.py:1027-1059)
    def mask_splats(self, mask):
        with torch.no_grad():
            self._carry_3D_filter(mask)
            keep = lambda t: None if t is None else t.detach()[mask].contiguous().requires_grad_(t.requires_grad)
            self._xyz, self._opacity, self._scaling_factor = keep(self._xyz), keep(self._opacity), keep(self._scaling_factor)
            if self.is_color_indexed:
                self._feature_indices = self._feature_indices[mask].contiguous()
            else:
                self._features_dc, self._features_rest = keep(self._features_dc), keep(self._features_rest)
            if self.is_gaussian_indexed:
                self._gaussian_indices = self._gaussian_indices[mask].contiguous()
            else:
                self._scaling, self._rotation = keep(self._scaling), keep(self._rotation)

    def set_color_indexed(self, features, indices):
        self._feature_indices = indices.detach().to(self.device, torch.int64).contiguous()
        self._features_dc = features[:, :1].detach().contiguous().requires_grad_(True)
        self._features_rest = features[:, 1:].detach().contiguous().requires_grad_(True)
        self.color_index_mode = ColorMode.ALL_INDEXED

    def set_gaussian_indexed(self, rotation, scaling, indices):
        self._gaussian_indices = indices.detach().to(self.device, torch.int64).contiguous()
        self._rotation = rotation.detach().contiguous().requires_grad_(True)
        self._scaling = scaling.detach().contiguous().requires_grad_(True)

    def zero_grad(self):
        for t in self.parameters():
            t.grad = None

    # ---- on-disk payload (gaussian_model.py:505-623 save_npz, :625-720 load_npz, :997-1023 _sort_morton)
    def _sort_morton(self):
        from . import encode
        with torch.no_grad():
            order = encode.morton_order(self._xyz.detach())
            self._carry_3D_filter(order)
            take = lambda t: None if t is None else t.detach()[order].contiguous().requires_grad_(t.requires_grad)
            self._xyz, self._opacity, self._scaling_factor = take(self._xyz), take(self._opacity), take(self._scaling_factor)
            if self.is_color_indexed:
                self._feature_indices = self._feature_indices[order].contiguous()
            else:
                self._features_rest, self._features_dc = take(self._features_rest), take(self._features_dc)
            if self.is_gaussian_indexed:
                self._gaussian_indices = self._gaussian_indices[order].contiguous()
            else:
                self._scaling, self._rotation = take(self._scaling), take(self._rotation)

    def quantized_payload(self):
        """int8 codes of every fake-quantised tensor with the modules' current scale / zero_point, as
        torch.quantize_per_tensor(...).int_repr() gives them in save_npz: ONE launch for all six tensors."""
        dev = self.device
        i8 = lambda t: None if t is None else torch.empty(t.shape, dtype=torch.int8, device=dev)
        raw = dict(opacity=self._opacity, scaling=self._scaling, scaling_factor=self._scaling_factor, rotation=self._rotation,
                   fdc=self._features_dc, frest=self._features_rest)
        raw = {k: (None if v is None else v.detach().contiguous()) for k, v in raw.items()}
        out = {k: i8(v) for k, v in raw.items()}
        q = _qat_params(self, self._fq_state, **raw)
        _lib.check(_lib.lib().c3dgs_qat_quantize(C.byref(q), int(not self.use_factor_scaling), _ptr(out["opacity"]),
                                                 _ptr(out["scaling"]), _ptr(out["scaling_factor"]), _ptr(out["rotation"]),
                                                 _ptr(out["fdc"]), _ptr(out["frest"]), _stream(dev)))
        return out

    def save_npz(self, path, compress=True, half_precision=False, sort_morton=False):
        """Same keys, dtypes and shapes as the reference writes, so its load_npz / the web viewer read the file."""
        import os
        import numpy as np
        with torch.no_grad():
            if sort_morton:
                self._sort_morton()
            if isinstance(path, str):
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            dtype = torch.half if half_precision else torch.float32
            d = {"quantization": self.quantization}
            host = lambda t: t.detach().cpu().numpy()
            if self.quantization:
                codes = self.quantized_payload()
                d["xyz"] = host(self._xyz.detach().half())
                for key, name, slot in (("features_dc", "fdc", "features_dc"), ("features_rest", "frest", "features_rest"),
                                        ("opacity", "opacity", "opacity"), ("scaling", "scaling", "scaling"),
                                        ("scaling_factor", "scaling_factor", "scaling_factor"),
                                        ("rotation", "rotation", "rotation")):
                    if codes[name] is None:
                        continue
                    mod = self._modules_qa[slot]
                    d[key] = host(codes[name])
                    d[key + "_scale"] = host(mod.scale)
                    d[key + "_zero_point"] = host(mod.zero_point)
            else:
                d["xyz"] = host(self._xyz)
                d["features_dc"], d["features_rest"] = host(self._features_dc), host(self._features_rest)
                d["opacity"] = host(self._opacity.detach().to(dtype))
                d["scaling"] = host(self._scaling.detach().to(dtype))
                if self._scaling_factor is not None:
                    d["scaling_factor"] = host(self._scaling_factor.detach().to(dtype))
                d["rotation"] = host(self._rotation.detach().to(dtype))
            if self.is_color_indexed:
                d["feature_indices"] = host(self._feature_indices.int())
            if self.is_gaussian_indexed:
                d["gaussian_indices"] = host(self._gaussian_indices.int())
            # key order of the reference's file
            order = ["quantization", "xyz", "features_dc", "features_dc_scale", "features_dc_zero_point", "features_rest",
                     "features_rest_scale", "features_rest_zero_point", "opacity", "opacity_scale", "opacity_zero_point",
                     "feature_indices", "gaussian_indices", "scaling", "scaling_scale", "scaling_zero_point",
                     "scaling_factor", "scaling_factor_scale", "scaling_factor_zero_point", "rotation", "rotation_scale",
                     "rotation_zero_point"]
            if self.filter_3D is not None:                      # behind the reference's keys: its loader never asks for it
                d["filter_3D"] = host(self.filter_3D.to(dtype))
                order.append("filter_3D")
            (np.savez_compressed if compress else np.savez)(path, **{k: d[k] for k in order if k in d})

    def load_npz(self, path, override_quantization=False):
        import numpy as np
        sd = np.load(path)                                      # plain arrays only (allow_pickle stays False)
        quantization = bool(sd["quantization"])
        if not override_quantization and self.quantization != quantization:
            print("WARNING: model is not quantisation aware but loaded model is")
        if override_quantization:
            self.quantization = quantization
        dev = self.device
        par = lambda t: t.to(dev, torch.float32).contiguous().requires_grad_(True)

        def dequant(key, slot):
            qv = torch.from_numpy(sd[key]).int().to(dev)
            scale = torch.from_numpy(sd[key + "_scale"]).to(dev)
            zp = torch.from_numpy(sd[key + "_zero_point"]).to(dev)
            val = (qv - zp) * scale
            row = self._modules_qa[slot]._row
            row[0], row[1], row[2] = val.min(), val.max(), scale.reshape(-1)[0]
            row[3:4].view(torch.int32)[0] = zp.reshape(-1)[0].int()
            return val

        self._xyz = par(torch.from_numpy(sd["xyz"]).float())
        if quantization:
            self._features_rest = par(dequant("features_rest", "features_rest"))
            self._features_dc = par(dequant("features_dc", "features_dc"))
            op = dequant("opacity", "opacity")
            self._opacity = par(torch.log(op / (1 - op)))       # inverse_sigmoid
            sc = dequant("scaling", "scaling")
            self._scaling = par(sc if self.use_factor_scaling else torch.log(sc))
            self._scaling_factor = par(dequant("scaling_factor", "scaling_factor")) if "scaling_factor" in sd else None
            self._rotation = par(dequant("rotation", "rotation"))
        else:
            self._features_dc, self._features_rest = par(torch.from_numpy(sd["features_dc"]).float()), \
                par(torch.from_numpy(sd["features_rest"]).float())
            self._opacity = par(torch.from_numpy(sd["opacity"]).float())
            self._scaling_factor = par(torch.from_numpy(sd["scaling_factor"]).float()) if "scaling_factor" in sd else None
            self._scaling = par(torch.from_numpy(sd["scaling"]).float())
            self._rotation = par(torch.from_numpy(sd["rotation"]).float())
        self._feature_indices = torch.from_numpy(sd["feature_indices"]).long().to(dev) if "feature_indices" in sd else None
        self._gaussian_indices = torch.from_numpy(sd["gaussian_indices"]).long().to(dev) if "gaussian_indices" in sd else None
        self.color_index_mode = ColorMode.ALL_INDEXED if self._feature_indices is not None else ColorMode.NOT_INDEXED
        self.active_sh_degree = self.max_sh_degree
        self.filter_3D = torch.from_numpy(sd["filter_3D"]).to(dev, torch.float32).contiguous() if "filter_3D" in sd else None
        self._filter_3D_stale = False
        return self

    # ---- PLY files (gaussian_model.py:324-387 save_ply, :389-396 load, :398-503 load_ply)
    def _ply_attributes(self):                                  # construct_list_of_attributes, :324-337
        names = ["x", "y", "z", "nx", "ny", "nz"]
        names += [f"f_dc_{i}" for i in range(self._features_dc.shape[1] * self._features_dc.shape[2])]
        names += [f"f_rest_{i}" for i in range(self._features_rest.shape[1] * self._features_rest.shape[2])]
        names.append("opacity")
        names += [f"scale_{i}" for i in range(self._scaling.shape[1])]
        names += [f"rot_{i}" for i in range(self._rotation.shape[1])]
        return names

    def save_ply(self, path, fuse_filter=False):
        """The standard 3DGS PLY every viewer reads: dense per-Gaussian attributes (an indexed model is expanded),
        raw opacity, log of the activated scale (scale factor folded in), activated rotation, zero normals.
        A model with a 3D filter appends it as the property `filter_3D`, which load_ply restores; with fuse_filter=True the
        filter is baked in instead (scale sqrt(s^2 + f^2), opacity logit(o coef)): a standard PLY for viewers that know nothing of
        the filter, which renders like the filtered model when the rotations are unit quaternions."""
        import os
        import numpy as np
        from . import ply
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        if self.is_gaussian_indexed or self.is_color_indexed:
            print("WARNING: indexed colors/gaussians are not supported for ply files and are converted to dense attributes")
        with torch.no_grad():
            color = self.get_features.detach()                 # getter order of the reference: features, scaling, rotation
            xyz = self._xyz.detach().cpu().numpy()
            f_dc = color[:, :1].transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
            f_rest = color[:, 1:].transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
            opacities = self._opacity.detach().cpu().numpy()
            scale = torch.log(self.get_scaling.detach()).cpu().numpy()   # scaling_factor_inverse / scaling_inverse = log
            rotation = self.get_rotation.detach().cpu().numpy()
            names = self._ply_attributes()
            extra = ()
            if self.filter_3D is not None and fuse_filter:
                o = self.get_opacity_with_3D_filter.detach().double()
                opacities = torch.log(o / (1 - o)).float().cpu().numpy()
                scale = torch.log(self.get_scaling_with_3D_filter.detach()).cpu().numpy()
            elif self.filter_3D is not None:
                names, extra = names + ["filter_3D"], (self.filter_3D[:, None].cpu().numpy(),)
        attributes = np.concatenate((xyz, np.zeros_like(xyz), f_dc, f_rest, opacities, scale, rotation) + extra, axis=1)
        ply.write_ply(path, {name: attributes[:, k] for k, name in enumerate(names)})

    def load(self, path, override_quantization=False):
        import os
        ext = os.path.splitext(path)[1]
        if ext == ".ply":
            return self.load_ply(path)
        if ext == ".npz":
            return self.load_npz(path, override_quantization)
        raise NotImplementedError(f"file ending '{ext}' not supported")

    def load_ply(self, path):
        """A trained 3DGS PLY, or a point cloud (x y z [nx ny nz] red green blue): missing opacity -> logit(0.1), missing
        scales -> log(sqrt(max(distCUDA2(xyz), 1e-7))) per axis, missing rotation -> identity (gaussian_model.py:398-503)."""
        import numpy as np
        from . import ply
        from .knn import distCUDA2
        v = ply.read_ply(path)
        keys = list(v)
        dev = self.device
        xyz = np.stack((v["x"], v["y"], v["z"]), axis=1)
        n = xyz.shape[0]
        if "opacity" in keys:
            opacities = v["opacity"][..., None]
        else:
            x = 0.1 * np.ones((n, 1))
            opacities = np.log(x / (1 - x))
        features_dc = np.zeros((n, 3, 1))
        color_codes = ["red", "green", "blue"] if "red" in keys else ["f_dc_0", "f_dc_1", "f_dc_2"]
        for i, name in enumerate(color_codes):
            if name not in v:
                raise ValueError(f"{path}: vertex element has no '{name}' property")
            features_dc[:, i, 0] = v[name]
        if "red" in keys:
            features_dc = (features_dc / 255.0 - 0.5) / 0.28209479177387814      # RGB2SH, in float64 as numpy does
        rest = sorted((k for k in keys if k.startswith("f_rest_")), key=lambda k: int(k.split("_")[-1]))
        if rest:
            degree = {3 * ((d + 1) ** 2 - 1): d for d in range(self.max_sh_degree + 1)}
            if degree.get(len(rest)) is None:
                raise ValueError(f"{path}: {len(rest)} f_rest_* properties match no SH degree <= {self.max_sh_degree}")
            self.active_sh_degree = degree[len(rest)]
            features_extra = np.zeros((n, len(rest)))
            for i, name in enumerate(rest):
                features_extra[:, i] = v[name]
            features_extra = features_extra.reshape((n, 3, len(rest) // 3))
        else:
            self.active_sh_degree = 0
            features_extra = np.zeros((n, 3, (self.max_sh_degree + 1) ** 2 - 1))
        scale_names = sorted((k for k in keys if k.startswith("scale_") and not k.startswith("scale_factor")),
                             key=lambda k: int(k.split("_")[-1]))
        if scale_names:
            scales = np.zeros((n, len(scale_names)))
            for i, name in enumerate(scale_names):
                scales[:, i] = v[name]
            scaling = torch.tensor(scales, dtype=torch.float, device=dev)
        else:
            dist2 = torch.clamp_min(distCUDA2(torch.from_numpy(xyz).float().to(dev)), 0.0000001)
            scaling = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rot_names = sorted((k for k in keys if k.startswith("rot")), key=lambda k: int(k.split("_")[-1]))
        if rot_names:
            rots = np.zeros((n, len(rot_names)))
            for i, name in enumerate(rot_names):
                rots[:, i] = v[name]
        else:
            rots = np.zeros((n, 4))
            rots[:, 0] = 1
        par = lambda t: t.detach().contiguous().requires_grad_(True)
        self._xyz = par(torch.tensor(xyz, dtype=torch.float, device=dev))
        self._features_dc = par(torch.tensor(features_dc, dtype=torch.float, device=dev).transpose(1, 2))
        self._features_rest = par(torch.tensor(features_extra, dtype=torch.float, device=dev).transpose(1, 2))
        self._opacity = par(torch.tensor(opacities, dtype=torch.float, device=dev))
        if self.use_factor_scaling:
            scaling = torch.exp(scaling)
            norm = scaling.norm(2, -1, keepdim=True)
            self._scaling = par(scaling / norm)
            self._scaling_factor = par(torch.log(norm))
        else:
            self._scaling = par(scaling)
            self._scaling_factor = None
        self._rotation = par(torch.tensor(rots, dtype=torch.float, device=dev))
        self._feature_indices = self._gaussian_indices = None
        self.color_index_mode = ColorMode.NOT_INDEXED
        self.max_radii2D = torch.zeros(n, device=dev)
        self.filter_3D = torch.tensor(v["filter_3D"], dtype=torch.float, device=dev).contiguous() if "filter_3D" in keys else None
        self._filter_3D_stale = False
        return self

    # ---- optimizer plumbing of the fine-tuning loop (gaussian_model.py:292-322)
    def training_setup(self, training_args, optimizer_type=None):
        """Same parameter groups, names and learning rates as the reference; the optimizer is the fused Adam
        (c3dgs_amd.optim.Adam, one launch for all groups) instead of torch.optim.Adam(l, lr=0.0, eps=1e-15).

        `optimizer_type` (None: training_args.optimizer_type, "default" where it has none): "sparse_adam" (not in the reference;
        upstream 3DGS's accelerated optimizer) builds optim.SparseGaussianAdam over the same groups, each flagged per-Gaussian, so
        that step(visibility) updates only the rows a view saw. Non-indexed models only: the rows of a codebook are shared
        between Gaussians, there is no per-Gaussian row to skip."""
        from . import optim
        if optimizer_type is None:
            optimizer_type = getattr(training_args, "optimizer_type", "default")
        if optimizer_type not in ("default", "sparse_adam"):
            raise ValueError(f"training_setup: optimizer_type must be 'default' or 'sparse_adam', not {optimizer_type!r}")
        if optimizer_type == "sparse_adam" and (self.is_color_indexed or self.is_gaussian_indexed):
            raise NotImplementedError("training_setup: optimizer_type='sparse_adam' needs a non-indexed model (codebook rows are "
                                      "shared between Gaussians)")
        self.percent_dense = training_args.percent_dense
        n = self._xyz.shape[0]
        self.xyz_gradient_accum = torch.zeros((n, 1), device=self.device)
        self.denom = torch.zeros((n, 1), device=self.device)
        groups = [
            {"params": [self._xyz], "lr": training_args.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": training_args.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": training_args.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": training_args.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": training_args.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": training_args.rotation_lr, "name": "rotation"},
        ]
        if self._scaling_factor is not None:
            groups.append({"params": [self._scaling_factor], "lr": training_args.scaling_lr, "name": "scaling_factor"})
        if optimizer_type == "sparse_adam":
            for g in groups:
                g["per_gaussian"] = True
            self.optimizer = optim.SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
        else:
            self.optimizer = optim.Adam(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(
            lr_init=training_args.position_lr_init * self.spatial_lr_scale,
            lr_final=training_args.position_lr_final * self.spatial_lr_scale,
            lr_delay_mult=training_args.position_lr_delay_mult, max_steps=training_args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for param_group in self.optimizer.param_groups:
            if param_group["name"] == "xyz":
                lr = self.xyz_scheduler_args(iteration)
                param_group["lr"] = lr
                return lr

    # ---- adaptive density control (gaussian_model.py:288-290, :1061-1403), non-indexed models; csrc/densify.hip
    _GROUPS = (("xyz", "_xyz", _lib.ROLE_XYZ), ("f_dc", "_features_dc", 0), ("f_rest", "_features_rest", 0),
               ("opacity", "_opacity", 0), ("scaling", "_scaling", _lib.ROLE_SCALING), ("rotation", "_rotation", 0),
               ("scaling_factor", "_scaling_factor", 0))

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def _dense_only(self, what):
        if self._feature_indices is not None or self._gaussian_indices is not None:
            raise NotImplementedError(f"c3dgs_amd: {what} supports non-indexed models only (the reference's index remapping in "
                                      "prune_points is not mirrored here: prune_points_indexed prunes an indexed model, "
                                      "to_unindexed converts it)")

    def _density_stats(self):
        """xyz_gradient_accum / denom / max_radii2D of the current length (training_setup and load_ply create them; a model
        filled with set_tensors gets them here)."""
        n = self._xyz.shape[0]
        for name, shape in (("xyz_gradient_accum", (n, 1)), ("denom", (n, 1)), ("max_radii2D", (n,))):
            t = getattr(self, name, None)
            if t is None or tuple(t.shape) != shape or t.device != self._xyz.device:
                setattr(self, name, torch.zeros(shape, device=self.device))
        return self.xyz_gradient_accum, self.denom, self.max_radii2D

    def add_densification_stats(self, viewspace_point_tensor, update_filter, radii=None):
        """:1399-1402, and with `radii` the max_radii2D update of train.py:105, in one launch that neither allocates nor
        synchronises. `update_filter`: bool [P]; `radii`: int32 [P] (per Gaussian, like the filter)."""
        self._dense_only("add_densification_stats")
        accum, denom, max_radii = self._density_stats()
        grad = viewspace_point_tensor.grad
        P = self._xyz.shape[0]
        if grad is None or tuple(grad.shape) != (P, 3) or update_filter.shape[0] != P:
            raise RuntimeError("add_densification_stats: viewspace gradient [P,3] and filter [P] of the model's length are needed")
        grad = _lib.gpu_tensor(grad, "viewspace gradient")
        flt = update_filter.contiguous()
        if flt.dtype == torch.bool:
            flt = flt.view(torch.uint8)
        elif flt.dtype != torch.uint8:
            raise RuntimeError("update_filter must be a bool (or uint8) tensor")
        if radii is not None:
            if radii.dtype != torch.int32 or radii.shape[0] != P:
                raise RuntimeError("radii must be the rasterizer's int32 [P] tensor")
            radii = radii.contiguous()
        _lib.check(_lib.lib().c3dgs_densify_stats(P, grad.data_ptr(), flt.data_ptr(), _ptr(radii), accum.data_ptr(),
                                                  denom.data_ptr(), max_radii.data_ptr() if radii is not None else None,
                                                  _stream(self.device)))

    def _activated_scaling(self, raw, factor):
        """get_scaling (:214-222) on explicit raw rows: one observer access per module, as the property."""
        if self.use_factor_scaling:
            scaling_n = self._get(scaling=raw)[4]
            return self._get(scaling_factor=factor)[3] * scaling_n
        return self.scaling_qa(self.scaling_activation(raw))

    def _read_host(self, t):
        """The one blocking device->host read of a rebuild: a small integer tensor (the four int32 totals of a plan, the two
        int64 of relocate_gs) -> its Python ints, through a pinned buffer per dtype (kept on the model), a non-blocking copy and
        an event."""
        bufs = self.__dict__.setdefault("_host_bufs", {})
        host = bufs.get(t.dtype)
        if host is None or host.numel() < t.numel():
            host = bufs[t.dtype] = torch.empty(t.numel(), dtype=t.dtype).pin_memory()
        host = host[:t.numel()]
        host.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        ev.synchronize()
        return host.tolist()

    def _row_table(self, n_out, attrs, roles):
        """A rows.RowTable (out of place to `n_out` rows; None: in place) over the parameters named by `attrs`, each with the
        moments the optimizer holds for it; roles: {attr: role}, copy where it has none."""
        tab = _rows.RowTable(self.device, n_out)
        for attr in attrs:
            old = getattr(self, attr)
            if old is not None:
                tab.add(old, roles.get(attr, _lib.ROLE_COPY), attr, self.optimizer.state.get(old) if self.optimizer is not None else None)
        return tab

    def plan_rows(self, code, N=2):
        """code uint8[P] (bits: include/c3dgs_hip.h C3DGS_ROW_*) -> (src int32[P_new], kind uint8[P_new], draw_row int32[P_new],
        (kept, clones, S, parents with surviving children)). One host read."""
        lib = _lib.lib()
        dev = self.device
        P = int(code.shape[0])
        s = _stream(dev)
        ws = torch.empty(max(int(lib.c3dgs_rows_plan_workspace_bytes(P)), 256), dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.c3dgs_rows_plan(P, _ptr(code), N, 0, None, None, None, totals.data_ptr(), ws.data_ptr(), s))
        K, Cn, S, CK = self._read_host(totals)
        P_new = K + Cn + N * CK
        src = torch.empty(P_new, dtype=torch.int32, device=dev)
        kind = torch.empty(P_new, dtype=torch.uint8, device=dev)
        draw_row = torch.empty(P_new, dtype=torch.int32, device=dev)
        if P_new > 0:
            _lib.check(lib.c3dgs_rows_plan(P, _ptr(code), N, P_new, src.data_ptr(), kind.data_ptr(), draw_row.data_ptr(),
                                           totals.data_ptr(), ws.data_ptr(), s))
        return src, kind, draw_row, (K, Cn, S, CK)

    def _rebuild(self, code, N=2, std=None, draws=None, carry_stats=False):
        """plan -> one host read -> _apply_plan. Returns (src, kind, draw_row, totals)."""
        src, kind, draw_row, tot = self.plan_rows(code, N)
        K, Cn, S, CK = tot
        self._apply_plan(src, kind, draw_row, K + Cn + N * CK, N, S, std=std, draws=draws, carry_stats=carry_stats)
        return src, kind, draw_row, tot

    def _apply_plan(self, src, kind, draw_row, P_new, N=2, S=0, std=None, draws=None, carry_stats=False, new_xyz=None):
        """A given plan (include/c3dgs_hip.h c3dgs_rows_apply) -> allocate every new tensor once -> ONE apply launch -> install
        parameters and optimizer state (cat_tensors_to_optimizer / _prune_optimizer, :1081-1099, :1161-1185: `step` kept,
        moments of surviving originals copied, zero for new rows). `new_xyz(xyz_out)`, if given, runs between the launch and
        the install and overwrites positions in the new xyz tensor."""
        lib = _lib.lib()
        dev = self.device
        P = self._xyz.shape[0]
        accum, denom, max_radii = self._density_stats()
        if S > 0 and std is None:
            raise RuntimeError("split rows need their activated scales")
        if draws is None:
            draws = torch.randn((N * S, 3), device=dev)     # torch.normal(mean, std) is randn * std + mean (:1242)
        if tuple(draws.shape) != (N * S, 3):
            raise RuntimeError(f"draws must be [N*S, 3] = [{N * S}, 3] unit normals, got {tuple(draws.shape)}")
        draws = _lib.gpu_tensor(draws, "draws")
        std = None if std is None else _lib.gpu_tensor(std, "std")
        rotation = _lib.gpu_tensor(self._rotation.detach(), "rotation")
        tab = self._row_table(P_new, [attr for _, attr, _ in self._GROUPS], {attr: role for _, attr, role in self._GROUPS})
        stats_new = None
        if carry_stats:                                       # prune_points gathers the accumulators (:1150-1152)
            stats_new = [tab.add(old) for old in (accum, denom, max_radii)]
        if P_new > 0 and P > 0:
            _lib.check(lib.c3dgs_rows_apply(P, P_new, src.data_ptr(), kind.data_ptr(), draw_row.data_ptr(), len(tab.jobs), tab.array(),
                                            N, N * S, rotation.data_ptr(), _ptr(std),
                                            draws.data_ptr() if draws.numel() else None,
                                            int(not self.use_factor_scaling), int(self.quantization), _stream(dev)))
        if new_xyz is not None:
            new_xyz(tab.new["_xyz"])
        self._install(tab.new, tab.moments)
        # carry_stats is prune_points: every new row is an original (the 3D filter follows); anything else creates rows
        if carry_stats:
            self._carry_3D_filter(src)
        else:
            self._drop_3D_filter()
        if stats_new is not None:
            self.xyz_gradient_accum, self.denom, self.max_radii2D = stats_new
        else:                                                 # densification_postfix, :1209-1211
            self.xyz_gradient_accum = torch.zeros((P_new, 1), device=dev)
            self.denom = torch.zeros((P_new, 1), device=dev)
            self.max_radii2D = torch.zeros((P_new,), device=dev)

    def _install(self, new, moments):
        """The new parameter tensors {attr: tensor} become the model's leaves; each one's param group is re-pointed and its
        optimizer state follows it (`step` kept, moments replaced where `moments` has them)."""
        for name, attr, _ in self._GROUPS:
            if attr not in new:
                continue
            old, param = getattr(self, attr), new[attr].requires_grad_(True)
            if self.optimizer is not None:
                for group in self.optimizer.param_groups:
                    if group.get("name") == name:
                        st = self.optimizer.state.pop(old, None)
                        group["params"][0] = param
                        if st is not None:
                            if attr in moments:
                                st["exp_avg"], st["exp_avg_sq"] = moments[attr]
                            self.optimizer.state[param] = st
            setattr(self, attr, param)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, draws=None, N=2, scores=None):
        """:1336-1349 fused: the reference's clone stage, split stage and final prune decided per row in one classification
        pass, the scene rebuilt in one pass. Every decision is taken on the values the staged sequence would have seen and the
        three observers (scaling, scaling_factor, opacity) are left as it leaves them (DESIGN.md "Density control").
        `draws`: [N*S,3] unit normals for the S split parents (default torch.randn). Returns the plan (src, kind, draw_row,
        (kept, clones, S, parents with surviving children)).
        `scores`: f32 [P], e.g. error_max of add_error_stats / error_stats. It takes the place of xyz_gradient_accum / denom in
        the classification (handed over as the accumulator with a denominator of ones: the kernel is the same), `max_grad` is
        then the score threshold; every other decision and the rebuild are unchanged, and the error accumulators are zeroed
        behind the rebuild."""
        self._dense_only("densify_and_prune")
        lib = _lib.lib()
        dev = self.device
        with torch.no_grad():
            P = self._xyz.shape[0]
            accum, denom, _ = self._density_stats()
            if scores is not None:
                if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.numel() != P:
                    raise RuntimeError(f"densify_and_prune: scores must be a float32 tensor of {P} elements")
                accum = _lib.gpu_tensor(scores.detach().reshape(P), "scores")
                denom = torch.ones(P, dtype=torch.float32, device=dev)
            raw_s = self._scaling.detach()
            raw_f = self._scaling_factor.detach() if self._scaling_factor is not None else None
            dense_extent, big_extent = self.percent_dense * extent, 0.1 * extent
            s1 = self._activated_scaling(raw_s, raw_f).contiguous()             # get_scaling of the clone stage, :1284
            s2 = self._activated_scaling(raw_s, raw_f).contiguous()             # get_scaling of the split stage, :1225; children's std
            opacity = self._get(opacity=self._opacity.detach())[2].contiguous()  # get_opacity on the post-split scene, :1344
            code = torch.empty(P, dtype=torch.uint8, device=dev)
            sp_self = sp_child = None

            def classify(min_op):
                _lib.check(lib.c3dgs_densify_classify(P, accum.data_ptr(), denom.data_ptr(), s1.data_ptr(), s2.data_ptr(),
                                                      _ptr(sp_self), _ptr(sp_child), opacity.data_ptr(), max_grad, dense_extent,
                                                      min_op, big_extent, code.data_ptr(), _stream(dev)))
            if max_screen_size and P > 0:
                # get_scaling on the post-split scene (:1347): its value set is every non-parent original, every clone (raw rows)
                # and the children (std / (0.8 N)); a [2P,3] batch holds exactly that set with duplicates, which leaves the
                # min / max the observers see unchanged
                classify(float("-inf"))                                           # nothing pruned: the raw clone and split bits
                split = (code & _lib.ROW_SPLIT).bool()[:, None]
                pure_parent = split & ((code & _lib.ROW_CLONE) == 0)[:, None]
                child_raw = s2 / torch.full((1,), 0.8 * N, device=dev)
                if not self.use_factor_scaling:
                    child_raw = torch.log(child_raw)
                batch = torch.empty(2 * P, 3, device=dev)
                torch.where(pure_parent, child_raw, raw_s, out=batch[:P])
                torch.where(split, child_raw, raw_s, out=batch[P:])
                factors = raw_f.expand(2, P, 1).reshape(2 * P, 1) if raw_f is not None else None
                s3 = self._activated_scaling(batch, factors).contiguous()
                sp_self, sp_child = s3[:P], s3[P:]
            if P > 0:
                classify(min_opacity)
            plan = self._rebuild(code, N, std=s2, draws=draws)
            if scores is not None:
                self.error_max = self.error_sum_acc = None        # zeros at the new length on the next add_error_stats
                self._error_accumulators()
            return plan

    def _append_clones(self, rows, new_xyz=None):
        """Every original, then a copy of each row of `rows` (int32, in the order given; moments zero), through the one apply
        launch; `new_xyz(xyz_out)` as in _apply_plan."""
        dev = self.device
        P, n = self._xyz.shape[0], int(rows.shape[0])
        src = torch.cat((torch.arange(P, dtype=torch.int32, device=dev), rows))
        kind = torch.zeros(P + n, dtype=torch.uint8, device=dev)
        kind[P:] = 1                                              # C3DGS_KIND_CLONE
        draw_row = torch.full((P + n,), -1, dtype=torch.int32, device=dev)
        self._apply_plan(src, kind, draw_row, P + n, new_xyz=new_xyz)
        return src, kind, draw_row

    # ---- MCMC density control (not in the reference: "3D Gaussian Splatting as Markov Chain Monte Carlo", gsplat's MCMCStrategy);
    # non-indexed models; csrc/mcmc.hip, DESIGN.md "MCMC density control"
    def _mcmc_table(self):
        """The in-place tensor table of c3dgs_mcmc_apply: every parameter with its moments (where the optimizer has them), the raw
        opacity and the tensor that carries the log scale flagged (the factor when the model has one, its activation being exp)."""
        scale_attr = "_scaling_factor" if self._scaling_factor is not None else "_scaling"
        return self._row_table(None, [attr for _, attr, _ in self._GROUPS],
                               {"_opacity": _lib.MCMC_ROLE_OPACITY, scale_attr: _lib.MCMC_ROLE_SCALE}).jobs

    def relocate_gs(self, dead_mask=None, min_opacity=0.005, draws=None):
        """Move every dead Gaussian onto a live one sampled by opacity; opacity and scale of the source and of its copies are
        corrected so that together they composite to what the single Gaussian did (the paper's eq. 9, N = min(copies + 1, 51),
        evaluated in double). In place: P and the parameter tensors stay, `step` stays. -> the number relocated.

        `dead_mask`: bool / uint8 [P]; None: sigmoid(_opacity) <= min_opacity, derived by the kernel on the raw parameter (the
        opacity observer is not touched). `draws`: float64 uniforms in [0, 1), at least one per dead row (default torch.rand in
        float64); the j-th dead row in ascending row order uses draws[j]. All dead, none dead or no live row with weight: nothing
        changes, returns 0. exp_avg / exp_avg_sq of every source AND every destination row become zero: gsplat zeroes only the
        sources, but a destination's moments describe a Gaussian that is no longer there. One device->host read."""
        self._dense_only("relocate_gs")
        from . import mcmc, optim
        with torch.no_grad():
            P = self._xyz.shape[0]
            if P == 0:
                return 0
            w = mcmc.weights(self._opacity, dead_mask, None if dead_mask is not None else min_opacity)
            rows, count = optim.visible_rows(w.dead)                # the stable device-side selection of sparse Adam
            n, T = self._read_host(torch.cat((count.reshape(1).to(torch.int64), w.T.reshape(1).to(torch.int64))))
            if n == 0 or n == P or T == 0:
                return 0
            if draws is None:
                draws = torch.rand(n, dtype=torch.float64, device=self.device)
            sources = mcmc.draw(w, draws, n)
            mcmc.apply(P, n, rows, 0, sources, w.counts, self._mcmc_table(), True, min_opacity, w.ws, self.device)
            self._drop_3D_filter()                                  # the relocated rows are new Gaussians
            return n

    def add_new_gs(self, cap_max, draws=None, min_opacity=0.005):
        """Grow the scene by 5 % up to `cap_max` rows: n_new = max(0, min(cap_max, int(1.05 P)) - P) sources sampled by opacity
        over all rows, appended as copies (_append_clones: moments of the originals kept, zero for the new rows), then every
        source and its copies take the relocation opacity and scale, and the moments of the sources and the new rows are
        zeroed, as in relocate_gs. `draws`: float64 [>= n_new] uniforms (default torch.rand). -> the number added. No
        device->host read. (A scene without any opacity above 2^-20 has nothing to sample from: the new rows are zero.)"""
        self._dense_only("add_new_gs")
        from . import mcmc
        with torch.no_grad():
            P = self._xyz.shape[0]
            n_new = max(0, min(int(cap_max), int(1.05 * P)) - P)
            if n_new == 0 or P == 0:
                return 0
            if draws is None:
                draws = torch.rand(n_new, dtype=torch.float64, device=self.device)
            w = mcmc.weights(self._opacity, None, None, counts_rows=P + n_new)
            sources = mcmc.draw(w, draws, n_new)
            self._append_clones(sources)
            mcmc.apply(P + n_new, n_new, None, P, sources, w.counts, self._mcmc_table(), False, min_opacity, w.ws, self.device)
            return n_new

    def add_position_noise(self, noise_lr, xyz_lr=None, draws=None):
        """The per-iteration perturbation of MCMC training, in place on _xyz, one launch:
            xyz += Sigma xi g(o) noise_lr xyz_lr,   Sigma = R diag(s^2) R^T,   g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995)))
        from the RAW parameters through the model's activations (normalised quaternion; exp, or normalize(relu(.)) * exp(factor);
        sigmoid). FakeQuantize is NOT applied and the observers are not touched: the noise is a property of the optimisation,
        not of the quantised render. `xyz_lr`: None takes the current learning rate of the "xyz" group. `draws`: [P,3] unit
        normals (default torch.randn)."""
        self._dense_only("add_position_noise")
        from . import mcmc
        with torch.no_grad():
            P = self._xyz.shape[0]
            if xyz_lr is None:
                if self.optimizer is None:
                    raise RuntimeError("add_position_noise: xyz_lr=None needs training_setup (the learning rate of the xyz group)")
                xyz_lr = next(g["lr"] for g in self.optimizer.param_groups if g.get("name") == "xyz")
            if draws is None:
                draws = torch.randn((P, 3), device=self.device)
            mcmc.noise(self._xyz.detach(), self._rotation.detach(), self._scaling.detach(),
                       None if self._scaling_factor is None else self._scaling_factor.detach(), self._opacity.detach(), draws,
                       noise_lr, xyz_lr)

    def densify_and_clone(self, grads=None, grad_threshold=None, scene_extent=None, selected_pts_mask=None, new_xyz=None):
        """:1279-1330. The gradient-mask form: row order every original, then the clones; returns (src, kind, draw_row,
        totals). The explicit form (`selected_pts_mask`: a bool mask or an index tensor; `new_xyz`: [n,3] positions that
        replace the copies' own): the selected rows are appended in the order given; returns (src, kind, draw_row)."""
        self._dense_only("densify_and_clone")
        if selected_pts_mask is not None:
            with torch.no_grad():
                P = self._xyz.shape[0]
                sel = torch.as_tensor(selected_pts_mask, device=self.device)
                if sel.dtype == torch.bool:
                    if tuple(sel.shape) != (P,):
                        raise ValueError(f"densify_and_clone: a bool mask must have shape ({P},), got {tuple(sel.shape)}")
                    rows = torch.nonzero(sel).squeeze(1)
                else:
                    rows = sel.reshape(-1).to(torch.int64)
                    rows = torch.where(rows < 0, rows + P, rows)          # torch indexing counts negatives from the end
                    if rows.numel() and not bool(((rows >= 0) & (rows < P)).all()):
                        raise IndexError(f"densify_and_clone: row index out of range for {P} rows")
                n = int(rows.shape[0])
                if P + n > 2**31 - 256:
                    raise ValueError(f"densify_and_clone: {P + n} rows do not fit the row plan")
                fill = None
                if new_xyz is not None:
                    pos = torch.as_tensor(new_xyz, dtype=torch.float32, device=self.device)
                    if tuple(pos.shape) != (n, 3):
                        raise ValueError(f"densify_and_clone: new_xyz must be [{n}, 3], got {tuple(pos.shape)}")

                    def fill(out):
                        out[P:] = pos
                return self._append_clones(rows.to(torch.int32), fill)
        if new_xyz is not None:
            raise ValueError("densify_and_clone: new_xyz goes with selected_pts_mask")
        with torch.no_grad():
            mask = torch.norm(grads, dim=-1) >= grad_threshold
            mask &= self.get_scaling.detach().amax(dim=1) <= self.percent_dense * scene_extent
            code = mask.to(torch.uint8) * _lib.ROW_CLONE + _lib.ROW_KEEP
            return self._rebuild(code.contiguous())

    def densify_initial(self, dist_thr_coeff=1.0, max_points=None):
        """:1352-1389 in one pass (csrc/ray_fill.hip; DESIGN.md "Initial densification"): the gaps between every point and its
        three nearest neighbours are filled with new points one `average_step` apart. Every other attribute of a new row is
        its source row's, its moments are zero, the accumulators restart at the new length. Returns (src int32[n], slot
        uint8[n], level int32[n], (n0, n1, n2)) for the n new rows, in the reference's row order: slot, then level, then
        source index. A call that adds no row leaves the model untouched. Two host reads (the step, the totals).
        ValueError, with the model unchanged: fewer than 4 points, a zero or non-finite step (a planar cloud), and a new
        row count that overflows int32 or exceeds `max_points` (checked before anything is allocated)."""
        self._dense_only("densify_initial")
        from .knn import knn3
        lib = _lib.lib()
        dev = self.device
        with torch.no_grad():
            x = _lib.gpu_tensor(self._xyz.detach(), "xyz")                      # the raw _xyz, not get_xyz (:1355-1364)
            P = int(x.shape[0])
            if P < 4:
                raise ValueError(f"densify_initial: three neighbours need at least 4 points, the model has {P}")
            # :1355-1358: the product in fp32 (on the host, where its order is the reference's on a CPU model), the rest in doubles
            volume = torch.prod((x.max(dim=0)[0] - x.min(dim=0)[0]).cpu()).item() / P
            average_step = dist_thr_coeff * volume ** (1.0 / 3)
            step = C.c_float(average_step).value                          # numpy divides float32 by it: used rounded to fp32
            if not (math.isfinite(step) and step > 0.0):
                raise ValueError(f"densify_initial: the average step is {average_step!r} (bounding-box volume {volume * P!r}): "
                                 "the cloud has no extent on some axis, or dist_thr_coeff is not a positive finite number")
            idx, d2 = knn3(x)
            s = _stream(dev)
            totals = torch.empty(4, dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.c3dgs_ray_fill_plan_workspace_bytes(P, 0)), dtype=torch.uint8, device=dev)
            _lib.check(lib.c3dgs_ray_fill_plan(P, d2.data_ptr(), step, 0, None, None, None, totals.data_ptr(), ws.data_ptr(),
                                               ws.numel(), s))
            n0, n1, n2, overflow = self._read_host(totals)
            n = n0 + n1 + n2
            if overflow:
                raise ValueError(f"densify_initial: more than {2**31 - 256 - P} new rows (at least {n} counted) for {P} points "
                                 f"at step {step!r}: an outlier far from the cloud? Raise dist_thr_coeff or remove it")
            if max_points is not None and P + n > max_points:
                raise ValueError(f"densify_initial: {P} points would become {P + n} rows, more than max_points = {max_points} "
                                 f"(step {step!r}); an outlier adds one row per step of its distance")
            src = torch.empty(n, dtype=torch.int32, device=dev)
            slot = torch.empty(n, dtype=torch.uint8, device=dev)
            level = torch.empty(n, dtype=torch.int32, device=dev)
            if n == 0:
                return src, slot, level, (0, 0, 0)
            ws = torch.empty(int(lib.c3dgs_ray_fill_plan_workspace_bytes(P, n)), dtype=torch.uint8, device=dev)
            _lib.check(lib.c3dgs_ray_fill_plan(P, d2.data_ptr(), step, n, src.data_ptr(), slot.data_ptr(), level.data_ptr(),
                                               totals.data_ptr(), ws.data_ptr(), ws.numel(), s))

            def fill(out):
                _lib.check(lib.c3dgs_ray_fill_xyz(P, x.data_ptr(), idx.data_ptr(), d2.data_ptr(), step, n, src.data_ptr(),
                                                  slot.data_ptr(), level.data_ptr(), out[P:].data_ptr(), s))
            self._append_clones(src, fill)
            return src, slot, level, (n0, n1, n2)

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, draws=None):
        """:1213-1277. Row order: the originals that are not selected, then child copy 0 .. N-1 of the selected ones."""
        self._dense_only("densify_and_split")
        with torch.no_grad():
            P = self._xyz.shape[0]
            scaling = self.get_scaling.detach().contiguous()
            padded = torch.zeros(P, device=self.device)
            padded[:grads.shape[0]] = grads.squeeze()
            mask = (padded >= grad_threshold) & (scaling.amax(dim=1) > self.percent_dense * scene_extent)
            code = torch.where(mask, _lib.ROW_SPLIT | _lib.ROW_CHILD_KEPT, _lib.ROW_KEEP).to(torch.uint8)
            return self._rebuild(code.contiguous(), N, std=scaling, draws=draws)

    def prune_points(self, mask):
        """:1101-1158 for a non-indexed model: rows with mask are removed; the accumulators are gathered like the parameters."""
        self._dense_only("prune_points")
        with torch.no_grad():
            code = (~mask.to(self.device).bool()).to(torch.uint8).contiguous()
            return self._rebuild(code, carry_stats=True)

    # ---- indexed models: prune, codebook compaction and the two conversions (:889-910, :1101-1158); csrc/index_plan.hip
    _COLOR_ATTRS = ("_features_dc", "_features_rest")
    _GEOMETRY_ATTRS = ("_scaling", "_rotation")

    def _gather_rows(self, attrs, n_in, src, extra=()):
        """out[j] = in[src[j]] for the parameter tensors named by `attrs`, each with its two Adam moments, and for the plain
        tensors of `extra`: ONE copy-only c3dgs_rows_apply launch (kind all original, so moments are copied).
        -> ({attr: new tensor}, {attr: (exp_avg, exp_avg_sq)}, [new extra tensors]); nothing is installed."""
        dev = self.device
        n_out = int(src.shape[0])
        tab = self._row_table(n_out, attrs, {})
        extra_new = [tab.add(old) for old in extra]
        if n_out > 0 and n_in > 0 and tab.jobs:
            kind = torch.zeros(n_out, dtype=torch.uint8, device=dev)            # C3DGS_KIND_ORIGINAL
            # draw_row is read for child rows only: any [n_out] int32 buffer serves
            _lib.check(_lib.lib().c3dgs_rows_apply(n_in, n_out, src.data_ptr(), kind.data_ptr(), src.data_ptr(), len(tab.jobs),
                                                   tab.array(), 1, 0, None, None, None, 0, 0, _stream(dev)))
        return tab.new, tab.moments, extra_new

    def plan_index_prune(self, keep, idx0, K0, idx1, K1):
        """c3dgs_index_plan in its two calls around the one host read. keep: uint8 [P] or None; idx: int64 [P] or None.
        -> (src int32 [P_new], new_idx0, new_idx1 (int64 [P_new] or None), cb_src0, cb_src1 (int32 [K_new] or None),
        (P_new, K0_new, K1_new, out_of_range))."""
        lib = _lib.lib()
        dev = self.device
        s = _stream(dev)
        P = int(idx0.shape[0] if idx0 is not None else idx1.shape[0] if idx1 is not None else keep.shape[0])
        K0, K1 = (int(K0) if idx0 is not None else 0), (int(K1) if idx1 is not None else 0)
        ws = torch.empty(max(int(lib.c3dgs_index_plan_workspace_bytes(P, K0, K1)), 256), dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        args = (P, _ptr(keep), _ptr(idx0), K0, _ptr(idx1), K1)
        _lib.check(lib.c3dgs_index_plan(*args, 0, 0, 0, None, None, None, None, None, totals.data_ptr(), ws.data_ptr(), s))
        tot = tuple(self._read_host(totals))
        P_new, K0n, K1n, bad = tot
        if bad:
            raise RuntimeError(f"{bad} codebook indices lie outside their codebook ({K0} colour rows, {K1} geometry rows)")
        src = torch.empty(P_new, dtype=torch.int32, device=dev)
        new0 = torch.empty(P_new, dtype=torch.int64, device=dev) if idx0 is not None else None
        new1 = torch.empty(P_new, dtype=torch.int64, device=dev) if idx1 is not None else None
        cb0 = torch.empty(K0n, dtype=torch.int32, device=dev) if idx0 is not None else None
        cb1 = torch.empty(K1n, dtype=torch.int32, device=dev) if idx1 is not None else None
        if P_new > 0:
            _lib.check(lib.c3dgs_index_plan(*args, P_new, K0n, K1n, src.data_ptr(), _ptr(new0), _ptr(new1), _ptr(cb0), _ptr(cb1),
                                            totals.data_ptr(), ws.data_ptr(), s))
        return src, new0, new1, cb0, cb1, tot

    def prune_points_indexed(self, mask):
        """:1101-1158 for a model with either or both index arrays: the Gaussians with `mask` go, every codebook row no
        survivor references is dropped from _features_dc / _features_rest and from _scaling / _rotation together with its Adam
        moments, and both index arrays are remapped. Surviving Gaussians keep their order, surviving codebook rows are the
        referenced old rows in ascending old id, the new index is the rank of the old one among them (the reference's result,
        without its Python loop over the ids). Optimizer handling as in _rebuild: groups re-pointed, moments gathered, `step`
        kept; xyz_gradient_accum, denom and max_radii2D are gathered like the per-Gaussian parameters. One device->host read
        (the four totals), at most three gather launches, no getter: no observer moves.

        All rows pruned: the reference crashes (`unique_ids[-1]` of an empty tensor); here the result is a model with empty
        parameters, empty codebooks and empty index arrays. An index outside its codebook raises before anything is changed.

        Returns (src, cb_src0, cb_src1, (P_new, K0_new, K1_new, out_of_range)): the source row of every surviving Gaussian and
        the old id of every surviving colour / geometry codebook row (None for a half that is not indexed)."""
        fi, gi = self._feature_indices, self._gaussian_indices
        if fi is None and gi is None:
            raise RuntimeError("prune_points_indexed: the model has no index array; use prune_points")
        dev = self.device
        with torch.no_grad():
            P = self._xyz.shape[0]
            keep = None
            if mask is not None:
                if mask.shape[0] != P:
                    raise RuntimeError(f"prune_points_indexed: mask of {mask.shape[0]} rows for {P} Gaussians")
                keep = (~mask.to(dev).bool()).contiguous().view(torch.uint8)
            for idx, what in ((fi, "_feature_indices"), (gi, "_gaussian_indices")):        # the reference asserts this, :1131-1132
                if idx is not None and tuple(idx.shape) != (P,):
                    raise RuntimeError(f"prune_points_indexed: {what} has shape {tuple(idx.shape)} for {P} Gaussians")
            K0 = self._features_dc.shape[0] if fi is not None else 0
            K1 = self._scaling.shape[0] if gi is not None else 0
            accum, denom, max_radii = self._density_stats()
            src, new0, new1, cb0, cb1, tot = self.plan_index_prune(keep, fi, K0, gi, K1)
            rows = ["_xyz", "_opacity", "_scaling_factor"]
            rows += [] if fi is not None else list(self._COLOR_ATTRS)
            rows += [] if gi is not None else list(self._GEOMETRY_ATTRS)
            new, moments, stats = self._gather_rows(rows, P, src, extra=(accum, denom, max_radii))
            for attrs, n_in, cb in ((self._COLOR_ATTRS, K0, cb0), (self._GEOMETRY_ATTRS, K1, cb1)):
                if cb is not None:
                    n, m, _ = self._gather_rows(attrs, n_in, cb)
                    new.update(n)
                    moments.update(m)
            self._install(new, moments)
            self._carry_3D_filter(src)
            self.xyz_gradient_accum, self.denom, self.max_radii2D = stats
            if fi is not None:
                self._feature_indices = new0
            if gi is not None:
                self._gaussian_indices = new1
        return src, cb0, cb1, tot

    def compact_codebooks(self):
        """prune_points_indexed with nothing masked: drops the codebook rows no Gaussian references (mask_splats and a pruning
        compress_gaussians leave them behind) and renumbers the indices. Nothing calls it implicitly."""
        return self.prune_points_indexed(None)

    def to_indexed(self):
        """:902-910: identity index arrays, no compression. Parameters and optimizer are untouched; a half that is already
        indexed keeps its array."""
        n = self._xyz.shape[0]
        if self._feature_indices is None:
            self._feature_indices = torch.arange(0, n, dtype=torch.int64, device=self.device)
        if self._gaussian_indices is None:
            self._gaussian_indices = torch.arange(0, n, dtype=torch.int64, device=self.device)
        self.color_index_mode = ColorMode.ALL_INDEXED

    def to_unindexed(self):
        """:889-899: the four codebook tensors become per-Gaussian tensors, codebook[indices], and the index arrays go; a
        half-indexed model expands the half it has. Unlike the reference, which leaves the optimizer pointing at the dead
        codebook tensors, the param groups are re-pointed and every expanded row takes a copy of its codebook row's Adam
        moments (`step` kept). An index outside its codebook gives a zero row, it is never dereferenced."""
        with torch.no_grad():
            for attrs, name in ((self._COLOR_ATTRS, "_feature_indices"), (self._GEOMETRY_ATTRS, "_gaussian_indices")):
                idx = getattr(self, name)
                if idx is None:
                    continue
                K = getattr(self, attrs[0]).shape[0]
                # decided on the int64 value: narrowing first would fold 2^32 + 3 onto row 3
                src = torch.where((idx >= 0) & (idx < K), idx, -1).to(torch.int32)
                new, moments, _ = self._gather_rows(attrs, K, src)
                self._install(new, moments)
                setattr(self, name, None)
        self.color_index_mode = ColorMode.NOT_INDEXED

    def reset_opacity(self):
        """:1391-1397 with replace_tensor_to_optimizer (:1061-1079): opacity <- inverse_sigmoid(min(get_opacity, 0.01)), its
        moments zeroed, `step` kept."""
        with torch.no_grad():
            # the reference writes torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01): two accesses, so the
            # opacity observer moves twice; the value is the first one's
            m = torch.min(self.get_opacity.detach(), torch.ones_like(self.get_opacity) * 0.01)
            new = torch.log(m / (1 - m)).contiguous().requires_grad_(True)
        old = self._opacity
        if self.optimizer is not None:
            for group in self.optimizer.param_groups:
                if group.get("name") == "opacity":
                    st = self.optimizer.state.pop(old, None)
                    group["params"][0] = new
                    if st is not None:
                        if "exp_avg" in st:
                            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(new), torch.zeros_like(new)
                        self.optimizer.state[new] = st
        self._opacity = new

    # ---- render (gaussian_model.py:766-886)
    def render(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, override_color=None, clamp_color=True,
               cov3d=None, gather_visible=True, return_depth=False, return_contrib=False, error_target=None,
               pose_grad="reference", depth_grad=False, antialiasing=None, distortion=False, normal=False):
        """pose_grad: what a camera pose that requires grad receives. "reference" (the default): the reference's formula on the
        indexed rasterizer (rasterizer.camera_pose_jacobian_sum), nothing on the other. "exact": the gradient of the render itself
        on both (rasterizer._C.pose_grad, one pass behind the backward). A pose that does not require grad costs nothing either way.
        return_depth=True: the dict also carries "depth" (sum of alpha T z, not normalised), "alpha" (accumulated opacity)
        and "median_depth", each [H, W] (rasterizer._C.render_depth); forward-only, no gradient flows through them.
        return_contrib=True: the dict also carries "contrib_sum", "contrib_max" (sum / max of alpha T over the (pixel, entry)
        pairs the forward blended) and "contrib_hits" (their number), indexed like "radii" (rasterizer._C.render_contrib), and
        "contrib_rank" (see _extra_keys); forward-only as well.
        error_target=[3, H, W] fp32 device tensor (the view's ground truth): the dict also carries "error_sum", per Gaussian the
        sum of alpha T x mean |render - target| over the pairs the forward blended (rasterizer._C.render_error), indexed like
        "radii", and "error_rank" (the same convention as "contrib_rank"); forward-only as well.
        depth_grad=True: the keys of return_depth, but "depth" and "alpha" carry gradient to the model's parameters, on the fused
        indexed and the composed path alike (GaussianRasterizationSettings(depth_grad=True), csrc/render_maps_backward.hip);
        "median_depth" stays non-differentiable. The pose receives no gradient on this path, whatever `pose_grad` says: a camera
        pose that requires grad raises ValueError (not covered yet).
        distortion=True | (near, far): the keys and gradients of depth_grad plus "distortion", [H, W]: per pixel
        sum_i sum_j w_i w_j |s_i - s_j| over the blended entries (w = alpha T; s = the view-space depth z, or with a pair
        far / (far - near) (1 - near / z), 2DGS's mapping), Mip-NeRF 360's distortion regulariser, with gradient to the model's
        parameters on the fused indexed and the composed path alike (GaussianRasterizationSettings(distortion=),
        csrc/render_distortion.hip, csrc/render_maps_backward.hip). It composes with `antialiasing` and the 3D filter as
        depth_grad does, and like it refuses a camera pose that requires grad (ValueError).
        normal=True: the keys and gradients of depth_grad plus "normal", [3, H, W]: per pixel sum_k w_k n_k over the blended
        entries, n the Gaussian's shortest axis in VIEW space (x right, y down, z forward), unit length and facing the camera; not
        normalised, no background term (GaussianRasterizationSettings(normal=True), csrc/normals.hip, csrc/render_normal.hip,
        csrc/render_maps_backward.hip), with gradient to the model's parameters -- the rotations included -- on the fused indexed
        and the composed path alike. normals.normal_consistency(out["depth"], out["alpha"], out["normal"], camera.intrinsic) is
        2DGS's term on it. It composes with `antialiasing` and `distortion` (one blend replay in the backward for all maps) and
        refuses a camera pose that requires grad (ValueError). A covariance has no axes: `cov3d=` and pipe.compute_cov3D_python
        raise ValueError. With a 3D filter the rasterizer blends the filtered covariance as ever and the normals are made from the
        model's own scales and rotations: the filter adds the same amount to every squared scale, so the shortest axis is the same.
        antialiasing: None (the default) reads `pipe.antialiasing`; True multiplies every opacity by the compensation factor of the
        rasterizer's 0.3 px^2 low-pass (GaussianRasterizationSettings(antialiasing=True), csrc/aa_opacity.hip), on the fused indexed
        and the composed path alike, with gradients to the model's parameters. As with depth_grad, the pose receives no gradient
        and a camera pose that requires grad raises ValueError.
        With a 3D filter (compute_3D_filter) both paths draw every Gaussian with Sigma + (scaling_modifier f)^2 I and the opacity
        o sqrt(prod_k s_k^2 / (s_k^2 + f^2)) (filter3d.apply in front of the rasterizer, which takes them as cov3D_precomp and
        opacities), with gradients to the model's parameters; every option above sees those. A caller's `cov3d=` becomes
        cov3d + (scaling_modifier f)^2 I and keeps its gradient, the opacity factor then takes the model's scales as constants.
        pipe.compute_cov3D_python then raises NotImplementedError, a pose that requires grad ValueError, and a filter that rows
        were added behind RuntimeError until compute_3D_filter has run again."""
        if antialiasing is None:
            antialiasing = getattr(pipe, "antialiasing", False)
        if depth_grad and viewpoint_camera.extrinsic_vector.requires_grad:
            raise ValueError("render(depth_grad=True): the gradient to a camera pose that requires grad is not covered yet")
        if distortion is None:
            distortion = False
        if distortion is not False and viewpoint_camera.extrinsic_vector.requires_grad:
            raise ValueError("render(distortion=...): the gradient to a camera pose that requires grad is not covered yet")
        if antialiasing and viewpoint_camera.extrinsic_vector.requires_grad:
            raise ValueError("render(antialiasing=True): the gradient to a camera pose that requires grad is not covered")
        if normal and viewpoint_camera.extrinsic_vector.requires_grad:
            raise ValueError("render(normal=True): the gradient to a camera pose that requires grad is not covered yet")
        if normal and (cov3d is not None or pipe.compute_cov3D_python):
            raise ValueError("render(normal=True): a precomputed covariance has no axes, so no normal")
        if pipe.convert_SHs_python and override_color is None:
            raise NotImplementedError("convert_SHs_python: SH evaluation in Python is outside the mirrored render path")
        if pose_grad not in ("reference", "exact"):
            raise ValueError(f'pose_grad must be "reference" or "exact", not {pose_grad!r}')
        filter_3D = self._checked_3D_filter(pipe, cov3d, viewpoint_camera)
        dev = self.device
        settings = GaussianRasterizationSettings(
            intrinsic=viewpoint_camera.intrinsic.to(dev), extrinsic_vector=viewpoint_camera.extrinsic_vector.to(dev),
            bg=bg_color.to(dev), scale_modifier=scaling_modifier, sh_degree=self.active_sh_degree, prefiltered=False,
            debug=pipe.debug, clamp_color=clamp_color, depth=bool(return_depth), contrib=bool(return_contrib),
            error_target=error_target, depth_grad=bool(depth_grad) or distortion is not False or bool(normal),
            antialiasing=bool(antialiasing), distortion=distortion, normal=bool(normal))
        indexed = self.color_index_mode == ColorMode.ALL_INDEXED and self.is_gaussian_indexed
        fused = indexed and self.use_factor_scaling and cov3d is None and override_color is None and \
            not pipe.compute_cov3D_python
        screenspace_points = torch.zeros(self._xyz.shape, dtype=torch.float32, device=dev, requires_grad=True)
        if fused:
            return self._render_indexed_fused(settings, screenspace_points, pose_grad, filter_3D)
        return self._render_composed(settings, screenspace_points, indexed, pipe, scaling_modifier, override_color, cov3d,
                                     gather_visible, pose_grad, filter_3D)

    def _visible(self, settings):
        """visible flags, their exclusive scan and a deferred host read of the count."""
        lib = _lib.lib()
        dev = self.device
        P = self._xyz.shape[0]
        view = _rz.camera_matrices(settings.intrinsic, settings.extrinsic_vector, dev)[0]
        visible = torch.empty(P, dtype=torch.uint8, device=dev)
        rank = torch.empty(P, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        scan = torch.empty(max(int(lib.c3dgs_qat_scan_bytes(P)), 256), dtype=torch.uint8, device=dev)
        q = _qat_params(self, self._fq_state, xyz=self._xyz)
        _lib.check(lib.c3dgs_qat_visible(C.byref(q), view.data_ptr(), visible.data_ptr(), rank.data_ptr(), count.data_ptr(),
                                         scan.data_ptr(), _stream(dev)))
        if self._count_host is None:
            self._count_host = torch.empty(1, dtype=torch.int32).pin_memory()
        self._count_host.copy_(count, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))

        def read():
            spins = 0
            while not ev.query():                 # poll: a blocking wait can cost milliseconds of wake-up on a busy host
                spins += 1
                if spins > 2_000_000:
                    ev.synchronize()
                    break
            return int(self._count_host[0])
        return visible, rank, read

    def _render_indexed_fused(self, settings, screenspace_points, pose_grad="reference", filter_3D=None):
        visible, rank, read = self._visible(settings)
        (means3D, means2D, opac, sfac, scales_n, rotations, shs, sh_idx, g_idx) = _QatGetters.apply(
            self, (visible, rank, read), self._feature_indices, self._gaussian_indices, self._xyz, screenspace_points,
            self._opacity, self._scaling_factor, self._scaling, self._rotation, self._features_dc, self._features_rest)
        if filter_3D is not None:
            # the getters hand out the visible subset; the kernel reads the filter's rows through the same visible / rank tables.
            # The rasterizer then runs on (cov3D_precomp, opacities) = (Sigma', o'), without a pose gradient (render() has refused one)
            from . import filter3d
            cov3D, opac = filter3d.apply(opac, scales_n, rotations, filter_3D, settings.scale_modifier, scale_factors=sfac,
                                         g_indices=g_idx, visible=visible, rank=rank)
            # with `normal`: the scales and rotations ride beside the covariance as the normals' axes (unfiltered: the filter moves
            # no axis and leaves the shortest one the shortest)
            axes = (scales_n, rotations) if settings.normal else (_rz._empty(), _rz._empty())
            image, radii, *extras = _rz.rasterize_gaussians_indexed(means3D, means2D, shs, sh_idx, g_idx, _rz._empty(), opac,
                                                                    axes[0], _rz._empty(), axes[1], cov3D, settings,
                                                                    settings.extrinsic_vector)
            return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
                    "visible": visible.bool(), **self._extra_keys(settings, extras, rank)}
        # what GaussianRasterizerIndexed(settings, optimize_camera=True)(...) calls, without building an nn.Module per view
        # (the host has ~0.2 ms of Python between the visible count's arrival and the rasterizer's first launch, and the GPU
        # idles for the part of it the getter kernels do not cover)
        rasterize = _rz.rasterize_gaussians_indexed_camera_exact if pose_grad == "exact" else _rz.rasterize_gaussians_indexed_camera
        if settings.depth_grad or settings.antialiasing:   # no pose gradient in these modes (render() has refused a pose that wants one)
            rasterize = _rz.rasterize_gaussians_indexed
        image, radii, *extras = rasterize(means3D, means2D, shs, sh_idx, g_idx, _rz._empty(), opac, scales_n, sfac, rotations,
                                          _rz._empty(), settings, settings.extrinsic_vector)
        return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
                "visible": visible.bool(), **self._extra_keys(settings, extras, rank)}

    @staticmethod
    def _extra_keys(settings, extras, rank):
        """the rasterizer's extra outputs -> the keys render() adds: the three maps under settings.depth, then under
        settings.contrib the three per-Gaussian rows and "contrib_rank" (int32 [P]: the row of a visible Gaussian in them, or
        None when they are indexed by Gaussian), then under settings.error_target "error_sum" and "error_rank" (the same rank),
        then under settings.distortion the "distortion" map, then under settings.normal the "normal" map, the rasterizer's last
        output"""
        scored = settings.error_target is not None
        names = (("depth", "alpha", "median_depth") if (settings.depth or settings.depth_grad) else ()) + \
            (("contrib_sum", "contrib_max", "contrib_hits") if settings.contrib else ()) + (("error_sum",) if scored else ()) + \
            (("distortion",) if settings.distortion is not False else ()) + (("normal",) if settings.normal else ())
        assert len(names) == len(extras)
        out = dict(zip(names, extras))
        if settings.contrib:
            out["contrib_rank"] = rank
        if scored:
            out["error_rank"] = rank
        return out

    # ---- error scores over a set of views, the signal of densify_and_prune(scores=) (csrc/render_error.hip; not in the reference)
    def _error_accumulators(self):
        """error_max / error_sum_acc of the current length: zeros when absent or of another length, like _density_stats"""
        n = self._xyz.shape[0]
        for name in ("error_max", "error_sum_acc"):
            t = getattr(self, name, None)
            if t is None or tuple(t.shape) != (n,) or t.device != self._xyz.device:
                setattr(self, name, torch.zeros((n,), dtype=torch.float32, device=self.device))
        return self.error_max, self.error_sum_acc

    def add_error_stats(self, error_sum, visible=None, rank=None):
        """One view's "error_sum" of render(error_target=) into the model-sized accumulators: error_max[i] = max(error_max[i], e),
        error_sum_acc[i] += e with e = error_sum[rank[i]] for the rows with visible[i] (render()'s "visible" and "error_rank"),
        or e = error_sum[i] when both are None. One c3dgs_error_accumulate launch that neither allocates nor synchronises (the
        accumulators are created as zeros on the first call at a length)."""
        acc_max, acc_sum = self._error_accumulators()
        P = self._xyz.shape[0]
        if (visible is None) != (rank is None):
            raise RuntimeError("add_error_stats: visible and rank come as a pair")
        if error_sum.dtype != torch.float32 or error_sum.dim() != 1 or not error_sum.is_contiguous():
            raise RuntimeError("add_error_stats: error_sum must be the rasterizer's contiguous float32 row")
        if visible is not None:
            if visible.shape[0] != P or rank.shape[0] != P or rank.dtype != torch.int32 or visible.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError("add_error_stats: visible bool [P] and rank int32 [P] of the model's length are needed")
        elif error_sum.shape[0] != P:
            raise RuntimeError(f"add_error_stats: {error_sum.shape[0]} rows for {P} Gaussians and no visible / rank")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().c3dgs_error_accumulate(P, int(error_sum.shape[0]), _ptr(visible), _ptr(rank), error_sum.data_ptr(),
                                                         acc_max.data_ptr(), acc_sum.data_ptr(), _stream(self.device)))

    def error_stats(self, cameras, pipe, bg_color):
        """-> dict(error_max f32 [P], error_sum f32 [P]) over `cameras`: per Gaussian the maximum and the sum over the views of
        its error score against `cam.original_image`. One render(error_target=) per camera under no_grad and one
        c3dgs_error_accumulate launch per view; no host read of its own. The model's own accumulators (add_error_stats) are not
        touched. As in contribution_stats the observer / quantiser state is saved in front of the pass and put back behind it."""
        dev = self.device
        P = self._xyz.shape[0]
        acc = dict(error_max=torch.zeros(P, dtype=torch.float32, device=dev), error_sum=torch.zeros(P, dtype=torch.float32, device=dev))
        lib = _lib.lib()
        with torch.no_grad():
            fq_saved = self._fq_state.clone()
            for cam in cameras:
                target = cam.original_image.to(dev)
                out = self.render(cam, pipe, bg_color, error_target=target)
                visible, rank, es = out["visible"], out["error_rank"], out["error_sum"]
                if rank is None:
                    visible = None
                with torch.cuda.device(dev):
                    _lib.check(lib.c3dgs_error_accumulate(P, int(es.shape[0]), _ptr(visible), _ptr(rank), _ptr(es),
                                                          acc["error_max"].data_ptr(), acc["error_sum"].data_ptr(), _stream(dev)))
            self._fq_state.copy_(fq_saved)
        return acc

    # ---- contribution statistics over a set of views, and pruning by them (csrc/render_contrib.hip; not in the reference)
    def contribution_stats(self, cameras, pipe, bg_color):
        """-> dict(weight_sum f32 [P], weight_max f32 [P], hits int64 [P], views int32 [P]) over `cameras`: per Gaussian the sum
        and the maximum of its blend weight alpha T, the number of (pixel, entry) pairs that blended it, and the number of views
        in which at least one did. One render(return_contrib=True) per camera under no_grad and one c3dgs_contrib_accumulate
        launch per view (through the view's visible flags and the ranks render() hands out with them); no host read of its own.
        The renders go through the getters, which on a quantisation-aware model move the observers; the observer / quantiser
        state is saved in front of the pass and put back behind it, so the statistics leave the model as they found it."""
        dev = self.device
        P = self._xyz.shape[0]
        acc = dict(weight_sum=torch.zeros(P, dtype=torch.float32, device=dev), weight_max=torch.zeros(P, dtype=torch.float32, device=dev),
                   hits=torch.zeros(P, dtype=torch.int64, device=dev), views=torch.zeros(P, dtype=torch.int32, device=dev))
        lib = _lib.lib()
        with torch.no_grad():
            fq_saved = self._fq_state.clone()
            for cam in cameras:
                out = self.render(cam, pipe, bg_color, return_contrib=True)
                visible, rank = out["visible"], out["contrib_rank"]       # bool [P] (one byte each), int32 [P]
                ws, wm, h = out["contrib_sum"], out["contrib_max"], out["contrib_hits"]
                with torch.cuda.device(dev):
                    _lib.check(lib.c3dgs_contrib_accumulate(P, int(ws.shape[0]), _ptr(visible), _ptr(rank), _ptr(ws), _ptr(wm), _ptr(h),
                                                            acc["weight_sum"].data_ptr(), acc["weight_max"].data_ptr(),
                                                            acc["hits"].data_ptr(), acc["views"].data_ptr(), _stream(dev)))
            self._fq_state.copy_(fq_saved)
        return acc

    def prune_by_contribution(self, stats, min_views=1, min_weight_max=0.0):
        """Removes the Gaussians that `stats` (contribution_stats) saw blended in fewer than `min_views` views or whose largest
        blend weight is below `min_weight_max`, with prune_points_indexed on an indexed model and prune_points otherwise, as
        finetune prunes. -> how many went (one host read)."""
        P = self._xyz.shape[0]
        if stats["views"].shape[0] != P:
            raise RuntimeError(f"prune_by_contribution: statistics of {stats['views'].shape[0]} rows for {P} Gaussians")
        with torch.no_grad():
            mask = (stats["views"] < int(min_views)) | (stats["weight_max"] < float(min_weight_max))
            n = int(mask.sum())
            if n:
                if self.is_color_indexed or self.is_gaussian_indexed:
                    self.prune_points_indexed(mask)
                else:
                    self.prune_points(mask)
        return n

    def _render_composed(self, settings, screenspace_points, indexed, pipe, scaling_modifier, override_color, cov3d,
                         gather_visible=True, pose_grad="reference", filter_3D=None):
        """Every other configuration of render(): the same getters, composed with torch gathers like the reference.
        gather_visible=False (the sensitivity pass) hands all rows to the rasterizer instead of the reference's `t[visible]`
        copies: the rasterizer culls the same Gaussians itself (mark_visible is its own frustum test), so image and gradients
        are the same, `radii` / `viewspace_points` are then indexed by Gaussian rather than by visible row."""
        means3D = self.get_xyz
        opacity = self.get_opacity
        exact = pose_grad == "exact"
        if settings.depth_grad or settings.antialiasing or filter_3D is not None:   # no pose gradient in these modes (render() has refused a pose that wants one)
            rasterizer = (GaussianRasterizerIndexed if indexed else GaussianRasterizer)(raster_settings=settings, optimize_camera=False)
        else:
            rasterizer = GaussianRasterizerIndexed(raster_settings=settings, optimize_camera="exact" if exact else True) if indexed \
                else GaussianRasterizer(raster_settings=settings, optimize_camera="exact" if exact else False)
        scales = rotations = None
        cov3D_precomp = cov3d
        if cov3D_precomp is None:
            if pipe.compute_cov3D_python:
                cov3D_precomp = self.get_covariance(scaling_modifier)
            else:
                scales = self.get_scaling_normalized if indexed else self.get_scaling
                rotations = self._rotation_post_activation if indexed else self.get_rotation
        scale_factors = self.get_scaling_factor if indexed else None
        if filter_3D is not None:
            # all P rows in one launch, in front of the gathers: the rasterizer takes (cov3D_precomp, opacities) = (Sigma', o')
            from . import filter3d
            if indexed and not torch.is_tensor(scale_factors):
                scale_factors = torch.ones_like(opacity)
            given = cov3D_precomp
            if given is not None:
                # a caller's covariance (train()'s frozen one, the sensitivity pass's leaf): Sigma' = cov3d + f^2 I with the
                # gradient to cov3d untouched; the opacity factor takes the model's own scales, as constants like the covariance
                scales = (self.get_scaling_normalized if indexed else self.get_scaling).detach()
                scale_factors = scale_factors.detach() if indexed else None
            cov3D_precomp, opacity = filter3d.apply(opacity, scales, rotations, filter_3D, scaling_modifier,
                                                    scale_factors=scale_factors if indexed else None,
                                                    g_indices=self._gaussian_indices if indexed else None, cov3d=given)
            if not (settings.normal and given is None):         # with `normal` the pair stays, as the normals' axes
                scales = rotations = None
            scale_factors = None
        shs = colors_precomp = None
        if override_color is None:
            shs = self._get_features_raw if indexed else self.get_features
        else:
            colors_precomp = override_color
        visible = rasterizer.markVisible(means3D, extrinsic_vector=settings.extrinsic_vector)
        # `t[visible]` of the reference (gaussian_model.py:851-862) for every input, from ONE nonzero: a boolean-mask index
        # runs nonzero (with its host sync) per tensor, and its backward is a sort-based index_put(accumulate) -- 2 ms
        # per tensor for 6M rows -- although the rows are unique.
        rank = None
        if gather_visible:
            rows = visible.nonzero(as_tuple=False).squeeze(1)
            if settings.contrib or settings.error_target is not None:   # model row -> row of the gathered tensors: the exclusive scan of the flags
                rank = torch.cumsum(visible, 0, dtype=torch.int32) - visible.to(torch.int32)
            pick = lambda t: None if t is None else (_MaskGather.apply(t, rows) if t.requires_grad else t.index_select(0, rows))  # noqa: E731
        else:
            pick = lambda t: t  # noqa: E731
        if indexed:
            image, radii, *extras = rasterizer(means3D=pick(means3D), means2D=pick(screenspace_points), shs=shs,
                                               sh_indices=pick(self._feature_indices), g_indices=pick(self._gaussian_indices),
                                               colors_precomp=None, opacities=pick(opacity), scales=scales,
                                               scale_factors=pick(scale_factors), rotations=rotations,
                                               cov3D_precomp=pick(cov3D_precomp), extrinsic_vector=settings.extrinsic_vector)
        else:
            image, radii, *extras = rasterizer(means3D=pick(means3D), means2D=pick(screenspace_points), shs=pick(shs),
                                               colors_precomp=pick(colors_precomp), opacities=pick(opacity), scales=pick(scales),
                                               rotations=pick(rotations), cov3D_precomp=pick(cov3D_precomp),
                                               extrinsic_vector=settings.extrinsic_vector)
        return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
                "visible": visible, **self._extra_keys(settings, extras, rank)}


class _MaskGather(torch.autograd.Function):
    """t[mask] with the row numbers of the mask given: forward index_select, backward a plain scatter into zeros (the rows
    are unique, nothing accumulates)."""

    @staticmethod
    def forward(ctx, t, rows):
        ctx.save_for_backward(rows)
        ctx.n = t.shape[0]
        return t.index_select(0, rows)

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        out = g.new_zeros((ctx.n,) + tuple(g.shape[1:]))
        out.index_copy_(0, rows, g.contiguous())
        return out, None


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:32-65: log-linear interpolation from lr_init (step 0) to lr_final (step max_steps), optionally
    eased in over lr_delay_steps; 0 for negative steps or when both rates are 0."""
    import math

    def rate(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return rate


def _covariance(scaling, scaling_modifier, rotation, strip_sym=True):
    """build_covariance_from_scaling_rotation (gaussian_model.py:55-64): Sigma = R S S^T R^T, upper triangle."""
    r = rotation / rotation.norm(dim=1, keepdim=True)          # build_rotation normalises again (general_utils.py:84-89)
    w, x, y, z = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = R * (scaling_modifier * scaling)[:, None, :]
    # L @ L^T written out: a batched 3x3 GEMM of millions of matrices runs at a few GB/s in the BLAS library (52 ms for 6M)
    r0, r1, r2 = L[:, 0], L[:, 1], L[:, 2]
    sym = torch.stack([(r0 * r0).sum(1), (r0 * r1).sum(1), (r0 * r2).sum(1), (r1 * r1).sum(1), (r1 * r2).sum(1),
                       (r2 * r2).sum(1)], dim=1)
    if strip_sym:
        return sym
    return sym[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
