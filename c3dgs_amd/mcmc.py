"""Thin entries of the MCMC density-control kernels (csrc/mcmc.hip; include/c3dgs_hip.h "MCMC density control"), on plain
tensors. GaussianModel.relocate_gs / add_new_gs / add_position_noise are built from them; tests and tools call them directly.
No CPU path."""
import ctypes as C

import torch

from . import _lib

WEIGHT_ONE = 1 << 20          # the integer weight of opacity 1
MAX_N = 51                    # relocation: N = min(count + 1, MAX_N)


def workspace(P, device):
    need = C.c_size_t(0)
    _lib.check(_lib.lib().c3dgs_mcmc_workspace_bytes(P, C.byref(need)))
    return _lib.workspace("mcmc", device, need.value)


def _mask_u8(mask, P):
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (P,):
        raise ValueError(f"c3dgs_amd.mcmc: the dead mask must be a bool or uint8 tensor of shape [{P}]")
    if not mask.is_cuda:
        raise RuntimeError("c3dgs_amd.mcmc: the dead mask must be a GPU tensor (there is no CPU path)")
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _draws(draws, n):
    if not torch.is_tensor(draws) or draws.dtype != torch.float64 or draws.dim() != 1 or draws.shape[0] < n:
        raise ValueError(f"c3dgs_amd.mcmc: draws must be a float64 tensor of at least {n} uniforms in [0, 1)")
    return _lib.gpu_tensor(draws, "draws", torch.float64)


class Weights:
    """What the weights stage of one sample call left behind: q (int32 view of the uint32 weights), counts, T (int64 [1], on the
    device), dead (uint8, the mask that was used or derived; None when every row took part), and the workspace that holds the
    prefix, valid until the next call on that device."""

    def __init__(self, P, q, counts, T, dead, ws):
        self.P, self.q, self.counts, self.T, self.dead, self.ws = P, q, counts, T, dead, ws


def weights(raw_opacity, dead_mask=None, min_opacity=None, counts_rows=None):
    """The weights stage alone (c3dgs_mcmc_sample with n = 0) -> Weights. `dead_mask`: the excluded rows; None with `min_opacity`:
    derived as sigmoid(raw) <= min_opacity; None without: every row takes part. `counts_rows` > P allocates a longer, zeroed
    counts tensor (add_new_gs hands it to the apply of the grown scene)."""
    op = _lib.gpu_tensor(raw_opacity.detach(), "raw_opacity").reshape(-1)
    P, dev = op.shape[0], op.device
    derive = dead_mask is None and min_opacity is not None
    dead = torch.empty(P, dtype=torch.uint8, device=dev) if derive else (None if dead_mask is None else _mask_u8(dead_mask, P))
    q = torch.empty(P, dtype=torch.int32, device=dev)
    counts = torch.zeros(max(P, counts_rows or 0), dtype=torch.int32, device=dev)
    T = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = workspace(max(P, counts_rows or 0), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().c3dgs_mcmc_sample(P, op.data_ptr(), None if derive else _lib.ptr(dead), int(derive),
                                                float(min_opacity) if derive else 0.0, dead.data_ptr() if derive else None, 0, None,
                                                0, q.data_ptr(), None, counts.data_ptr(), T.data_ptr(), ws.data_ptr(),
                                                _lib.stream(dev)))
    return Weights(P, q, counts, T, dead, ws)


def draw(w, draws, n=None):
    """n draws (default: all of `draws`) from the weights `w` -> sources int32 [n]; w.counts is zeroed and refilled."""
    n = draws.shape[0] if n is None else int(n)
    draws = _draws(draws, n)
    sources = torch.empty(n, dtype=torch.int32, device=draws.device)
    with torch.cuda.device(draws.device):
        _lib.check(_lib.lib().c3dgs_mcmc_sample(w.P, None, None, 0, 0.0, None, n, draws.data_ptr(), 1, None, sources.data_ptr(),
                                                w.counts.data_ptr(), None, w.ws.data_ptr(), _lib.stream(draws.device)))
    return sources


def sample(raw_opacity, draws, dead_mask=None, min_opacity=None):
    """One full c3dgs_mcmc_sample call -> (q, sources, counts, T, dead): weights, scan and the draws in one entry."""
    op = _lib.gpu_tensor(raw_opacity.detach(), "raw_opacity").reshape(-1)
    P, dev = op.shape[0], op.device
    n = int(draws.shape[0])
    draws = _draws(draws, n)
    derive = dead_mask is None and min_opacity is not None
    dead = torch.empty(P, dtype=torch.uint8, device=dev) if derive else (None if dead_mask is None else _mask_u8(dead_mask, P))
    q = torch.empty(P, dtype=torch.int32, device=dev)
    counts = torch.zeros(P, dtype=torch.int32, device=dev)
    sources = torch.empty(n, dtype=torch.int32, device=dev)
    T = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = workspace(P, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().c3dgs_mcmc_sample(P, op.data_ptr(), None if derive else _lib.ptr(dead), int(derive),
                                                float(min_opacity) if derive else 0.0, dead.data_ptr() if derive else None, n,
                                                draws.data_ptr() if n else None, 0, q.data_ptr(), sources.data_ptr() if n else None,
                                                counts.data_ptr(), T.data_ptr(), ws.data_ptr(), _lib.stream(dev)))
    return q, sources, counts, T, dead


def apply(P, n, dst, dst_base, sources, counts, table, copy_rows, min_opacity, ws, device):
    """c3dgs_mcmc_apply over `table`, a list of _lib.RowsTensor (in place: in_* == out_*)."""
    arr = (_lib.RowsTensor * len(table))(*table)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().c3dgs_mcmc_apply(P, n, _lib.ptr(dst), dst_base, sources.data_ptr(), counts.data_ptr(), len(table), arr,
                                               int(copy_rows), float(min_opacity), ws.data_ptr(), _lib.stream(device)))


def noise(xyz, rotation, scaling, scaling_factor, raw_opacity, xi, noise_lr, xyz_lr):
    """c3dgs_mcmc_noise: xyz [P,3] in place. scaling_factor None: s = exp(scaling); else normalize(relu(scaling)) * exp(factor)."""
    P, dev = xyz.shape[0], xyz.device
    for name, t, shape in (("xyz", xyz, (P, 3)), ("rotation", rotation, (P, 4)), ("scaling", scaling, (P, 3)), ("xi", xi, (P, 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f"c3dgs_amd.mcmc.noise: {name} must be [{shape[0]}, {shape[1]}], not {tuple(t.shape)}")
    if raw_opacity.numel() != P or (scaling_factor is not None and scaling_factor.numel() != P):
        raise ValueError("c3dgs_amd.mcmc.noise: opacity and scaling_factor have one value per row")
    if not xyz.is_cuda or xyz.dtype != torch.float32 or not xyz.is_contiguous():
        raise RuntimeError("c3dgs_amd.mcmc.noise: xyz must be a contiguous float32 GPU tensor (it is updated in place)")
    rot, sc, op, xi = (_lib.gpu_tensor(t, n) for t, n in ((rotation, "rotation"), (scaling, "scaling"), (raw_opacity, "opacity"), (xi, "xi")))
    fac = None if scaling_factor is None else _lib.gpu_tensor(scaling_factor, "scaling_factor")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().c3dgs_mcmc_noise(P, xyz.data_ptr(), rot.data_ptr(), sc.data_ptr(), _lib.ptr(fac), op.data_ptr(),
                                               xi.data_ptr(), float(noise_lr), float(xyz_lr), _lib.stream(dev)))
