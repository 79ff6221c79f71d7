"""Fused Adam for the QAT inner loop (finetune.py:65-66; the optimizer the reference builds at
scene/gaussian_model.py:296-308: torch.optim.Adam(param_groups, lr=0.0, eps=1e-15)).

`Adam` is a torch.optim.Optimizer with torch.optim.Adam's constructor arguments and state keys ("step", "exp_avg",
"exp_avg_sq": state dicts are interchangeable), whose step() updates every parameter of every group with ONE kernel
launch per 16 tensors (csrc/adam.hip) instead of torch's dozen multi-tensor passes. weight_decay, amsgrad and maximize
are not used by the reference and are rejected. No CPU path.

`SparseGaussianAdam` (not in the reference; upstream 3DGS's optimizer_type="sparse_adam") is the same optimizer with
step(visibility): the parameter groups that carry "per_gaussian": True update only the rows (Gaussians) the mask lists and
leave every other row's parameter and moments untouched (csrc/sparse_adam.hip); all other groups take the dense step.
`visible_rows(mask)` is the list the step walks, for tests and tools."""
import ctypes as C
import math

import torch

from . import _lib

_MASK_KINDS = {torch.bool: 0, torch.uint8: 0, torch.int32: 1}      # c3dgs_sparse_adam_select's mask_kind


def _check_mask(mask):
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise RuntimeError("c3dgs_amd.optim: the visibility mask must be a GPU tensor (there is no CPU path)")
    if mask.dtype not in _MASK_KINDS:
        raise ValueError(f"c3dgs_amd.optim: the visibility mask must be bool, uint8 or int32, not {mask.dtype}")
    if mask.dim() != 1 or not mask.is_contiguous():
        raise ValueError("c3dgs_amd.optim: the visibility mask must be a contiguous tensor of shape [P]")


def _select(mask):
    """The list of the rows `mask` names, into the cached workspace of its device (no host read) -> the workspace."""
    L = _lib.lib()
    P, dev = mask.shape[0], mask.device
    need = C.c_size_t(0)
    _lib.check(L.c3dgs_sparse_adam_workspace_bytes(P, C.byref(need)))
    ws = _lib.workspace("optim", dev, need.value, zeroed=True)
    if P == 0:
        ws[:4].zero_()                                 # the library does nothing for P == 0: the count is this side's to clear
        return ws
    with torch.cuda.device(dev):
        _lib.check(L.c3dgs_sparse_adam_select(P, mask.data_ptr(), _MASK_KINDS[mask.dtype], ws.data_ptr(), _lib.stream(dev)))
    return ws


def visible_rows(mask):
    """-> (rows int32 [P], count int32 [1]): views of the cached workspace, valid until the next select on that device.
    rows[:count] are the ascending ids of the rows `mask` lists (bool / uint8: non-zero, int32: > 0)."""
    _check_mask(mask)
    ws = _select(mask)
    return ws[256:256 + 4 * mask.shape[0]].view(torch.int32), ws[:4].view(torch.int32)


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if weight_decay != 0 or amsgrad or maximize:
            raise RuntimeError("c3dgs_amd.optim.Adam mirrors the reference's plain Adam (no weight_decay / amsgrad / maximize)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._step(None)
        return loss

    def _step(self, visibility):
        """visibility=None: every tensor takes the dense launch. A mask: the tensors of the groups flagged "per_gaussian" go to
        the sparse launch over its rows instead (SparseGaussianAdam)."""
        L = _lib.lib()
        # one batch per kernel, [tensors, gradients kept alive, (betas, eps, device) shared by the tensors of one launch]
        dense, sparse = [[], [], None], [[], [], None]
        ws = None

        def flush(b):
            batch, keep, key = b
            if not batch:
                return
            (beta1, beta2), eps, dev = key
            with torch.cuda.device(dev):
                if b is dense:
                    arr = (_lib.AdamTensor * len(batch))(*batch)
                    _lib.check(L.c3dgs_adam_step(len(batch), arr, beta1, beta2, eps, _lib.stream(dev)))
                else:
                    arr = (_lib.SparseAdamTensor * len(batch))(*batch)
                    _lib.check(L.c3dgs_sparse_adam_step(len(batch), arr, visibility.shape[0], ws.data_ptr(), beta1, beta2, eps,
                                                        _lib.stream(dev)))
            batch.clear()
            keep.clear()

        if visibility is not None:                   # refuse a stale mask before any state moves
            for group in self.param_groups:
                for p in group["params"] if group.get("per_gaussian") else ():
                    if p.grad is not None and (p.dim() == 0 or p.shape[0] != visibility.shape[0]):
                        raise ValueError(f"SparseGaussianAdam.step: a per-Gaussian tensor has {p.shape[0] if p.dim() else 'no'} rows, the "
                                         f"visibility mask {visibility.shape[0]} (a mask from before densification or pruning?)")
                    if p.grad is not None and p.device != visibility.device:
                        raise RuntimeError("SparseGaussianAdam.step: the visibility mask is on another device than the parameters")

        for group in self.param_groups:              # the learning rate travels per tensor: groups share a launch
            beta1, beta2 = group["betas"]
            lr, eps = float(group["lr"]), float(group["eps"])
            b = sparse if visibility is not None and group.get("per_gaussian") else dense
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("c3dgs_amd.optim.Adam: parameters must be contiguous float32 GPU tensors (there is no CPU path)")
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                t = float(st["step"])
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                k = ((float(beta1), float(beta2)), eps, p.device)
                if b[2] is not None and k != b[2]:
                    flush(b)
                b[2] = k
                b[1].append(g)
                if b is sparse:
                    if ws is None:
                        ws = _select(visibility)
                    a = _lib.SparseAdamTensor()
                    a.row_len = p.numel() // p.shape[0] if p.shape[0] else 1
                else:
                    a = _lib.AdamTensor()
                a.param, a.grad, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                a.n = p.numel()
                a.step_size = lr / (1.0 - beta1 ** t)                      # double arithmetic, as torch's Python side
                a.bias_correction2_sqrt = math.sqrt(1.0 - beta2 ** t)
                b[0].append(a)
                if len(b[0]) == 16:
                    flush(b)
        flush(dense)
        flush(sparse)


class SparseGaussianAdam(Adam):
    """Adam whose step(visibility) updates only the listed rows of the groups that carry "per_gaussian": True. Same constructor
    rules and state keys as Adam. state["step"] advances on every call for every tensor with a gradient, listed or not, and
    the bias correction uses that global count (as upstream's sparse Adam does)."""

    @torch.no_grad()
    def step(self, visibility=None, closure=None):
        """visibility=None: Adam.step(). Otherwise a contiguous bool / uint8 (listed: non-zero) or int32 (listed: > 0, so `radii`
        goes in as it is) GPU tensor of shape [P]; every flagged tensor with a gradient must have P rows (ValueError otherwise:
        the mask predates a densification). No device-to-host read, no synchronisation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if visibility is not None:
            _check_mask(visibility)
        self._step(visibility)
        return loss
