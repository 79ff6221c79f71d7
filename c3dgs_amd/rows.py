"""The table of c3dgs_rows_tensor entries (include/c3dgs_hip.h) that c3dgs_rows_apply and c3dgs_mcmc_apply walk: the one
place that fills a _lib.RowsTensor. GaussianModel builds every density-control launch from it. No CPU path."""
import torch

from . import _lib


class RowTable:
    """Out of place (`n_out` rows per output): add() allocates the output, and both moment outputs where the optimizer state
    has moments. In place (`n_out` None): in_* == out_*, nothing is allocated. A tensor with zero floats per row gets its
    (empty) outputs and no job: the library refuses row_floats < 1, and there is nothing to move.

    jobs: the list of _lib.RowsTensor; new: {attr: output}; moments: {attr: (exp_avg, exp_avg_sq)}, both as _install takes
    them. The table keeps the contiguous inputs alive: hold it until the launch is issued."""

    def __init__(self, device, n_out=None):
        self.device, self.n_out = device, n_out
        self.jobs, self.new, self.moments, self._keep = [], {}, {}, []

    def add(self, old, role=_lib.ROLE_COPY, attr=None, state=None):
        """One tensor [rows, ...] with `role` (_lib.ROLE_*, _lib.MCMC_ROLE_*), under `attr` in new / moments if given, with the
        moments of its optimizer `state` (None, or a state without moments: a plain tensor). -> its output."""
        mom = (state["exp_avg"], state["exp_avg_sq"]) if state is not None and "exp_avg" in state else ()
        if self.n_out is None:
            for x in (old,) + mom:
                if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
                    raise RuntimeError(f"c3dgs_amd: {attr} and its moments must be contiguous float32 GPU tensors (the MCMC step is in place)")
            ins = outs = (old,) + mom
        else:
            ins = (_lib.gpu_tensor(old.detach(), attr or "tensor"),) + tuple(m.contiguous() for m in mom)
            outs = tuple(torch.empty((self.n_out,) + tuple(old.shape[1:]), dtype=torch.float32, device=self.device) for _ in ins)
        t = _lib.RowsTensor()
        t.row_floats, t.role = int(torch.Size(old.shape[1:]).numel()), role
        t.in_param, t.out_param = ins[0].data_ptr(), outs[0].data_ptr()
        if mom:
            t.in_exp_avg, t.in_exp_avg_sq, t.out_exp_avg, t.out_exp_avg_sq = (x.data_ptr() for x in ins[1:] + outs[1:])
        if t.row_floats > 0:
            self.jobs.append(t)
            self._keep.append(ins)
        if attr is not None:
            self.new[attr] = outs[0]
            if mom:
                self.moments[attr] = outs[1:]
        return outs[0]

    def array(self):
        return (_lib.RowsTensor * len(self.jobs))(*self.jobs)
