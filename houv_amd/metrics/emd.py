"""Earth mover's distance operator: the interface of utils/metrics/EMD/emd_module.py:54-101 on top of the gfx950 kernels
(houv_emd_forward / houv_emd_backward).  The auction runs in one launch per call, with exact tie rules: the assignment is
deterministic (the reference's award step races).  Contract: include/houv_hip.h ``houv_emd_forward``, DESIGN.md section 9."""
import torch
from torch import nn
from torch.autograd import Function

from .. import ops


class emdFunction(Function):
    """(xyz1[B,N,3], xyz2[B,N,3], eps, iters) -> (dist[B,N] squared distances, assignment[B,N] int32).  The gradient flows
    to xyz1 only; xyz2's is a zero tensor, as the reference returns (emd_module.py:87-95)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters):
        dist, assignment, _ = ops.emd_forward(xyz1, xyz2, eps, iters)
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        xyz1, xyz2, assignment = ctx.saved_tensors
        gradxyz1 = ops.emd_backward(xyz1, xyz2, graddist, assignment).to(xyz1.dtype)
        return gradxyz1, torch.zeros_like(xyz2), None, None


class emdModule(nn.Module):
    """``metrics.emd()`` (emd_module.py:97-101): forward(input1, input2, eps, iters) -> (dist, assignment)."""

    def forward(self, input1, input2, eps, iters):
        return emdFunction.apply(input1, input2, eps, iters)
