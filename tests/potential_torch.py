"""Torch restatement of the reference's gradient lines (transform.py:508-515), channels reversed, and of the stream part
from the same differences: what tests/potential_ref.py is held to on the CPU and what autograd differentiates in the
oracle chain of the GPU tests."""
import torch


def torch_grad_reversed(p):
    """the gradient lines of transform.py:508-515 for p [D,H,W] (a torch tensor), channels reversed: per axis the
    difference of the two shifted slices with its last slice appended once more, stacked as (axis D, axis H, axis W).
    Those lines have no value on an axis of length 1 (nothing to append); the kernels define the difference as zero there,
    which is what the same lines give on the field replicated to two slices along that axis, first slice taken."""
    out = []
    for ax in range(3):
        x = torch.cat([p, p], dim=ax) if p.shape[ax] == 1 else p
        n = x.shape[ax]
        dif = x.narrow(ax, 1, n - 1) - x.narrow(ax, 0, n - 1)
        dif = torch.cat([dif, dif.narrow(ax, n - 2, 1)], dim=ax)
        out.append(dif.narrow(ax, 0, p.shape[ax]))
    return torch.stack(out, dim=-1)


def torch_stream_part(s):
    """the channel-reversed curl of s [D,H,W,3] from the same differences (component c of s along axis ax)"""
    d = lambda c, ax: torch_grad_reversed(s[..., c])[..., ax]
    return torch.stack([d(1, 2) - d(0, 1), d(0, 0) - d(2, 2), d(2, 1) - d(1, 0)], dim=-1)
