"""Float64 reference of one step of Laplacian-normalised descent (``engine.LapDescentState``):

    g^ = lap_normalize(g, scale_n=lap_n)     the oracle's restatement of util.py:95-110 with torch convolutions, over all
                                             channels of the variable at once; lap_n = 0: g / max(mean|g|, 1e-7)
    x' = x - lr * g^

Arrays are [D,H,W,C] (3-D) or [H,W,C] (2-D); everything is NumPy / torch float64 on the host."""
import numpy as np
import torch

from oracle import nfs_oracle as O


def kernel(is_3d):
    from neural_flow_style_amd import util
    return util.lap_kernel(is_3d).astype(np.float64)


def normalized(g, lap_n, is_3d):
    g = np.asarray(g, np.float64)
    assert g.ndim == (4 if is_3d else 3), g.shape
    return O.lap_normalize(torch.tensor(g, dtype=torch.float64), kernel(is_3d), int(lap_n)).numpy()


def step(x, g, lr, lap_n, is_3d):
    """-> (x', the update x' - x) in float64"""
    upd = -float(lr) * normalized(g, lap_n, is_3d)
    return np.asarray(x, np.float64) + upd, upd


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def one_rounding(got32, x32, lr, g32):
    """is every element of ``got32`` the float64 value x - lr * g (from the float32 inputs, lr as the float32 the kernel
    takes) rounded once?  |diff| <= 2^-24 |result|, element by element; returns the worst ratio diff / (2^-24 |result|)"""
    want = np.asarray(x32, np.float64) - float(np.float32(lr)) * np.asarray(g32, np.float64)
    diff = np.abs(np.asarray(got32, np.float64) - want)
    bound = 2.0 ** -24 * np.abs(want)
    worst = float(np.max(np.where(diff > 0, diff / np.maximum(bound, 1e-300), 0.0)))
    return bool(np.all(diff <= bound)), worst
