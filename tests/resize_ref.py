"""NumPy restatement of the 3-D resize (include/nfs_hip.h: nfs_resize3d; reference util.py:128-167).

The TF-1 legacy resize kernels (``tf.compat.v1.image.resize``: no half-pixel centres) as the reference's
``resize_tf(is_3d=True)`` applies them -- over (H, W) of every depth slice, then over D -- written as fancy-indexed
lerps in the kernel's order, every operation rounded to ``dtype``.  ``np.float32`` is the contract the HIP kernel is
held to bit for bit; ``np.float64`` is the check on that contract."""
import numpy as np

METHODS = {"nearest": 0, "bilinear": 1}


def axis_table(n_in, n_out, method, align_corners, dtype=np.float32):
    """(lo, hi, t) per output index of one axis: s = n_in / n_out (or (n_in-1) / (n_out-1) with align_corners and
    n_out > 1), one division; p = i * s, one product"""
    dt = np.dtype(dtype).type
    if align_corners and n_out > 1:
        s = dt(n_in - 1) / dt(n_out - 1)
    else:
        s = dt(n_in) / dt(n_out)
    p = np.arange(n_out).astype(dtype) * dt(s)
    f = np.floor(p)
    if METHODS[method] == 0:
        if align_corners:                                   # roundf: halves away from zero (p - floor(p) is exact)
            f = f + (p - f >= dt(0.5)).astype(dtype)
        lo = np.minimum(f.astype(np.int64), n_in - 1)
        return lo, lo, np.zeros(n_out, dtype)
    lo = np.minimum(f.astype(np.int64), n_in - 1)
    hi = np.minimum(np.ceil(p).astype(np.int64), n_in - 1)
    return lo, hi, (p - f).astype(dtype)


def resize3d(x, size, method="bilinear", align_corners=False, scale=1.0, dtype=np.float32):
    """x [D,H,W] or [D,H,W,C] -> [oD,oH,oW(,C)], times ``scale``, in ``dtype`` arithmetic"""
    x = np.asarray(x)
    squeeze = x.ndim == 3
    v = (x[..., None] if squeeze else x).astype(dtype)
    D, H, W, _ = v.shape
    oD, oH, oW = (int(s) for s in size)
    dlo, dhi, td = axis_table(D, oD, method, align_corners, dtype)
    hlo, hhi, th = axis_table(H, oH, method, align_corners, dtype)
    wlo, whi, tw = axis_table(W, oW, method, align_corners, dtype)
    sc = np.dtype(dtype).type(scale)
    if METHODS[method] == 0:
        out = v[dlo][:, hlo][:, :, wlo] * sc
        return out[..., 0] if squeeze else out
    tw_, th_, td_ = tw[None, None, :, None], th[None, :, None, None], td[:, None, None, None]

    def lerp(a, b, t):
        d = b - a
        m = d * t
        return a + m

    top = lerp(v[:, hlo][:, :, wlo], v[:, hlo][:, :, whi], tw_)        # [D,oH,oW,C]: rows hlo
    bot = lerp(v[:, hhi][:, :, wlo], v[:, hhi][:, :, whi], tw_)
    r = lerp(top, bot, th_)
    out = lerp(r[dlo], r[dhi], td_) * sc
    assert out.dtype == np.dtype(dtype)
    return out[..., 0] if squeeze else out


def resize_tf(x, size, method="nearest", is_3d=False, dtype=np.float32):
    """x [B,D,H,W,C] -> size (d, h, w) with is_3d, else x [B,H,W,C] -> size (h, w) (a volume of depth 1)"""
    x = np.asarray(x)
    if is_3d:
        return np.stack([resize3d(b, size, method, False, 1.0, dtype) for b in x])
    return np.stack([resize3d(b[None], [1] + [int(s) for s in size], method, False, 1.0, dtype)[0] for b in x])


def rescale_size(n, scale):
    """the reference's casts (util.py:151-157): int32(float32(n) * scale)"""
    return [int(np.float32(k) * np.float32(scale)) for k in n]


def rescale_tf(x, scale, method="bilinear", is_3d=False, dtype=np.float32):
    x = np.asarray(x)
    return resize_tf(x, rescale_size(x.shape[1:4] if is_3d else x.shape[1:3], scale), method, is_3d, dtype)


def potential_factor(n_in, n_out):
    """the factor a resampled potential takes (styler_grid: mean over the axes of (n_out-1)/(n_in-1), formed in float64,
    cast to float32 once)"""
    return np.float32(np.mean([(float(o) - 1.0) / (float(i) - 1.0) for i, o in zip(n_in, n_out)], dtype=np.float64))
