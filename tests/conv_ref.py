"""The VGG 3x3 convolution chain restated in float64 numpy (no torch, no tiles): the SAME stride-1 convolution, its data
gradient, the layer rules of include/nfs_hip.h around them, the two Winograd algorithms the kernels run (restated in
float64 to prove the matrices and in float32 to measure what float32 rounding alone does), the F(2x2) algorithm that
NFS_WINOGRAD_TILE=2 selects, restated the same two ways, and a worst-case float32 bound for every output element.  Layout NHWC, filters HWIO [3,3,Ci,Co].

Exact inputs.  With integer x, w, gy (|.| <= 3) and integer bias / addend every product and every partial sum of the
DIRECT kernels is an integer below 2^24 (``exact_units`` asserts it through loss_ref.units), so float32 holds each of
them in whatever order they are added and the output must EQUAL the float64 value.  The Winograd kernels are not exact
on integers (G holds 1/6, 1/24, ...), but with ZERO filters U = G 0 G^T = 0 exactly, every product is 0, and what remains
-- the bias, the ReLU, the pool, the mask and the addend -- is exact again.

Bounds (u = 2^-24, one float32 rounding; K input channels of the kernel's GEMM):

  direct kernels    1.01 (9 K + 20) u S + u |y|,  S = sum |x| |w|:  one rounding per fma step of the 9 K terms, up to 16
                    split-K partial sums, the bias or addend, 3 to spare; u |y| for the rounding of the stored value.

  Winograd          1.01 (K + c) u AW + u |y|,  c = 40.
                    AW = |A^T| ( sum_k |G||g||G^T| (.) |B^T||d||B| ) |A| per tile is the same algorithm with every matrix
                    and every operand replaced by its absolute value: the magnitude that a relative error made at any stage
                    is carried to the output with.  Stage by stage, to first order, a rounding made while forming a value
                    of that stage is at most u times the absolute chain up to there, and reaches the output through the
                    absolute matrices that follow, so each costs at most u AW:
                      filter passes (wg_g, twice)       <= 6 each: three constants that are no float32 (1/6, 1/24, 32/45 ...),
                                                        three products and two adds make at most 6 on the worst row     12
                      input passes (B^T, twice)         <= 7 each: the worst F(5x5) row has six terms, two products that
                                                        round (2.5, 5: the powers of two are exact) and five adds        14
                      the K sum                         K: one rounding per accumulated product; the split-limb GEMM carries
                                                        a product to 2^-26 < u instead of exactly, within the same count   K
                      output passes (A^T, twice)        <= 5 each: the worst F(5x5) row has two partial sums, no rounded
                                                        product (2, 4, 8, 16, 1/2 .. 1/16 are exact) and three adds      10
                      the add of the two K parts, the bias, the addend                                                    3
                    39, rounded up to c = 40; the factor 1.01 covers the second-order terms ((K + c) u < 4e-5).
                    F(4x4) needs less at every stage; one constant serves both families.

  F(2x2) Winograd   1.01 (K + c2) u AW2 + u |y|,  c2 = 12  (NFS_WINOGRAD_TILE=2: winograd_pack_kernel, winograd_input_kernel,
                    winograd_output_kernel).  The same argument with the F(2x2) matrices, which hold only 0, +-1 and 1/2:
                      filter passes (G, twice)          <= 2 each: the rows 1/2 (g0 +- g1 + g2) are two adds, the product by
                                                        1/2 is exact                                                      4
                      input passes (B^T, twice)         1 each: every row is one difference or one sum                   2
                      the K sum                         K, as above (the f32-input MFMA of the batched GEMM; there is no
                                                        split into K parts on this path)                                 K
                      output passes (A^T, twice)        2 each: three terms, two adds, no product                        4
                      the bias, the addend                                                                               2
                    12 = c2.  AW2 is built from |G2|, |B2^T|, |A2^T|; the rows of |B2^T| and |A2^T| sum to at most 2 and 3
                    where F(4x4)'s sum to 10 and 19, so on the same input the F(2x2) bound is several times tighter
                    (tests/test_conv_ref_cpu.py prints the ratio): the F(4x4) bound would let a wrong F(2x2) transform
                    row through and is not borrowed.

  pooled output     the mean of the four bounds + 3 u y_pool  (three adds; the factor 1/4 is exact)

The bound is loose against rounding (float32 Winograd sits at a thousandth of it) and tight against structure: a dropped
tap, pixel, mask bit or 16-channel slice exceeds it (tests/test_conv_ref_cpu.py plants them).  Rounding-level defects are
caught by comparing a kernel's error/bound with the float32 restatement's on the same input.
"""
import numpy as np

from tests.loss_ref import LIMIT, U, avgpool2, avgpool2_bwd, err_ratio, f64, units  # noqa: F401  (re-exported)

C_WINO = 40
C_WINO2 = 12
C_DIRECT = 20


# ---- the operation -------------------------------------------------------------------------------------------------------
def _pad1(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def conv(x, w, bias=None, relu=False):
    """(y [B,H,W,Co] = relu?(sum_{r,s,ci} x[h+r-1, w+s-1, ci] w[r,s,ci,co] + bias), S = sum |x| |w|): nine shifted
    matmuls; S has no bias in it"""
    x, w = f64(x), f64(w)
    B, H, W, _ = x.shape
    xp, ap, aw = _pad1(x), _pad1(np.abs(x)), np.abs(w)
    y = np.zeros((B, H, W, w.shape[3]))
    S = np.zeros_like(y)
    for r in range(3):
        for s in range(3):
            y += xp[:, r:r + H, s:s + W] @ w[r, s]
            S += ap[:, r:r + H, s:s + W] @ aw[r, s]
    if bias is not None:
        y = y + f64(bias)
    if relu:
        y = np.maximum(y, 0.0)
    return y, S


def dgrad_filters(w):
    """the data gradient's filters: taps flipped, channels transposed ([3,3,Co,Ci])"""
    return np.ascontiguousarray(f64(w)[::-1, ::-1].transpose(0, 1, 3, 2))


def dgrad(gy, w):
    """(gx [B,H,W,Ci] = sum_{r,s,co} gy[p-r+1, q-s+1, co] w[r,s,ci,co], the same sum over |terms|): the adjoint of conv
    wrt x written as the same sum with flipped taps and transposed channels"""
    return conv(gy, dgrad_filters(w))


# ---- the layer rules of nfs_hip.h ------------------------------------------------------------------------------------------
def layer_dgrad(g, x_in=None, addend=None, addend_unmasked=False, mask=None):
    """g = dgrad(gy) -> gx = g (x_in > 0) + addend, or (g + addend) (x_in > 0) with ``addend_unmasked``.  ``mask``
    replaces (x_in > 0) where given"""
    g = f64(g)
    m = mask if mask is not None else (None if x_in is None else f64(x_in) > 0)
    a = 0.0 if addend is None else f64(addend)
    if addend_unmasked:
        assert m is not None
        return (g + a) * m
    return (g if m is None else g * m) + a


def pooled_gy(gy_pool, out_mask):
    """g_y [B,H,W,Co] = 0.25 gy_pool[h/2, w/2] (x_out > 0), zero beyond the floored pooled area; out_mask = (x_out > 0).
    Every value is a float32 when gy_pool is (1/4 is a power of two)"""
    return avgpool2_bwd(gy_pool, out_mask.shape) * out_mask


# ---- Winograd --------------------------------------------------------------------------------------------------------------
# F(4x4, 3x3): points 0, +-1, +-2, inf (winograd_math.h, winograd_transform.h wg_g<6>)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
               [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
# F(5x5, 3x3): Cook-Toom points 0, +-1, +-2, 1/2, inf (winograd_transform.h w5_bt / w5_at / wg_g<7>)
G5 = np.array([[-1 / 2, 0, 0], [-1 / 3, -1 / 3, -1 / 3], [1 / 9, -1 / 9, 1 / 9], [1 / 36, 1 / 18, 1 / 9],
               [-1 / 60, 1 / 30, -1 / 15], [32 / 45, 16 / 45, 8 / 45], [0, 0, 1]])
BT5 = np.array([[-2, 4, 2.5, -5, -0.5, 1, 0], [0, 2, -2, -4.5, 0.5, 1, 0], [0, -2, 6, -3.5, -1.5, 1, 0],
                [0, 1, -1.5, -2, 1.5, 1, 0], [0, -1, 2.5, 0, -2.5, 1, 0], [0, 4, 0, -5, 0, 1, 0],
                [0, -2, 4, 2.5, -5, -0.5, 1]])
AT5 = np.array([[1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 0], [0, 1, -1, 8, -8, 1 / 8, 0],
                [0, 1, 1, 16, 16, 1 / 16, 1]])
# F(2x2, 3x3): points 0, +-1, inf (winograd.hip: winograd_pack_kernel, winograd_input_kernel, winograd_output_kernel)
G2 = np.array([[1, 0, 0], [1 / 2, 1 / 2, 1 / 2], [1 / 2, -1 / 2, 1 / 2], [0, 0, 1]])
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
MATS = {2: (G2, BT2, AT2), 4: (G4, BT4, AT4), 5: (G5, BT5, AT5)}


def patches(x, m):
    """x [B,H,W,K] -> the (m+2) x (m+2) patches of its m x m tiles [B,TH,TW,m+2,m+2,K], zero beyond the image"""
    B, H, W, K = x.shape
    TH, TW = -(-H // m), -(-W // m)
    xp = np.zeros((B, TH * m + 2, TW * m + 2, K), x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.empty((B, TH, TW, m + 2, m + 2, K), x.dtype)
    for i in range(m + 2):
        for j in range(m + 2):
            d[:, :, :, i, j] = xp[:, i:i + TH * m:m, j:j + TW * m:m]
    return d


def untile(Y, H, W):
    """[B,TH,TW,m,m,N] -> [B,H,W,N]"""
    B, TH, TW, m, _, N = Y.shape
    return Y.transpose(0, 1, 3, 2, 4, 5).reshape(B, TH * m, TW * m, N)[:, :H, :W]


def winograd64(x, w, m, absolute=False):
    """the convolution through F(m x m, 3x3) in float64 (m = 2 | 4 | 5): A^T ( sum_k (G g G^T) (.) (B^T d B) ) A per tile.
    ``absolute``: every matrix and operand by its absolute value -- AW of the bound"""
    x, w = f64(x), f64(w)
    G, BT, AT = MATS[m]
    if absolute:
        x, w, G, BT, AT = np.abs(x), np.abs(w), np.abs(G), np.abs(BT), np.abs(AT)
    H, W = x.shape[1:3]
    Uf = np.einsum("ir,rskn,js->ijkn", G, w, G)
    d = patches(x, m)
    B, TH, TW, S = d.shape[:4]
    V = np.einsum("ip,tpqk->tiqk", BT, d.reshape(B * TH * TW, S, S, -1), optimize=True)
    V = np.einsum("jq,tiqk->ijtk", BT, V, optimize=True)                       # [S,S,T,K]
    M = np.matmul(np.ascontiguousarray(V), np.ascontiguousarray(Uf))            # [S,S,T,N]: S^2 batched products (BLAS)
    Y = np.einsum("pi,ijtn->pjtn", AT, M, optimize=True)
    Y = np.einsum("qj,pjtn->tpqn", AT, Y, optimize=True)
    return untile(Y.reshape(B, TH, TW, m, m, -1), H, W)


def wino_bound(x, w, m, y):
    """the float32 bound of every element of y (the FINAL stored value: after bias, ReLU, mask, addend) computed through
    F(m x m) from x and w"""
    K = np.shape(x)[-1]
    return 1.01 * (K + (C_WINO2 if m == 2 else C_WINO)) * U * winograd64(x, w, m, absolute=True) + U * np.abs(f64(y))


def direct_bound(S, K, y):
    return 1.01 * (9 * K + C_DIRECT) * U * f64(S) + U * np.abs(f64(y))


def pool_bound(bound_y, y_pool):
    return avgpool2(bound_y) + 3.0 * U * np.abs(f64(y_pool))


# ---- the float32 restatement --------------------------------------------------------------------------------------------
_f = np.float32


def _g32(g0, g1, g2, m):
    """wg_g<6> / wg_g<7> / winograd_pack_kernel: the kernels' expressions, every operation rounded to float32"""
    if m == 2:
        return [g0, _f(0.5) * (g0 + g1 + g2), _f(0.5) * (g0 - g1 + g2), g2]
    if m == 4:
        return [_f(0.25) * g0, _f(-1 / 6) * (g0 + g1 + g2), _f(-1 / 6) * (g0 - g1 + g2),
                _f(1 / 24) * g0 + _f(1 / 12) * g1 + _f(1 / 6) * g2, _f(1 / 24) * g0 - _f(1 / 12) * g1 + _f(1 / 6) * g2, g2]
    return [_f(-0.5) * g0, _f(-1 / 3) * (g0 + g1 + g2), _f(1 / 9) * (g0 - g1 + g2),
            _f(1 / 36) * g0 + _f(1 / 18) * g1 + _f(1 / 9) * g2, _f(-1 / 60) * g0 + _f(1 / 30) * g1 - _f(1 / 15) * g2,
            _f(32 / 45) * g0 + _f(16 / 45) * g1 + _f(8 / 45) * g2, g2]


def _bt32(d, m):
    """wg4_bt / w5_bt / winograd_input_kernel"""
    if m == 2:
        return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    if m == 4:
        p, q = _f(-4) * d[2] + d[4], _f(-4) * d[1] + d[3]
        e, f = -d[2] + d[4], _f(-2) * d[1] + _f(2) * d[3]
        return [_f(4) * d[0] - _f(5) * d[2] + d[4], p + q, p - q, e + f, e - f, _f(4) * d[1] - _f(5) * d[3] + d[5]]
    return [_f(-2) * d[0] + _f(4) * d[1] + _f(2.5) * d[2] - _f(5) * d[3] - _f(0.5) * d[4] + d[5],
            _f(2) * d[1] - _f(2) * d[2] - _f(4.5) * d[3] + _f(0.5) * d[4] + d[5],
            _f(-2) * d[1] + _f(6) * d[2] - _f(3.5) * d[3] - _f(1.5) * d[4] + d[5],
            d[1] - _f(1.5) * d[2] - _f(2) * d[3] + _f(1.5) * d[4] + d[5],
            -d[1] + _f(2.5) * d[2] - _f(2.5) * d[4] + d[5],
            _f(4) * d[1] - _f(5) * d[3] + d[5],
            _f(-2) * d[1] + _f(4) * d[2] + _f(2.5) * d[3] - _f(5) * d[4] - _f(0.5) * d[5] + d[6]]


def _at32(v, m):
    """wg4_at / w5_at / winograd_output_kernel"""
    if m == 2:
        return [v[0] + v[1] + v[2], v[1] - v[2] - v[3]]
    s12, d12, s34, d34 = v[1] + v[2], v[1] - v[2], v[3] + v[4], v[3] - v[4]
    if m == 4:
        return [v[0] + s12 + s34, d12 + _f(2) * d34, s12 + _f(4) * s34, d12 + _f(8) * d34 + v[5]]
    return [v[0] + s12 + s34 + v[5], d12 + _f(2) * d34 + _f(0.5) * v[5], s12 + _f(4) * s34 + _f(0.25) * v[5],
            d12 + _f(8) * d34 + _f(0.125) * v[5], s12 + _f(16) * s34 + _f(0.0625) * v[5] + v[6]]


def winograd32(x, w, m, channels=None):
    """The same algorithm as the kernels' in float32 numpy: the passes as the kernels write them (columns, then rows),
    every product rounded (no fused multiply-add), K accumulated one term at a time in channel order.  Returns the
    pre-epilogue product [B,H,W,N'] as float32; ``channels``: only these output channels (a slice)."""
    x, w = np.asarray(x, _f), np.asarray(w, _f)
    if channels is not None:
        w = w[..., channels]
    H, W = x.shape[1:3]
    S = m + 2
    t = [_g32(w[0, s], w[1, s], w[2, s], m) for s in range(3)]                  # t[s][r]  [K,N]
    Uf = [_g32(t[0][r], t[1][r], t[2][r], m) for r in range(S)]                 # Uf[r][q]
    d = patches(x, m)                                                           # [B,TH,TW,S,S,K]
    c = [_bt32([d[:, :, :, i, j] for i in range(S)], m) for j in range(S)]      # c[j][r]
    V = [_bt32([c[j][r] for j in range(S)], m) for r in range(S)]               # V[r][q]  [B,TH,TW,K]
    K = x.shape[-1]
    Vs = np.stack([V[r][q] for r in range(S) for q in range(S)])                # [S S,B,TH,TW,K]
    Us = np.stack([Uf[r][q] for r in range(S) for q in range(S)])               # [S S,K,N]
    acc = np.zeros(Vs.shape[:4] + (w.shape[-1],), _f)
    for k in range(K):                                                          # (all components at once, k in order)
        acc += Vs[..., k, None] * Us[:, None, None, None, k, :]
    M = [[acc[r * S + q] for q in range(S)] for r in range(S)]
    cc = [_at32([M[r][q] for r in range(S)], m) for q in range(S)]              # cc[q][a]
    Y = [_at32([cc[q][a] for q in range(S)], m) for a in range(m)]              # Y[a][b]
    Y = np.stack([np.stack(Y[a], axis=3) for a in range(m)], axis=3)            # [B,TH,TW,m,m,N]
    return untile(Y, H, W)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def int_tensor(shape, seed, lim=3):
    """integers |.| <= lim as float32, a third of them exactly zero"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-lim, lim + 1, size=shape).astype(np.float32)
    a[rng.rand(*shape) < 0.33] = 0.0
    return a


def exact_units(S, extra=0.0):
    """the precondition of an exact test: the sum of |terms| (+ |bias| or |addend|) is whole and below 2^24"""
    n = units(f64(S) + extra, 1.0)
    assert n < LIMIT, "%g units: a partial sum may round" % n
    return n


def realistic(B, H, W, K, N, seed, bias_std=10.0):
    """post-ReLU activations (randn * 30 clipped at 0), He-scaled filters, a bias of standard deviation ``bias_std``,
    all float32"""
    rng = np.random.RandomState(seed)
    x = np.maximum(rng.randn(B, H, W, K), 0.0).astype(np.float32) * np.float32(30.0)
    w = (rng.randn(3, 3, K, N) * np.sqrt(2.0 / (9 * K))).astype(np.float32)
    bias = (rng.randn(N) * bias_std).astype(np.float32)
    return x, w, bias


def undecided(pre, bound):
    """where the sign of a pre-activation is not decided by the reference: |pre| <= bound"""
    return np.abs(f64(pre)) <= f64(bound)


# ---- reading a mismatch ---------------------------------------------------------------------------------------------------
def decode(flat, shape, m):
    """flat index into [B,H,W,C] -> 'image b tile (ty, tx) at (row, col) channel c' for m x m tiles (m: int or (mh, mw))"""
    mh, mw = (m, m) if np.isscalar(m) else m
    b, h, w, c = np.unravel_index(int(flat), shape)
    return "image %d tile (%d, %d) at (%d, %d) channel %d" % (b, h // mh, w // mw, h % mh, w % mw, c)


def first_mismatches(got, ref, bound, m, n=5):
    """a report of the first n entries where |got - ref| > bound (or got is not a number), decoded; '' when none"""
    got, ref = f64(got), f64(ref)
    bad = ~(np.abs(got - ref) <= f64(bound))
    idx = np.flatnonzero(bad)
    if idx.size == 0:
        return ""
    bb = np.broadcast_to(f64(bound), ref.shape).reshape(-1)
    lines = ["%d of %d entries outside the bound; the first:" % (idx.size, bad.size)]
    for i in idx[:n]:
        lines.append("  %s: got %r, reference %r, bound %.3g" % (decode(i, ref.shape, m), got.reshape(-1)[i],
                                                                 ref.reshape(-1)[i], bb[i]))
    return "\n".join(lines)


# ---- the cases of tests/test_conv_gpu.py (tests/test_conv_ref_cpu.py holds their inputs to the conditions above) -----------
# A layer (B, H, W, Ci, Co) runs forward with K = Ci, N = Co and its data gradient with K = Co, N = Ci.  The two strings are
# the paths the forward pass and the gradient are named for, as ``plan_key`` spells what nfs_conv3x3_plan reports:
# family / whole | ragged / schedule of the input and output transform (w six or seven waves, t thread per item, - none) /
# K parts.  The smallest shapes that reach each path (found with the plan query):
#   three kernels: six waves need C % 128 == 0 and T C <= 65536, so 192 and 576 channels reach the thread schedule at a
#   dozen tiles and (2, 48, 48, 256) passes 65536 items; two K parts need T <= 64 and K >= 512; 2 x 3 and 3 x 2 are the
#   smallest images Winograd takes; 12 x 16 and 13 x 11 images have 3 or 4 tile columns, so their tile rows and the two
#   images wrap inside one 16-row GEMM tile.
#   single kernel: K = 64 at any size, K = 128 from 128 blocks (300 when ragged) of 16 tiles x 64 output channels; 20 and
#   18 tiles leave a last run of 4 and 2 tiles, and 18 tiles of 3 images cross image boundaries inside a run.
#   F(5x5): where 49 tiles5 <= 0.9 x 36 tiles4 and both channel counts are >= 128.
PLAIN_LAYERS = [
    ((2, 12, 16, 128, 128), "wg4_three/whole/ww/k1", "wg4_three/whole/ww/k1"),
    ((2, 13, 11, 256, 256), "wg4_three/ragged/ww/k1", "wg4_three/ragged/ww/k1"),
    ((2, 12, 16, 192, 192), "wg4_three/whole/tt/k1", "wg4_three/whole/tt/k1"),
    ((2, 13, 11, 192, 192), "wg4_three/ragged/tt/k1", "wg4_three/ragged/tt/k1"),
    ((2, 13, 11, 256, 192), "wg4_three/ragged/wt/k1", "wg4_three/ragged/tw/k1"),
    ((1, 8, 8, 512, 512), "wg4_three/whole/ww/k2", "wg4_three/whole/ww/k2"),
    ((1, 7, 6, 512, 512), "wg4_three/ragged/ww/k2", "wg4_three/ragged/ww/k2"),
    ((1, 8, 8, 576, 576), "wg4_three/whole/tt/k2", "wg4_three/whole/tt/k2"),
    ((1, 7, 6, 576, 576), "wg4_three/ragged/tt/k2", "wg4_three/ragged/tt/k2"),
    ((2, 48, 48, 256, 256), "wg4_three/whole/tt/k1", "wg4_three/whole/tt/k1"),       # 73728 items
    ((1, 4, 4, 256, 256), "wg4_three/whole/ww/k1", "wg4_three/whole/ww/k1"),         # a single tile
    ((1, 2, 3, 256, 256), "wg4_three/ragged/ww/k1", "wg4_three/ragged/ww/k1"),
    ((1, 3, 2, 256, 256), "wg4_three/ragged/ww/k1", "wg4_three/ragged/ww/k1"),
    ((1, 16, 20, 64, 64), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((3, 9, 7, 64, 64), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((3, 8, 12, 64, 128), "wg4_single/whole/--/k1", "wg4_three/whole/wt/k1"),
    ((2, 13, 11, 64, 128), "wg4_single/ragged/--/k1", "wg4_three/ragged/wt/k1"),
    ((4, 64, 64, 128, 128), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((3, 113, 114, 128, 128), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((8, 64, 64, 128, 64), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((6, 113, 114, 128, 64), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((8, 64, 64, 64, 128), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),      # (the gradient's <128, 64> instance)
    ((6, 113, 114, 64, 128), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((1, 5, 5, 128, 128), "wg5/whole/ww/k1", "wg5/whole/ww/k1"),                     # one tile
    ((2, 9, 14, 128, 256), "wg5/ragged/ww/k1", "wg5/ragged/ww/k1"),
    ((2, 10, 10, 512, 512), "wg5/whole/ww/k2", "wg5/whole/ww/k2"),
    ((1, 9, 9, 512, 512), "wg5/ragged/ww/k2", "wg5/ragged/ww/k2"),
    ((6, 25, 25, 512, 512), "wg5/whole/tt/k1", "wg5/whole/tt/k1"),                   # 76800 items
    ((6, 24, 25, 512, 512), "wg5/ragged/tt/k1", "wg5/ragged/tt/k1"),
]
# pooled layers: odd sides wherever the shape is ragged (the pool floors, the pooled gradient is zero beyond it).  The
# gradient's second string is its path when it masks from the float output: that input transform has no six-wave form.
POOLED_LAYERS = [
    ((2, 12, 16, 128, 128), "wg4_three/whole/ww/k1", "wg4_three/whole/ww/k1", "wg4_three/whole/tw/k1"),
    ((2, 13, 11, 256, 256), "wg4_three/ragged/ww/k1", "wg4_three/ragged/ww/k1", "wg4_three/ragged/tw/k1"),
    ((2, 12, 16, 192, 192), "wg4_three/whole/tt/k1", "wg4_three/whole/tt/k1", "wg4_three/whole/tt/k1"),
    ((2, 13, 11, 192, 192), "wg4_three/ragged/tt/k1", "wg4_three/ragged/tt/k1", "wg4_three/ragged/tt/k1"),
    ((1, 8, 8, 512, 512), "wg4_three/whole/ww/k2", "wg4_three/whole/ww/k2", "wg4_three/whole/tw/k2"),
    ((1, 7, 9, 512, 512), "wg4_three/ragged/ww/k2", "wg4_three/ragged/ww/k2", "wg4_three/ragged/tw/k2"),
    ((1, 8, 8, 576, 576), "wg4_three/whole/tt/k2", "wg4_three/whole/tt/k2", "wg4_three/whole/tt/k2"),
    ((1, 7, 9, 576, 576), "wg4_three/ragged/tt/k2", "wg4_three/ragged/tt/k2", "wg4_three/ragged/tt/k2"),
    ((1, 16, 20, 64, 64), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((3, 9, 7, 64, 64), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((3, 8, 12, 64, 128), "wg4_single/whole/--/k1", "wg4_three/whole/wt/k1", "wg4_three/whole/tt/k1"),
    ((2, 13, 11, 64, 128), "wg4_single/ragged/--/k1", "wg4_three/ragged/wt/k1", "wg4_three/ragged/tt/k1"),
    ((4, 64, 64, 128, 128), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((3, 113, 115, 128, 128), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((8, 64, 64, 128, 64), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((6, 113, 115, 128, 64), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
    ((8, 64, 64, 64, 128), "wg4_single/whole/--/k1", "wg4_single/whole/--/k1", "wg4_single/whole/--/k1"),
    ((6, 113, 115, 64, 128), "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1", "wg4_single/ragged/--/k1"),
]
PRECISION_TILES = 300      # the float32 restatement is compared on the cases of at most this many tiles
RESTATED_CHANNELS = 32     # ... over the first 32 output channels (about 10^5 elements at 200 tiles)
UNDECIDED_CAP = 0.10


def plan_key(p):
    """'family/whole|ragged/<in><out>/k<parts>' of an ops.conv3x3_plan dict"""
    s = {1: "w", 0: "t", -1: "-"}
    return "%s/%s/%s%s/k%d" % (p["family"], "ragged" if p["ragged"] else "whole", s[p["in_waves"]], s[p["out_waves"]],
                               p["kparts"])


def tile_of(key):
    return 5 if key.startswith("wg5") else 4


def tiles(shape, m):
    return shape[0] * -(-shape[1] // m) * -(-shape[2] // m)


def layer_inputs(shape, pooled=False):
    """the realistic input of a layer case, float32: x, w, bias, the gradient gy (at the pooled resolution for a pooled
    layer) and an addend.  One seed per shape"""
    B, H, W, Ci, Co = shape
    seed = (B * 1000003 + H * 10007 + W * 101 + Ci * 7 + Co + (5 if pooled else 0)) % (2 ** 31)
    x, w, bias = realistic(B, H, W, Ci, Co, seed)
    rng = np.random.RandomState(seed + 1)
    gh, gw = (H // 2, W // 2) if pooled else (H, W)
    gy = rng.randn(B, gh, gw, Co).astype(np.float32)
    addend = rng.randn(B, H, W, Ci).astype(np.float32)
    return dict(x=x, w=w, bias=bias, gy=gy, addend=addend)
