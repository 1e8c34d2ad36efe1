"""The Gram chain and the scalar losses restated in float64 numpy (no torch, no tiles, no slabs), the inputs on which
float32 arithmetic is exact, and the worst-case float32 bounds for everything else.

Exact inputs.  Every kernel here is sums of products.  With integer features (|F| <= 3), powers of two for every scale
and weight, and integer perturbations between a Gram matrix and its style target, every product and every partial sum
is an integer multiple of one power of two (the *unit*) and stays below 2^24 units, so float32 holds each of them
exactly in whatever order they are added -- an f32 MFMA (an fmaf chain), a slab reduce and a float atomic alike.  The
kernel's output must then EQUAL the float64 value: no tolerance is chosen.  ``units`` is the precondition; every exact
test asserts it on the CPU first.

Bounds (u = 2^-24, one float32 rounding):
  Gram entry     1.01 (HW + nslab + 4) u scale sum_p |F_pi F_pj|   one rounding per fma step, per slab add, the scale
  D = 2w(G-Gs)   2w 1.01 (that) + 2u |D|                           the subtraction and the product
  style loss     sum |D| (G's bound) + 1.01 (C^2 + P) u loss      first-order propagation + the summation (P partials)
  content grad   4u |g| (+ (2w/n) 2u (|f| + |amp t|) with a target) (+ u |g0 + g| accumulating)
  content loss   1.01 (n_b + 80) u sum |terms| per image
"""
import numpy as np

U = 2.0 ** -24
LIMIT = 2.0 ** 24


def f64(a):
    return np.asarray(a, dtype=np.float64)


def units(total_abs, unit):
    """the precondition of an exact test: ``total_abs`` (a float64 sum of |terms|, or an array of them) in units of the
    power of two ``unit``; below 2^24 every partial sum is a float32"""
    m, e = np.frexp(float(unit))
    assert m == 0.5 and e > -120, "unit %r is not a (normal) power of two" % (unit,)
    q = f64(total_abs) / float(unit)
    assert np.all(q == np.floor(q)), "terms are not whole units of %r" % (unit,)
    return float(np.max(q)) if np.size(q) else 0.0


def is_f32(a):
    """every value is a float32"""
    a = f64(a)
    with np.errstate(over="ignore"):
        return bool(np.all(a.astype(np.float32).astype(np.float64) == a))


# ---- Gram matrix and style loss ---------------------------------------------------------------------------------------
def per_image(scale, scale_dev, B):
    s = np.full(B, float(scale), np.float64)
    return s if scale_dev is None else s * f64(scale_dev)


def gram(F, scale, scale_dev=None):
    """F [B, ..., C] -> (G [B,C,C] = scale_b F_b^T F_b, the same sum over |terms|)"""
    F = f64(F)
    B, C = F.shape[0], F.shape[-1]
    F = F.reshape(B, -1, C)
    s = per_image(scale, scale_dev, B)[:, None, None]
    A = np.abs(F)
    return s * np.matmul(F.transpose(0, 2, 1), F), s * np.matmul(A.transpose(0, 2, 1), A)


def gram_bound(mag, HW, nslab):
    return 1.01 * (HW + nslab + 4) * U * f64(mag)


def style_loss(G, Gs, w):
    """(loss [B] = w sum (G_b - Gs_{b % Bs})^2, D [B,C,C] = 2 w (G_b - Gs_{b % Bs}))"""
    G, Gs = f64(G), f64(Gs)
    d = G - Gs[np.arange(G.shape[0]) % Gs.shape[0]]
    return float(w) * (d * d).sum(axis=(1, 2)), 2.0 * float(w) * d


def style_bounds(G, Gs, w, bG, parts):
    """(bound of D, bound of the per-image loss) from the bound ``bG`` of G"""
    loss, D = style_loss(G, Gs, w)
    C = G.shape[-1]
    return 2.0 * abs(float(w)) * 1.01 * bG + 2.0 * U * np.abs(D), \
        (np.abs(D) * bG).sum(axis=(1, 2)) + 1.01 * (C * C + parts) * U * loss


def gram_bwd(F, D, scale, scale_dev=None, relu_mask=False):
    """(dF [B,HW,C] = 2 scale_b F_b D_b (F > 0), its float32 bound C u 2 scale_b |F_b| |D_b|: one rounding per fma step)"""
    F, D = f64(F), f64(D)
    B, C = F.shape[0], F.shape[-1]
    shape = F.shape
    F = F.reshape(B, -1, C)
    a = 2.0 * per_image(scale, scale_dev, B)[:, None, None]
    m = (F > 0) if relu_mask else 1.0
    return (a * np.matmul(F, D) * m).reshape(shape), (C * U * a * np.matmul(np.abs(F), np.abs(D)) * m).reshape(shape)


# ---- content loss -----------------------------------------------------------------------------------------------------
def content_loss(F, weight, channel=0, target=None, amp=100.0, signed=False, g0=None):
    """The content term on F [B, ..., C] (its means run over the whole batch; image b holds its own share):
         target given:   mean((F - amp target_{b % Bt})^2)
         channel c != 0: -mean(F[..., c]) + mean|F[..., :c]| + mean|F[..., c+1:]|   (an empty slice contributes nothing)
         otherwise:      -mean(F)
       unsigned (F is a ReLU output, |f| = f): the gradient is the one wrt the pre-activation, nothing where f <= 0;
       ``signed``: |f| proper, d|f| = sign(f) (0 at 0), the gradient goes to every element.
       Returns loss [B], grad, sum |terms| [B], and the bounds of both (grad's with ``g0`` when accumulated onto it)."""
    F = f64(F)
    B, C = F.shape[0], F.shape[-1]
    n_all = float(F.size)
    n_pix = n_all / C
    w = float(weight)
    extra = 0.0
    if target is not None:
        t = f64(target)
        t = t[np.arange(B) % t.shape[0]]
        diff = F - amp * t
        term = w / n_all * diff * diff
        grad = 2.0 * w / n_all * diff
        extra = 2.0 * w / n_all * 2.0 * U * (np.abs(F) + np.abs(amp * t))
    elif channel:
        c = int(channel)
        k = np.empty(C)
        k[:c] = w / (n_pix * c)
        k[c] = -w / n_pix
        k[c + 1:] = w / (n_pix * (C - c - 1)) if c + 1 < C else 0.0
        off = np.arange(C) != c
        if signed:
            term = np.where(off, k * np.abs(F), k * F)
            grad = np.where(off, k * np.sign(F), k * np.ones_like(F))
        else:
            term = k * F
            grad = k * np.ones_like(F)
    else:
        term = -w / n_all * F
        grad = -w / n_all * np.ones_like(F)
    if not signed:
        grad = np.where(F > 0, grad, 0.0)
    ax = tuple(range(1, F.ndim))
    mag = np.abs(term).sum(axis=ax)
    n_b = F[0].size
    g_bound = 4.0 * U * np.abs(grad) + extra * (grad != 0)
    if g0 is not None:
        g_bound = np.where(grad != 0, g_bound + U * np.abs(f64(g0) + grad), 0.0)
        grad = f64(g0) + grad
    return dict(loss=term.sum(axis=ax), grad=grad, mag=mag, loss_bound=1.01 * (n_b + 80) * U * mag, grad_bound=g_bound)


# ---- total variation --------------------------------------------------------------------------------------------------
def tv(x, weight):
    """x [B,H,W,C]: loss = weight / B sum (|dh| + |dw|) and its gradient weight / B k, k the integer in -4 .. 4 that
    counts the signs of the four differences an element takes part in -- sign(0) = 0: a tie moves neither element.
    Also sum (|dh| + |dw|) itself, the integer k, and the share of differences that are ties."""
    x = f64(x)
    B = x.shape[0]
    dh = x[:, 1:] - x[:, :-1]
    dw = x[:, :, 1:] - x[:, :, :-1]
    k = np.zeros_like(x)
    k[:, :-1] -= np.sign(dh)
    k[:, 1:] += np.sign(dh)
    k[:, :, :-1] -= np.sign(dw)
    k[:, :, 1:] += np.sign(dw)
    total = np.abs(dh).sum() + np.abs(dw).sum()
    ndiff = dh.size + dw.size
    ties = ((dh == 0).sum() + (dw == 0).sum()) / float(ndiff) if ndiff else 1.0
    s = float(weight) / B
    return dict(loss=s * total, grad=s * k, total=total, k=k, ties=ties, scale=s)


# ---- 2x2 VALID average pool -------------------------------------------------------------------------------------------
def avgpool2(x):
    """x [B,H,W,C] -> [B,H//2,W//2,C]: odd sides floor (a window exists where its lower right element does)"""
    x = f64(x)
    H2, W2 = x.shape[1] // 2, x.shape[2] // 2
    v = x[:, :2 * H2, :2 * W2]
    return 0.25 * (v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2])


def avgpool2_bwd(gy, shape, x=None, addend=None):
    """the adjoint: gy / 4 to each element of a window, 0 beyond 2 (H//2), 2 (W//2); times (x > 0); plus the addend"""
    gy = f64(gy)
    g = np.zeros(shape)
    H2, W2 = shape[1] // 2, shape[2] // 2
    for i in (0, 1):
        for j in (0, 1):
            g[:, i:2 * H2:2, j:2 * W2:2] = 0.25 * gy
    if x is not None:
        g = g * (f64(x) > 0)
    if addend is not None:
        g = g + f64(addend)
    return g


# ---- style mask -------------------------------------------------------------------------------------------------------
def style_mask_apply(F, m):
    """F [B,h,w,C], m [B,h,w,1] -> (F m, scale [B] = 1 / (2 area_b C), area_b = sum of m over the image)"""
    F, m = f64(F), f64(m).reshape(F.shape[:-1] + (1,))
    area = m.reshape(F.shape[0], -1).sum(axis=1)
    with np.errstate(divide="ignore"):
        return F * m, 1.0 / (2.0 * area * F.shape[-1])


def style_mask_bwd(dFm, m, F):
    """dFm m (F > 0): the gradient wrt the pre-activation of the masked ReLU feature"""
    F = f64(F)
    return f64(dFm) * f64(m).reshape(F.shape[:-1] + (1,)) * (F > 0)


# ---- exact inputs -----------------------------------------------------------------------------------------------------
def int_features(B, HW, C, seed, lo=-3, hi=3):
    """integers in lo .. hi, a third of them forced to exact zero"""
    rng = np.random.RandomState(seed)
    F = rng.randint(lo, hi + 1, size=(B, HW, C)).astype(np.float32)
    F[rng.rand(B, HW, C) < 0.33] = 0.0
    return F


MARK_PIXELS = (0, 31, 32, -1)
MARK_CHANNELS = (0, 63, 64, -1)
MARK_A = (0, 1, 3, 7)      # a Sidon set: the ten sums a_j + a_k name the ten channel pairs


def marker_features(B, HW, C):
    """zero but for pixels {0, 31, 32, HW-1} x channels {0, 63, 64, C-1}; F[pixel i, channel j] = 2^(i + 8 a_j), image b
    shifted by 2^b.  G[c_j, c_k] = 4^b 2^(8 (a_j + a_k)) sum over the pixels i that reached it of 4^i: the exponent names
    the channel pair and the mantissa the pixels (``marker_decode``).  7 mantissa bits: exact in float32"""
    assert HW >= 34 and C >= 128
    F = np.zeros((B, HW, C), np.float32)
    for b in range(B):
        for i, p in enumerate(MARK_PIXELS):
            for j, c in enumerate(MARK_CHANNELS):
                F[b, p, c] = 2.0 ** (b + i + 8 * MARK_A[j])
    return F


def marker_decode(v, b=0):
    """what an entry of the marker Gram says: the channel-pair sum a_j + a_k and the pixels (0..3) that reached it"""
    v = float(v) / 4.0 ** b
    if v == 0.0:
        return "nothing"
    if not np.isfinite(v) or v < 0:
        return repr(v)
    q = int(np.floor(np.log2(v))) // 8
    m = v / 2.0 ** (8 * q)
    if m != np.floor(m) or int(m) & 0xAA:
        return "%r (no marker pattern)" % v
    px = [MARK_PIXELS[i] for i in range(4) if (int(m) >> (2 * i)) & 1]
    return "pair a_j+a_k = %d, pixels %s" % (q, px)


def tile_E(B, C, where, seed):
    """a symmetric integer perturbation |e| <= 3 [B,C,C] confined to one 64 x 64 tile (and its mirror image):
    'diag' tile (0, 0) -- (1, 1) where there are more than two --, 'off' tile (0, last) and (last, 0), 'last' the last diagonal
    tile, 'full' every entry"""
    rng = np.random.RandomState(seed)
    n = C // 64
    E = np.zeros((B, C, C))
    R = rng.randint(-3, 4, size=(B, C, C)).astype(np.float64)
    if where == "full":
        E = np.triu(R) + np.triu(R, 1).transpose(0, 2, 1)
        return E
    t1, t2 = {"diag": (1 if n > 2 else 0,) * 2, "off": (0, n - 1), "last": (n - 1, n - 1)}[where]
    r, c = slice(64 * t1, 64 * t1 + 64), slice(64 * t2, 64 * t2 + 64)
    if t1 == t2:
        blk = R[:, r, c]
        E[:, r, c] = np.triu(blk) + np.triu(blk, 1).transpose(0, 2, 1)
    else:
        E[:, r, c] = R[:, r, c]
        E[:, c, r] = R[:, r, c].transpose(0, 2, 1)
    return E


def style_case(B, Bs, C, where, seed, HW=6, k=3, wexp=-2, preload_exp=20):
    """the exact style-loss input: integer features |F| <= 1 (small sums, so that G_b - Gs_{b % Bs} stays small for
    b >= Bs too), scale 2^-k, Gs_i = G_i - 2^-k E_i, weight 2^wexp, loss_acc pre-loaded with 2^preload_exp units.
    Checks the precondition and returns everything a test needs."""
    F = int_features(B, HW, C, seed, -1, 1)
    s, w = 2.0 ** -k, 2.0 ** wexp
    G, mag = gram(F, s)
    E = tile_E(Bs, C, where, seed + 1)
    Gs = G[:Bs] - s * E
    unit = w * s * s
    loss, D = style_loss(G, Gs, w)
    d = (G - Gs[np.arange(B) % Bs]) / s
    pre = 2.0 ** preload_exp * unit
    assert units(mag, s) < LIMIT and is_f32(G) and is_f32(Gs)
    assert np.abs(d).max() < 2 ** 12                                   # d^2 < 2^24: every square is exact
    assert units(loss + pre, unit) < LIMIT and units(np.abs(D), 2 * w * s) < LIMIT
    if Bs == B:
        assert np.array_equal(D, 2 * w * s * E)
    return dict(F=F, s=s, w=w, G=G, Gs=Gs, E=E, loss=loss, D=D, pre=pre, unit=unit)


# (B, HW, C) of nfs_gram_fwd and the path each takes on a chip of ~256 compute units: 'one' slab (the tile kernel writes G
# itself), 'few' (a reduce with fewer slabs than its 4 waves), 'many', 'capped' (4-chunk slabs would be more than the
# reduce fan-in of 256).  The plan depends on the CU count; a test reads it back and does not assume it.
GRAM_SHAPES = [((1, 1, 64), "one"), ((1, 32, 64), "one"), ((1, 33, 128), "one"), ((2, 300, 64), "few"),
               ((3, 5003, 64), "many"), ((1, 1000, 128), "many"), ((3, 37, 256), "one"), ((8, 144, 512), "one"),
               ((1, 32801, 64), "capped")]


def on_path(path, nslab, HW):
    chunks = (HW + 31) // 32
    if path == "capped":
        return (chunks + 3) // 4 > 256 and nslab == (chunks + (chunks + 255) // 256 - 1) // ((chunks + 255) // 256)
    return {"one": nslab == 1, "few": 1 < nslab < 4, "many": nslab > 4}[path]


def gram_case(shape, k=3, with_dev=False, seed=None):
    """the exact Gram input of a shape: integer features, scale 2^-k, scale_dev[b] = 2^-(b+1); precondition checked"""
    B, HW, C = shape
    F = int_features(B, HW, C, 1000 * B + HW + C if seed is None else seed)
    s = 2.0 ** -k
    dev = 2.0 ** -(np.arange(B) + 1.0) if with_dev else None
    G, mag = gram(F, s, dev)
    for b, sb in enumerate(per_image(s, dev, B)):
        assert units(mag[b], sb) < LIMIT
    assert is_f32(G) and np.array_equal(G, G.transpose(0, 2, 1))
    return dict(F=F, s=s, dev=None if dev is None else dev.astype(np.float32), G=G, mag=mag)


# (HW, C, kind of style Gram) of the grouped call: 'full' a random integer Gs (D exact on every tile, the loss bounded),
# otherwise a tile-confined E (the loss exact too).  1025 pixels: three 16-chunk slabs, the last of one pixel; 1024: 32
# chunks, the longest image that is one slab.  Slab layers and one-slab layers of both kinds.
GROUP_LAYERS = [(1600, 64, "full"), (1295, 128, "off"), (1025, 64, "diag"), (1024, 64, "last"), (30, 512, "full"),
                (9, 512, "diag"), (600, 64, "full")]


def group_plan(layers, B):
    """(workspace floats, loss partials) of a grouped call: a layer of more than 32 chunks has 16-chunk slabs, a reduce
    block owns 4 rows of a tile (16 partials per tile pair); a shorter one is one slab (one partial per tile pair)"""
    ws = parts = 0
    for HW, C in layers:
        chunks, npair = (HW + 31) // 32, (C // 64) * (C // 64 + 1) // 2
        if chunks > 32:
            ws += B * npair * ((chunks + 15) // 16) * 4096
            parts += npair * 16
        else:
            parts += npair
    return ws, parts


def group_case(B, Bs, layers, seed=7):
    """the exact input of a grouped call, one dict per layer (HW, C, kind[, ch]).  Images b >= Bs are image b % Bs with
    its pixels permuted and its sign flipped: other data, the same Gram matrix, so that G_b - Gs_{b % Bs} is the small
    E there too.  With ``ch`` the channels from ch on are zero padding and the scale is 1 / (2 HW ch) (which must be a
    power of two); without, 2^-(3 + l % 3)."""
    out = []
    for l, (HW, C, kind, *ch) in enumerate(layers):
        rng = np.random.RandomState(seed + 31 * l)
        F = int_features(B, HW, C, seed + 31 * l + 1)
        if ch:
            F[..., ch[0]:] = 0.0
        for b in range(Bs, B):
            F[b] = -F[b % Bs][rng.permutation(HW)]
        s, w = 1.0 / (2.0 * HW * ch[0]) if ch else 2.0 ** -(3 + l % 3), 2.0 ** -(1 + l % 2)
        G, mag = gram(F, s)
        assert units(mag, s) < LIMIT and is_f32(G)
        if kind == "full":
            M = rng.randint(0, 1025, size=(Bs, C, C)).astype(np.float64)
            Gs = s * (np.triu(M) + np.triu(M, 1).transpose(0, 2, 1))
        else:
            Gs = G[:Bs] - s * tile_E(Bs, C, kind, seed + 31 * l + 2)
        loss, D = style_loss(G, Gs, w)
        assert is_f32(Gs) and units(np.abs(D), 2 * w * s) < LIMIT
        exact = kind != "full"
        if exact:
            assert np.abs(G - Gs[np.arange(B) % Bs]).max() / s < 2 ** 12 and units(loss, w * s * s) < LIMIT
        out.append(dict(HW=HW, C=C, ch=ch[0] if ch else C, F=F, s=s, w=w, G=G, Gs=Gs, D=D, loss=loss, exact=exact))
    return out


# nine layers (HW, C, kind, logical channels) with HW ch a power of two, for ops.gram_style_group: more than the eight
# of one launch, zero-padded layers whose denominator counts the logical channels, 2048 pixels in four slabs
SPLIT_LAYERS = [(4, 64, "diag", 64), (16, 64, "diag", 32), (32, 128, "off", 128), (64, 64, "last", 64),
                (128, 128, "diag", 64), (256, 64, "diag", 64), (512, 64, "last", 16), (1024, 128, "last", 128),
                (2048, 64, "diag", 64)]


def tv_image(shape, seed):
    """integer-valued 0 .. 255: along the longer side a third of random values, a third of zero background and a third of
    one constant per channel, so that most neighbour differences are exact ties"""
    B, H, W, C = shape
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, size=shape).astype(np.float32)
    const = rng.randint(1, 256, size=C).astype(np.float32)
    if W >= H:
        x[:, :, W // 3:2 * W // 3] = 0.0
        x[:, :, 2 * W // 3:] = const
    else:
        x[:, H // 3:2 * H // 3] = 0.0
        x[:, 2 * H // 3:] = const
    return x


def mask01(B, h, w, areas, seed):
    """a 0/1 mask [B,h,w,1] with exactly areas[b] ones in image b"""
    rng = np.random.RandomState(seed)
    m = np.zeros((B, h * w), np.float32)
    for b in range(B):
        m[b, rng.permutation(h * w)[:areas[b]]] = 1.0
    return m.reshape(B, h, w, 1)


def err_ratio(err, bound):
    """largest err / bound: 0 where the error is zero, inf where an error meets a zero bound or is not a number"""
    err, bound = f64(err), f64(bound)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(np.where(np.isfinite(r), r, np.inf)))
