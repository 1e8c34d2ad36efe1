"""Element-exact restatement of the histogram loss kernels (csrc/hist.hip: hist_loss_kernel and the hist_wide_*
pipeline), in the kernels' own float32 expressions, vectorised over the channels of an image.

Every discrete decision of the kernels -- the bin of each element, the template index each source bin maps to, the
bin an element reads its matched value from -- is taken here exactly as the kernels take it:
  sc = (v - vmin) / range;  k = clip(floor(255f * sc), 0, 254)                       (the two histograms)
  quantiles = cumsum / total in float64
  n = rint(j + (x - tq[j]) / (tq[j+1] - tq[j])), j the RIGHTMOST index with tq[j] <= x   (round half to even)
  lut[k] = (vmin + delta * n) + delta / 2                                             (float32)
  matched = lut[clip(int((v - vmin) / delta), 0, 254)]
so on inputs where no bin coordinate sits within rounding of a bin edge (``settle`` makes such inputs) the matched
value of every element is known exactly, and a kernel's gradient can be checked element by element.

``margin``: per element, the distance of its bin coordinates (255 * sc and (v - vmin) / delta) to the nearest bin
edge, in float32 ulps of the coordinate.  Edges where the clip makes both neighbours the same bin (0, and 255 and
beyond) are no decision and count as infinitely far.
"""
import numpy as np

HB = 255
F32 = np.float32


def _edge_ulps(u):
    """distance of float32 coordinates u >= 0 to the nearest decision edge 1..254, in ulps of u (inf: none near)"""
    r = np.rint(u)
    d = np.abs(u - r) / np.spacing(np.maximum(u, r).astype(F32))
    return np.where((r >= 1) & (r <= HB - 1), d, np.inf).astype(np.float64)


def _channel_tables(hs, ht):
    """the 255-entry table of template bins n[t, c] from the two histograms [255, C] (kernel steps 3-4)"""
    sq = np.cumsum(hs, axis=0).astype(np.float64)
    tq = np.cumsum(ht, axis=0).astype(np.float64)
    sq /= sq[-1:]
    tq /= tq[-1:]
    C = hs.shape[1]
    # rightmost j with tq[j] <= x: the count of template quantiles <= x, minus one (tq is non-decreasing)
    j = (tq.T[:, None, :] <= sq.T[:, :, None]).sum(-1).T - 1                  # [255, C]
    jc = np.clip(j, 0, HB - 2)
    cols = np.arange(C)[None, :]
    t0, t1 = tq[jc, cols], tq[jc + 1, cols]
    with np.errstate(invalid="ignore", divide="ignore"):
        y = jc.astype(np.float64) + (sq - t0) / (t1 - t0)
    n = np.clip(np.rint(np.where((sq >= tq[0:1]) & (sq < tq[-1:]), y, 0.0)), 0, HB - 1).astype(np.int64)
    n = np.where(sq < tq[0:1], 0, np.where(sq >= tq[-1:], HB - 1, n))
    return n, sq, tq


def reference(feat, templ, weight=1.0, mask=None, relu_mask=False, g_prefill=None):
    """feat [B, ..., C], templ [Bt, ..., C] float32, mask [B, ...] (pixels where it is 0 leave the source) or None.
    Image b matches against template min(b, Bt - 1).  Returns a dict:
      matched    [B, HW, C] float32 (the source value where the element is masked out or the channel skipped)
      grad       [B, HW, C] float32: g_prefill + 2w (v - matched) in the kernels' float32 order, 0 added where masked,
                 skipped or (relu_mask) v <= 0
      loss       [B] float64: w * sum of (v - matched)^2 over live elements, d in float32 as the kernels form it
      skip       [B, C] bool: channel has nothing to match (flat, or every source pixel masked out)
      vmin, vmax [B, C] float32 (the joint range; 0 where skipped)
      margin     [B, HW, C] float64: min of the two bin-coordinate margins of each live source element (inf elsewhere)
      margin_t   [B, HWt, C] float64: the histogram-coordinate margin of each template element under image b's range
      table      [B, 255, C] int64: the template bin n of each source bin"""
    f = np.ascontiguousarray(feat, F32)
    t = np.ascontiguousarray(templ, F32)
    B, C, Bt = f.shape[0], f.shape[-1], t.shape[0]
    f = f.reshape(B, -1, C)
    t = t.reshape(Bt, -1, C)
    HW, HWt = f.shape[1], t.shape[1]
    live = np.ones((B, HW), bool) if mask is None else (np.asarray(mask, F32).reshape(B, HW) != 0)
    w = F32(weight)
    out = dict(matched=f.copy(), grad=(np.zeros_like(f) if g_prefill is None else
                                       np.array(g_prefill, F32).reshape(B, HW, C)),
               loss=np.zeros(B), skip=np.ones((B, C), bool), vmin=np.zeros((B, C), F32), vmax=np.zeros((B, C), F32),
               margin=np.full((B, HW, C), np.inf), margin_t=np.full((B, HWt, C), np.inf),
               table=np.zeros((B, HB, C), np.int64))
    for b in range(B):
        lv = live[b]
        if not lv.any():
            continue
        s, tp = f[b][lv], t[min(b, Bt - 1)]
        vmax = np.maximum(s.max(0), tp.max(0))
        vmin = np.minimum(s.min(0), tp.min(0))
        skip = ~(vmax > vmin)
        rng_ = np.where(skip, F32(1), vmax - vmin).astype(F32)
        delta = (rng_ / F32(HB)).astype(F32)

        def coord(v):
            return (F32(HB) * ((v - vmin) / rng_)).astype(F32)

        def bins(u):
            return np.clip(np.floor(u).astype(np.int64), 0, HB - 1)

        us, ut = coord(s), coord(tp)
        cols = np.arange(C)[None, :]
        hs = np.bincount((bins(us) * C + cols).ravel(), minlength=HB * C).reshape(HB, C)
        ht = np.bincount((bins(ut) * C + cols).ravel(), minlength=HB * C).reshape(HB, C)
        n, _, _ = _channel_tables(hs, ht)
        lut = ((vmin + delta * n.astype(F32)) + delta * F32(0.5)).astype(F32)          # [255, C]
        a = ((s - vmin) / delta).astype(F32)
        m = lut[np.clip(a.astype(np.int64), 0, HB - 1), np.broadcast_to(cols, a.shape)]
        m = np.where(skip[None, :], s, m)
        d = (s - m).astype(F32)
        gsel = ~skip[None, :] & ((s > 0) if relu_mask else True)
        g = out["grad"][b][lv]
        g = np.where(gsel, (g + (F32(2) * w) * d).astype(F32), g)
        out["grad"][b][lv] = g
        out["matched"][b][lv] = m
        out["loss"][b] = float(w) * float((d.astype(np.float64) ** 2)[:, ~skip].sum())
        out["skip"][b] = skip
        out["vmin"][b] = np.where(skip, 0, vmin)
        out["vmax"][b] = np.where(skip, 0, vmax)
        mg = np.minimum(_edge_ulps(us), _edge_ulps(a))
        out["margin"][b][lv] = np.where(skip[None, :], np.inf, mg)
        out["margin_t"][b] = np.where(skip[None, :], np.inf, _edge_ulps(ut))
        out["table"][b] = n
    return out


def settle(feat, templ, mask=None, min_ulps=8.0, rounds=20):
    """copies of feat / templ in which every bin decision is unambiguous: each live source element and each template
    element whose margin (under the range of every image it is matched with) is below ``min_ulps`` moves to the
    centre of its histogram bin.  The range extremes have no decision and never move, so the ranges stay; moving a
    shared template element can put it near an edge of another image's bins, hence the rounds.  Raises ValueError if
    the inputs cannot be settled (a bin only a few ulps wide)."""
    f = np.array(feat, F32)
    t = np.array(templ, F32)
    B, C, Bt = f.shape[0], f.shape[-1], t.shape[0]
    fv = f.reshape(B, -1, C)
    tv = t.reshape(Bt, -1, C)
    for _ in range(rounds):
        r = reference(f, t, mask=mask)
        bad_s = r["margin"] < min_ulps
        bad_t = r["margin_t"] < min_ulps
        if not bad_s.any() and not bad_t.any():
            return f, t
        for b in range(B):
            vmin = r["vmin"][b].astype(np.float64)
            step = (r["vmax"][b].astype(np.float64) - vmin) / HB

            def centre(v):
                k = np.clip(np.floor((v - vmin) / np.where(step > 0, step, 1.0)), 0, HB - 1)
                return (vmin + (k + 0.5) * step).astype(F32)

            sel = bad_s[b]
            if sel.any():
                fv[b][sel] = np.broadcast_to(centre(fv[b].astype(np.float64)), fv[b].shape)[sel]
            sel = bad_t[b]
            if sel.any():
                bt = min(b, Bt - 1)
                tv[bt][sel] = np.broadcast_to(centre(tv[bt].astype(np.float64)), tv[bt].shape)[sel]
    raise ValueError("settle: bin decisions still within %g ulps after %d rounds" % (min_ulps, rounds))


def bin_centres(vmin, vmax, k):
    """float32 values in the middle of fixed-width bins k of [vmin, vmax]"""
    return (np.float64(vmin) + (np.asarray(k, np.float64) + 0.5) * ((np.float64(vmax) - vmin) / HB)).astype(F32)


def _with_ends(bins_, vmin, vmax, seed):
    """values at the centres of ``bins_`` (one per entry), the first of bin 0 replaced by vmin and the last of bin 254
    by vmax, in a fixed shuffled order"""
    v = bin_centres(vmin, vmax, bins_)
    v[np.flatnonzero(np.asarray(bins_) == 0)[0]] = vmin
    v[np.flatnonzero(np.asarray(bins_) == HB - 1)[-1]] = vmax
    return v[np.random.RandomState(seed).permutation(v.size)]


def half_tie_case(vmin, vmax):
    """(feat [1,16,32,1], templ [1,16,16,1]) whose table interpolates to EXACTLY k + 1/2 for every source bin k < 253:
    template 256 values, one per bin 0..253 and two in bin 254 (tq[j] = (2j + 2) / 512); source 512 values, three in
    bin 0, two in each of bins 1..253, three in bin 254 (sq[k] = (2k + 3) / 512).  Power-of-two totals: every quantile
    and every step of the interpolation is exact, so round-half-to-even decides every even k."""
    t = np.concatenate([np.arange(HB), [HB - 1]])
    s = np.concatenate([[0, 0, 0], np.repeat(np.arange(1, HB - 1), 2), [HB - 1] * 3])
    return (_with_ends(s, vmin, vmax, 1).reshape(1, 16, 32, 1), _with_ends(t, vmin, vmax, 2).reshape(1, 16, 16, 1))


def plateau_case(vmin, vmax, seed=0):
    """(feat [1,N,1], templ [1,2N,1]): a three-cluster source with long runs of empty bins and, as template, the same
    values twice -- identical quantile curves, so every source quantile EQUALS a template quantile, and after a source
    bin followed by empty bins that quantile is repeated: the rightmost-equal rule maps the bin past the run"""
    rng = np.random.RandomState(seed)
    occupied = np.concatenate([np.arange(0, 41), np.arange(100, 131), np.arange(201, HB)])
    bins_ = np.repeat(occupied, rng.randint(1, 4, occupied.size))
    s = _with_ends(bins_, vmin, vmax, seed)
    return s.reshape(1, -1, 1), np.concatenate([s, s[::-1]]).reshape(1, -1, 1)
