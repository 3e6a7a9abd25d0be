"""The numpy restatement of the ruler over time (include/sdr/sdr.h, "the ruler over time"): one map
from a stack of F frames, vectorised over the pixels, with a plain loop over the frames wherever the
definition fixes an order (the rank's tie-break, the double sum, the extremes)."""
import numpy as np

MEAN, MEDIAN = 0, 1
MAX_FRAMES = 32
EMPTY, SPARSE, UNSTABLE, FUSED = 0, 1, 2, 3  # a pixel's class (not part of the ABI: the record counts them)

DTYPE = np.dtype([
    ("frames", "<i4"), ("width", "<i4"), ("height", "<i4"), ("mode", "<i4"), ("n_fused", "<i4"), ("n_empty", "<i4"),
    ("n_sparse", "<i4"), ("n_unstable", "<i4"), ("n_filled", "<i4"), ("n_replaced", "<i4"), ("sum_support", "<i8"),
    ("n_disagree", "<i8"), ("reserved", "<i8")])
assert DTYPE.itemsize == 64
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def to_float(stack):
    """The stack's values as the kernel reads them: int16 as (float)v * 0.0625f."""
    s = np.asarray(stack)
    if s.dtype == np.int16:
        return s.astype(np.float32) * np.float32(0.0625)
    assert s.dtype == np.float32
    return s


def valid_mask(v, conf, min_disp, conf_min):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v > np.float32(min_disp))
        if conf is not None:
            ok &= np.asarray(conf, np.float32) >= np.float32(conf_min)  # a NaN confidence fails
    return ok


def fuse(stack, conf=None, min_disp=-1.0, conf_min=0.0, tol=1.0, min_count=2, mode=MEAN, fill=None, classes=False):
    """(fused float32 (H, W), record DTYPE scalar, support uint8 (H, W), spread float32 (H, W)
    [, the pixels' classes]) of a stack (F, H, W), float32 px or int16 1/16 px."""
    v = to_float(stack)
    if v.ndim == 2:
        v = v[None]
    F, H, W = v.shape
    assert 1 <= F <= MAX_FRAMES
    fill = np.float32(min_disp if fill is None else fill)
    tol = np.float32(tol)
    ok = valid_mask(v, conf if conf is None else np.asarray(conf).reshape(v.shape), min_disp, conf_min)
    n = ok.sum(axis=0)
    # rank of frame k's value among the valid ones: those before it by <, equal ones in frame order
    rank = np.zeros((F, H, W), np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(F):
            for j in range(F):
                if j == k:
                    continue
                before = (v[j] < v[k]) | ((v[j] == v[k]) & (j < k))
                rank[k] += (ok[j] & before).astype(np.int32)
    want = (n - 1) // 2
    m = np.zeros((H, W), np.float32)
    for k in range(F):
        pick = ok[k] & (rank[k] == want)
        m = np.where(pick, v[k], m)
    with np.errstate(invalid="ignore", over="ignore"):
        agree = ok & (np.abs((v - m[None]).astype(np.float32)) <= tol)
    n_in = agree.sum(axis=0)
    s = np.zeros((H, W), np.float64)
    lo = np.zeros((H, W), np.float32)
    hi = np.zeros((H, W), np.float32)
    seen = np.zeros((H, W), bool)
    with np.errstate(invalid="ignore"):
        for k in range(F):
            a = agree[k]
            s = np.where(a, s + v[k].astype(np.float64), s)
            lo = np.where(a & (~seen | (v[k] < lo)), v[k], lo)
            hi = np.where(a & (~seen | (hi < v[k])), v[k], hi)
            seen |= a
    cls = np.full((H, W), FUSED, np.int32)
    cls[n_in < min_count] = UNSTABLE
    cls[(n_in < min_count) & (n < min_count)] = SPARSE
    cls[n == 0] = EMPTY
    fused = cls == FUSED
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (s / np.maximum(n_in, 1).astype(np.float64)).astype(np.float32)
    out = np.where(fused, m if mode == MEDIAN else mean, fill).astype(np.float32)
    support = np.where(fused, n_in, 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        spread = np.where(fused, (hi - lo).astype(np.float32), QNAN).astype(np.float32)
    rec = np.zeros(1, DTYPE)
    rec["frames"], rec["width"], rec["height"], rec["mode"] = F, W, H, mode
    rec["n_fused"] = int(fused.sum())
    rec["n_empty"] = int((cls == EMPTY).sum())
    rec["n_sparse"] = int((cls == SPARSE).sum())
    rec["n_unstable"] = int((cls == UNSTABLE).sum())
    rec["n_filled"] = int((fused & ~ok[F - 1]).sum())
    rec["n_replaced"] = int((fused & ok[F - 1] & ~agree[F - 1]).sum())
    rec["sum_support"] = int(n_in[fused].sum())
    rec["n_disagree"] = int((n - n_in)[fused].sum())
    res = (out, rec[0], support, spread)
    return res + (cls,) if classes else res


def fuse_loops(stack, conf=None, min_disp=-1.0, conf_min=0.0, tol=1.0, min_count=2, mode=MEAN, fill=None):
    """The same definition pixel by pixel in plain Python (the check of fuse() itself)."""
    v = to_float(stack)
    F, H, W = v.shape
    fill = np.float32(min_disp if fill is None else fill)
    out = np.empty((H, W), np.float32)
    support = np.zeros((H, W), np.uint8)
    spread = np.full((H, W), QNAN, np.float32)
    rec = np.zeros(1, DTYPE)[0]
    rec["frames"], rec["width"], rec["height"], rec["mode"] = F, W, H, mode
    for y in range(H):
        for x in range(W):
            vals = []  # (value, frame) of the valid ones
            for k in range(F):
                d = v[k, y, x]
                good = bool(np.isfinite(d)) and bool(d > np.float32(min_disp))
                if good and conf is not None:
                    good = bool(np.float32(conf[k, y, x]) >= np.float32(conf_min))
                if good:
                    vals.append((d, k))
            n = len(vals)
            out[y, x] = fill
            if n == 0:
                rec["n_empty"] += 1
                continue
            # a stable insertion sort by < : equal values keep the frame order
            order = []
            for item in vals:
                pos = len(order)
                while pos > 0 and item[0] < order[pos - 1][0]:
                    pos -= 1
                order.insert(pos, item)
            m = order[(n - 1) // 2][0]
            with np.errstate(over="ignore"):
                inl = [(d, k) for d, k in vals if np.abs(np.float32(d - m)) <= np.float32(tol)]
            n_in = len(inl)
            if n_in < min_count:
                rec["n_sparse" if n < min_count else "n_unstable"] += 1
                continue
            s = 0.0
            lo = hi = inl[0][0]
            for d, k in inl:
                s = s + float(d)
                if d < lo:
                    lo = d
                if hi < d:
                    hi = d
            out[y, x] = m if mode == MEDIAN else np.float32(s / float(n_in))
            support[y, x] = n_in
            spread[y, x] = np.float32(hi - lo)
            rec["n_fused"] += 1
            rec["sum_support"] += n_in
            rec["n_disagree"] += n - n_in
            last = [k for _, k in vals if k == F - 1]
            if not last:
                rec["n_filled"] += 1
            elif not [k for _, k in inl if k == F - 1]:
                rec["n_replaced"] += 1
    return out, rec, support, spread


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_fusion_equal(got, want):
    """(fused, record, support, spread) against the same: the maps on their bits (a None map of
    `got`, one the call did not ask for, is skipped), the record field by field."""
    g_out, g_rec, g_sup, g_spr = got
    w_out, w_rec, w_sup, w_spr = want[:4]
    g_out = np.asarray(g_out).reshape(w_out.shape)
    bad = np.argwhere(_bits(g_out) != _bits(w_out))
    assert bad.size == 0, f"fused: {len(bad)} pixels differ, first {bad[0]}: {g_out[tuple(bad[0])]!r} != {w_out[tuple(bad[0])]!r}"
    if g_sup is not None:
        bad = np.argwhere(np.asarray(g_sup) != w_sup)
        assert bad.size == 0, f"support: {len(bad)} pixels differ, first {bad[0]}"
    if g_spr is not None:
        bad = np.argwhere(_bits(g_spr) != _bits(w_spr))
        assert bad.size == 0, f"spread: {len(bad)} pixels differ, first {bad[0]}"
    if g_rec is not None:
        g_rec = np.asarray(g_rec).reshape(-1).view(np.uint8).view(DTYPE)[0]
        for name in DTYPE.names:
            assert g_rec[name] == w_rec[name], f"record.{name}: {g_rec[name]} != {w_rec[name]}"
