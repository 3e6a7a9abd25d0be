"""numpy restatement of the clearance's definition (include/sdr/sdr.h, "the clearance of two labelled
things"): the members from the relief's pixel pipeline (relief_ref.heights) and the footprint's band,
each member's point from the lower median of its window's pixels of the same set (a stable sort, so
equal values keep the window's order) and ruler_ref.reproject, the closest pair by a chunked brute
force over all pairs in the precision the definition names (np.float32 where it says float,
np.float64 where it says double, no fused operation)."""
import numpy as np

import plane_ref as PR
import relief_ref as LR
import ruler_ref as RR

DTYPE = np.dtype([
    ("distance", "<f8"), ("along", "<f8"), ("across", "<f8"), ("p_a", "<f4", (3,)), ("p_b", "<f4", (3,)),
    ("d_a", "<f4"), ("d_b", "<f4"), ("xa", "<i4"), ("ya", "<i4"), ("xb", "<i4"), ("yb", "<i4"), ("area", "<i4"),
    ("n_a", "<i4"), ("n_b", "<i4"), ("m_a", "<i4"), ("m_b", "<i4"), ("frame", "<i4"), ("plane", "<i4"),
    ("label_a", "<i4"), ("label_b", "<i4"), ("flags", "<u4"), ("reserved", "<i4", (4,))])
VALID, OUT_OF_RANGE, NO_PLANE, EMPTY = 1, 2, 4, 8
MAX_QUERIES = 64
F32, F64 = np.float32, np.float64
FLOATS = ("distance", "along", "across", "p_a", "p_b", "d_a", "d_b")
PIXELS = ("xa", "ya", "xb", "yb")
CHUNK = 1 << 22  # pairs a chunk of the brute force


def queries(pairs):
    """(K, 8) int64 {frame, x0, y0, x1, y1, plane, label_a, label_b}."""
    r = np.asarray(pairs, np.int64)
    return r.reshape(-1, 8) if r.size else np.zeros((0, 8), np.int64)


def members(d, conf, lab, Q, plane, label, xs, ys, xe, ye, h_range, min_disp, conf_min):
    """bool (rh, rw): the members of the set of `label`."""
    _, _, member, hf = LR.heights(d, conf, lab, Q, plane, label, xs, ys, xe, ye, min_disp, conf_min)
    with np.errstate(all="ignore"):
        return member & (F32(h_range[0]) <= hf) & (hf <= F32(h_range[1]))


def medians(win, member, radius, min_count):
    """Each member's window of the rectangle restricted to the members: (has bool (rh, rw): at least
    min_count of them, d_med float32 (rh, rw): their lower median, the window's row-major order
    deciding among equal values)."""
    rh, rw = win.shape
    k = 2 * radius + 1
    vals = np.full((k * k, rh, rw), np.inf, F32)  # a member's disparity is finite: inf sorts behind them
    for j, (dy, dx) in enumerate((dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)):
        v0, v1 = max(0, -dy), rh - max(0, dy)
        u0, u1 = max(0, -dx), rw - max(0, dx)
        if v1 > v0 and u1 > u0:
            src = (slice(v0 + dy, v1 + dy), slice(u0 + dx, u1 + dx))
            vals[j][v0:v1, u0:u1] = np.where(member[src], win[src], F32(np.inf))
    n = np.isfinite(vals).sum(axis=0)
    order = np.argsort(vals, axis=0, kind="stable")
    pick = np.take_along_axis(order, (np.maximum(n, 1) - 1)[None] // 2, axis=0)
    dmed = np.take_along_axis(vals, pick, axis=0)[0]
    return member & (n >= min_count), dmed


def points(d, member, Q, xs, ys, radius, min_count):
    """The points of a set: (idx int64 (m,) ascending, xyz float32 (m, 3), d_med float32 (m,))."""
    rh, rw = member.shape
    has, dmed = medians(d[ys:ys + rh, xs:xs + rw], member, radius, min_count)
    vs, us = np.nonzero(has)  # row-major: ascending index
    dm = dmed[vs, us]
    with np.errstate(all="ignore"):
        xyz = RR.reproject(Q, xs + us, ys + vs, dm.astype(F64)).reshape(-1, 3)
    ok = np.isfinite(xyz).all(axis=-1)
    return (vs * rw + us)[ok].astype(np.int64), xyz[ok], dm[ok]


def pair_s(pa, pb):
    """s of every pair: float64 (len(pa), len(pb)) from the float32 differences."""
    with np.errstate(all="ignore"):
        v = [(pb[None, :, i] - pa[:, None, i]).astype(F64) for i in range(3)]  # float32 - float32
        return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def closest(pa, pb):
    """(i, j, s): the pair of the smallest s, ties to the smaller i, then j (the lists ascend in the
    pixel index, so the first minimum in row-major order of the (i, j) table is the definition's)."""
    best = None
    step = max(1, CHUNK // max(len(pb), 1))
    for i0 in range(0, len(pa), step):
        s = pair_s(pa[i0:i0 + step], pb)
        k = int(np.argmin(s))  # the first minimum; s holds no NaN
        i, j = divmod(k, len(pb))
        if best is None or s[i, j] < best[2]:
            best = (i0 + i, j, s[i, j])
    return best


def clearance(disp, planes, pairs, Q, labels, conf=None, radius=0, min_count=1, h_range=None, min_disp=-1.0,
              conf_min=0.0):
    """disp (F, H, W) / (H, W) float32 or int16; planes PLANE records; pairs rows {frame, x0, y0, x1,
    y1, plane, label_a, label_b}; labels uint8 (F, H, W) / (H, W): the DTYPE records."""
    d = RR.to_float(np.asarray(disp))
    if d.ndim == 2:
        d = d[None]
    F, H, W = d.shape
    if conf is not None:
        conf = np.asarray(conf, F32).reshape(F, H, W)
    labels = np.asarray(labels, np.uint8).reshape(F, H, W)
    planes = np.asarray(planes).reshape(-1)
    h_range = (-1048576.0, 1048576.0) if h_range is None else h_range
    qs = queries(pairs)
    out = np.zeros(len(qs), DTYPE)
    for k, (f, x0, y0, x1, y1, pi, la, lb) in enumerate(qs.tolist()):
        r = out[k]
        for name in FLOATS:
            r[name] = np.nan
        for name in PIXELS:
            r[name] = -1
        r["frame"], r["plane"], r["label_a"], r["label_b"] = f, pi, la, lb
        if not RR.in_range((f, x0, y0, x1, y1), W, H, F) or not 0 <= la <= 255 or not 0 <= lb <= 255 or la == lb:
            r["flags"] = OUT_OF_RANGE
            continue
        xs, xe, ys, ye = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        rw = xe - xs + 1
        r["area"] = rw * (ye - ys + 1)
        if not (0 <= pi < len(planes) and bool(planes[pi]["flags"] & PR.OK)):
            r["flags"] = NO_PLANE
            continue
        sets = []
        for label in (la, lb):
            m = members(d[f], conf[f] if conf is not None else None, labels[f], Q, planes[pi], label, xs, ys, xe, ye,
                        h_range, min_disp, conf_min)
            sets.append((int(m.sum()),) + points(d[f], m, Q, xs, ys, radius, min_count))
        (r["n_a"], ia, pa, da), (r["n_b"], ib, pb, db) = sets
        r["m_a"], r["m_b"] = len(ia), len(ib)
        if len(ia) == 0 or len(ib) == 0:
            r["flags"] = EMPTY
            continue
        i, j, s = closest(pa, pb)
        n = np.asarray(planes[pi]["normal"], F64)
        with np.errstate(all="ignore"):
            v = [F64(F32(pb[j][c]) - F32(pa[i][c])) for c in range(3)]
            al = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]
            t = s - al * al
            r["distance"] = RR.canon(np.sqrt(s))
            r["along"] = RR.canon(al)
            r["across"] = RR.canon(np.sqrt(t if t > 0.0 else F64(0.0)))
        r["p_a"], r["p_b"], r["d_a"], r["d_b"] = pa[i], pb[j], da[i], db[j]
        r["ya"], r["xa"] = ys + ia[i] // rw, xs + ia[i] % rw
        r["yb"], r["xb"] = ys + ib[j] // rw, xs + ib[j] % rw
        r["flags"] = VALID
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_clearances_equal(got, want):
    """Floats and doubles as bit patterns (every NaN the canonical one), integers exactly."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = a != b
        assert not np.any(bad), (name, np.argwhere(bad)[:4], got[name][bad][:4], want[name][bad][:4])
