"""numpy restatement of the relief's definition (include/sdr/sdr.h, "the relief of a region"): the
pixel pipeline vectorised over the rectangle, every operation in the precision the definition
names (np.float32 where it says float, np.float64 where it says double, no fused operation), the
sums as integers, the quantiles from np.sort."""
import numpy as np

import plane_ref as PR
import ruler_ref as RR

DTYPE = np.dtype([
    ("q", "<f4", (8,)), ("h_min", "<f4"), ("h_max", "<f4"), ("mean", "<f8"), ("mean_above", "<f8"),
    ("sum256", "<i8"), ("sum256_above", "<i8"), ("area", "<i4"), ("n_masked", "<i4"), ("n_valid", "<i4"),
    ("n", "<i4"), ("n_above", "<i4"), ("n_below", "<i4"), ("n_rejected", "<i4"), ("frame", "<i4"),
    ("plane", "<i4"), ("label", "<i4"), ("flags", "<u4"), ("reserved", "<i4", (3,))])
VALID, OUT_OF_RANGE, NO_PLANE, EMPTY = 1, 2, 4, 8
F32, F64 = np.float32, np.float64
FLOATS = ("q", "h_min", "h_max", "mean", "mean_above")


def queries(regions):
    """(K, 7) int64 {frame, x0, y0, x1, y1, plane, label} from rows of 5, 6 or 7."""
    r = np.asarray(regions, np.int64)
    if r.size == 0:
        return np.zeros((0, 7), np.int64)
    r = r.reshape(-1, r.shape[-1])
    q = np.zeros((len(r), 7), np.int64)
    q[:, 6] = -1
    q[:, :r.shape[1]] = r[:, :7]
    return q


def heights(d, conf, lab, Q, plane, label, xs, ys, xe, ye, min_disp=-1.0, conf_min=0.0):
    """Steps 1 to 5 on the rectangle of one frame (d float32 (H, W)): (masked, valid, member bool
    (rh, rw), hf float32 (rh, rw), meaningful on members)."""
    win = d[ys:ye + 1, xs:xe + 1]
    masked = np.ones(win.shape, bool) if label < 0 else lab[ys:ye + 1, xs:xe + 1] == label
    cw = conf[ys:ye + 1, xs:xe + 1] if conf is not None else None
    valid = masked & RR.valid_mask(win, cw, min_disp, conf_min)
    yy, xx = np.mgrid[ys:ye + 1, xs:xe + 1]
    with np.errstate(all="ignore"):
        xyz = RR.reproject(Q, xx, yy, win.astype(F64))  # float32 (rh, rw, 3)
        n, off = np.asarray(plane["normal"], F64), F64(plane["offset"])
        X, Y, Z = (xyz[..., i].astype(F64) for i in range(3))
        h = ((n[0] * X + n[1] * Y) + n[2] * Z) + off
        hf = h.astype(F32) + F32(0.0)
        member = valid & np.isfinite(xyz).all(axis=-1) & (np.abs(hf) < F32(1048576.0))
    return masked, valid, member, hf


def relief(disp, planes, regions, Q, labels=None, conf=None, quantiles=(50, 500, 950), band=0.0, min_disp=-1.0,
           conf_min=0.0):
    """disp (F, H, W) float32 or int16; planes PLANE records; regions rows {frame, x0, y0, x1, y1,
    plane, label}; labels uint8 (F, H, W) / (H, W) or None: the DTYPE records."""
    d = RR.to_float(np.asarray(disp))
    if d.ndim == 2:
        d = d[None]
    F, H, W = d.shape
    if conf is not None:
        conf = np.asarray(conf, F32).reshape(F, H, W)
    if labels is not None:
        labels = np.asarray(labels, np.uint8).reshape(F, H, W)
    planes = np.asarray(planes).reshape(-1)
    qs = queries(regions)
    nq = len(quantiles)
    band = F32(band)
    out = np.zeros(len(qs), DTYPE)
    for k, (f, x0, y0, x1, y1, pi, label) in enumerate(qs.tolist()):
        r = out[k]
        for name in FLOATS:
            r[name] = np.nan
        r["frame"], r["plane"], r["label"] = f, pi, label
        if not RR.in_range((f, x0, y0, x1, y1), W, H, F) or not -1 <= label <= 255 or (label >= 0 and labels is None):
            r["flags"] = OUT_OF_RANGE
            continue
        xs, xe, ys, ye = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        r["area"] = (xe - xs + 1) * (ye - ys + 1)
        if not (0 <= pi < len(planes) and bool(planes[pi]["flags"] & PR.OK)):
            r["flags"] = NO_PLANE
            continue
        masked, valid, member, hf = heights(d[f], conf[f] if conf is not None else None,
                                            labels[f] if labels is not None else None, Q, planes[pi], label, xs, ys,
                                            xe, ye, min_disp, conf_min)
        r["n_masked"], r["n_valid"] = int(masked.sum()), int(valid.sum())
        v = np.sort(hf[member])  # no NaN among the members; -0 cannot occur
        n = len(v)
        r["n_rejected"] = int(valid.sum()) - n
        if n == 0:
            r["flags"] = EMPTY
            continue
        above = v > band
        e = np.rint(v.astype(F64) * F64(256.0)).astype(np.int64)
        s, sa, na = int(e.sum()), int(e[above].sum()), int(above.sum())
        r["n"], r["n_above"], r["n_below"] = n, na, int((v < -band).sum())
        r["h_min"], r["h_max"] = v[0], v[-1]
        r["sum256"], r["sum256_above"] = s, sa
        r["mean"] = (F64(s) / F64(n)) / F64(256.0)
        if na:
            r["mean_above"] = (F64(sa) / F64(na)) / F64(256.0)
        for j in range(nq):
            r["q"][j] = v[((n - 1) * int(quantiles[j])) // 1000]
        r["flags"] = VALID
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_reliefs_equal(got, want):
    """Floats and doubles as bit patterns (every NaN the canonical one), integers exactly."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = a != b
        assert not bad.any(), (name, np.argwhere(bad)[:4], got[name][bad][:4], want[name][bad][:4])
