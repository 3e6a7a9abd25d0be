"""numpy restatement of the objects' definition (include/sdr/sdr.h, "the objects of a region"): the
members from the relief's pixel pipeline (relief_ref.heights) and the footprint's band, the joins
from float32 differences of the disparities, the components by min-label propagation (each pixel
takes the smallest label among itself and the neighbours it is joined to, then the label of its
label, until nothing changes), the ranking by np.lexsort, the records from integer sums."""
import numpy as np

import plane_ref as PR
import relief_ref as LR
import ruler_ref as RR

OBJECT_DTYPE = np.dtype([
    ("n", "<i4"), ("root", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("sum_x", "<i8"),
    ("sum_y", "<i8"), ("sum256", "<i8"), ("h_min", "<f4"), ("h_max", "<f4"), ("flags", "<u4"), ("reserved", "<i4")])
SCAN_DTYPE = np.dtype([
    ("flags", "<u4"), ("area", "<i4"), ("n_masked", "<i4"), ("n_valid", "<i4"), ("n", "<i4"),
    ("n_components", "<i4"), ("n_kept", "<i4"), ("count", "<i4"), ("largest_dropped", "<i4"), ("frame", "<i4"),
    ("plane", "<i4"), ("label", "<i4"), ("reserved", "<i4", (4,))])
VALID, OUT_OF_RANGE, NO_PLANE, EMPTY, TRUNCATED = 1, 2, 4, 8, 16
OBJECT_VALID, OBJECT_CUT = 1, 2
F32, F64 = np.float32, np.float64

NEIGHBOURS4 = ((0, 1), (1, 0))
NEIGHBOURS8 = ((0, 1), (1, 0), (1, 1), (1, -1))  # each pair once: (dv, du), the other end by symmetry


def joins(member, d, max_diff, connectivity):
    """[(dv, du, bool (rh, rw))]: pixel (v, u) is joined to (v + dv, u + du)."""
    rh, rw = member.shape
    out = []
    with np.errstate(all="ignore"):
        for dv, du in (NEIGHBOURS8 if connectivity == 8 else NEIGHBOURS4):
            j = np.zeros((rh, rw), bool)
            v0, v1 = max(0, -dv), rh - max(0, dv)
            u0, u1 = max(0, -du), rw - max(0, du)
            if v1 > v0 and u1 > u0:
                a = (slice(v0, v1), slice(u0, u1))
                b = (slice(v0 + dv, v1 + dv), slice(u0 + du, u1 + du))
                j[a] = member[a] & member[b] & (np.abs(d[a] - d[b]) <= F32(max_diff))  # float32 - float32
            out.append((dv, du, j))
    return out


def components(member, d, max_diff, connectivity):
    """int64 (rh, rw): each member's root (the smallest row-major index of its component), -1 on
    the others."""
    rh, rw = member.shape
    big = rh * rw
    lab = np.where(member, np.arange(big).reshape(rh, rw), big).astype(np.int64)
    ends = [(np.nonzero(j), dv, du) for dv, du, j in joins(member, d, max_diff, connectivity)]
    while True:
        new = lab.copy()
        for (vs, us), dv, du in ends:  # each end of a join appears once in its index arrays
            m = np.minimum(new[vs, us], new[vs + dv, us + du])
            new[vs, us] = m
            new[vs + dv, us + du] = np.minimum(new[vs + dv, us + du], m)  # a pixel may be both ends
        flat = np.append(new.reshape(-1), big)  # the label of a label (big maps to itself)
        for _ in range(4):
            flat = flat[flat]
        new = flat[:big].reshape(rh, rw)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(member, lab, -1)


def empty_objects(n):
    o = np.zeros(n, OBJECT_DTYPE)
    for name in ("root", "x0", "y0", "x1", "y1"):
        o[name] = -1
    o["h_min"] = o["h_max"] = np.nan
    return o


def find_objects(disp, planes, region, Q, labels=None, conf=None, h_range=(10.0, 1048576.0), max_diff=1.0,
                 connectivity=8, min_pixels=64, max_objects=16, min_disp=-1.0, conf_min=0.0):
    """disp (F, H, W) / (H, W) float32 or int16; planes PLANE records; region one row {frame, x0, y0,
    x1, y1, plane, label}; labels uint8 (F, H, W) / (H, W) or None.  Returns (all max_objects
    OBJECT_DTYPE records, one SCAN_DTYPE record, the (H, W) uint8 label map, the (rh, rw) root map or
    None when refused)."""
    raw = np.asarray(disp)
    d = RR.to_float(raw)
    if d.ndim == 2:
        d = d[None]
    F, H, W = d.shape
    if conf is not None:
        conf = np.asarray(conf, F32).reshape(F, H, W)
    if labels is not None:
        labels = np.asarray(labels, np.uint8).reshape(F, H, W)
    planes = np.asarray(planes).reshape(-1)
    (f, x0, y0, x1, y1, pi, label), = LR.queries(region).tolist()
    objs = empty_objects(max_objects)
    scan = np.zeros(1, SCAN_DTYPE)[0]
    lab_out = np.full((H, W), 255, np.uint8)
    scan["frame"], scan["plane"], scan["label"] = f, pi, label
    if not RR.in_range((f, x0, y0, x1, y1), W, H, F) or not -1 <= label <= 255 or (label >= 0 and labels is None):
        scan["flags"] = OUT_OF_RANGE
        return objs, scan, lab_out, None
    xs, xe, ys, ye = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    rw = xe - xs + 1
    scan["area"] = rw * (ye - ys + 1)
    if not (0 <= pi < len(planes) and bool(planes[pi]["flags"] & PR.OK)):
        scan["flags"] = NO_PLANE
        return objs, scan, lab_out, None
    masked, valid, member, hf = LR.heights(d[f], conf[f] if conf is not None else None,
                                           labels[f] if labels is not None else None, Q, planes[pi], label, xs, ys,
                                           xe, ye, min_disp, conf_min)
    with np.errstate(all="ignore"):
        member = member & (F32(h_range[0]) <= hf) & (hf <= F32(h_range[1]))
    scan["n_masked"], scan["n_valid"], scan["n"] = int(masked.sum()), int(valid.sum()), int(member.sum())
    roots = components(member, d[f][ys:ye + 1, xs:xe + 1], max_diff, connectivity)
    ids, sizes = np.unique(roots[member], return_counts=True)
    scan["n_components"] = len(ids)
    keep = sizes >= min_pixels
    scan["n_kept"] = int(keep.sum())
    scan["largest_dropped"] = int(sizes[~keep].max()) if (~keep).any() else 0
    kid, ksz = ids[keep], sizes[keep]
    order = np.lexsort((kid, -ksz))  # size descending, ties to the lower root
    count = min(len(order), max_objects)
    scan["count"] = count
    scan["flags"] = (VALID if scan["n_kept"] else EMPTY) | (TRUNCATED if scan["n_kept"] > max_objects else 0)
    for k in range(count):
        r, n = int(kid[order[k]]), int(ksz[order[k]])
        m = roots == r
        vs, us = np.nonzero(m)
        h = hf[m]
        o = objs[k]
        o["n"], o["root"] = n, r
        o["x0"], o["x1"], o["y0"], o["y1"] = xs + us.min(), xs + us.max(), ys + vs.min(), ys + vs.max()
        o["sum_x"], o["sum_y"] = int((xs + us).sum()), int((ys + vs).sum())
        o["sum256"] = int(np.rint(h.astype(F64) * F64(256.0)).astype(np.int64).sum())
        o["h_min"], o["h_max"] = h.min(), h.max()
        cut = o["x0"] == xs or o["x1"] == xe or o["y0"] == ys or o["y1"] == ye
        o["flags"] = OBJECT_VALID | (OBJECT_CUT if cut else 0)
        lab_out[ys:ye + 1, xs:xe + 1][m] = k
    return objs, scan, lab_out, roots


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_records_equal(got, want, dtype):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in dtype.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = a != b
        assert not np.any(bad), (name, np.argwhere(bad)[:4], got[name][bad][:4], want[name][bad][:4])


def assert_objects_equal(got, want):
    """(objects, scan, labels) against the restatement's: floats as bit patterns (every NaN the
    canonical one), integers exactly, the label maps on every pixel (labels None: not compared)."""
    assert_records_equal(got[0], want[0], OBJECT_DTYPE)
    assert_records_equal(got[1], want[1], SCAN_DTYPE)
    if got[2] is not None:
        a, b = np.asarray(got[2]), np.asarray(want[2])
        assert a.shape == b.shape and a.dtype == np.uint8
        bad = a != b
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], a[bad][:4], b[bad][:4])


# ---- the scene of the feature's tests: footprint_ref.box_scene's geometry with a hemisphere beside the box
def two_object_scene(Q, L=150.0, Wd=100.0, ang=25.0, H=240, W=320, sigma=0.15, holes=0.20, outliers=0.05, seed=3,
                     radius=60.0):
    """The floor of footprint_ref.box_scene; the box top (L x Wd mm, 150 mm above the floor) centred
    at P0 + 150 n - 80 e_s - 60 e_t; a hemisphere: the nearest intersection with the sphere of
    `radius` about P0 + 70 e_s + 40 e_t where it is nearer than the floor and not under the box.
    Noise, holes and outliers are drawn as box_scene draws them.  Returns (disp float32 (1, H, W),
    truth (H, W): 0 floor, 1 box, 2 hemisphere, -1 on holes and outliers, info)."""
    import footprint_ref as FR

    rng = np.random.default_rng(seed)
    n = np.array([0.05, -np.cos(np.radians(50.0)), -np.sin(np.radians(50.0))])
    n /= np.linalg.norm(n)
    P0 = np.array([0.0, 0.0, 1200.0])
    es, et = FR.basis(n)
    C = P0 + 150.0 * n - 80.0 * es - 60.0 * et
    Cs = P0 + 70.0 * es + 40.0 * et
    ca, sa = np.cos(np.radians(ang)), np.sin(np.radians(ang))
    ax, bx = ca * es + sa * et, -sa * es + ca * et
    f = Q[2, 3]
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.stack([xx + Q[0, 3], yy + Q[1, 3], np.full((H, W), f)], axis=-1) / f  # rays with Z = 1
    tb = np.dot(n, C) / (D @ n)
    Pb = D * tb[..., None]
    box = (np.abs((Pb - C) @ ax) <= L / 2) & (np.abs((Pb - C) @ bx) <= Wd / 2) & (tb > 0)
    tf = np.dot(n, P0) / (D @ n)
    # |t D - Cs|^2 = radius^2: the nearer root
    a2, b2, c2 = (D * D).sum(-1), D @ Cs, float(Cs @ Cs) - radius * radius
    disc = b2 * b2 - a2 * c2
    with np.errstate(all="ignore"):
        ts = (b2 - np.sqrt(disc)) / a2
    ball = (disc > 0) & (ts > 0) & (ts < tf) & ~box
    Z = np.where(box, tb, np.where(ball, ts, tf))
    d = Q[2, 3] / (Q[3, 2] * Z)
    d = np.round((d + rng.normal(0.0, sigma, (H, W))) * 16) / 16
    u = rng.random((H, W))
    truth = np.where(box, 1, np.where(ball, 2, 0)).astype(np.int64)
    out = (u >= holes) & (u < holes + outliers)
    d[out] = np.round(rng.uniform(1, 100, int(out.sum())) * 16) / 16
    d[u < holes] = -1.0
    truth[u < holes + outliers] = -1
    info = dict(n=n, P0=P0, es=es, et=et, centre=C, sphere=Cs, box=box, ball=ball)
    return d.astype(F32)[None], truth, info
