"""numpy restatement of the footprint's definition (include/sdr/sdr.h, "the footprint of a
region"): the relief's pixel pipeline (relief_ref.heights), the in-plane basis and cells in float64
with every operation rounded, the grid and the support rule as integer arrays, the 90 directions
from its own table (np.cos / np.sin / np.rint), and the scene of the feature's tests: a rectangular
plate ("box top") ray-cast over a tilted floor."""
import numpy as np

import plane_ref as PR
import relief_ref as LR
import ruler_ref as RR

DTYPE = np.dtype([
    ("side", "<f8", (2,)), ("fill", "<f8"), ("corner", "<f8", (4, 3)), ("basis_s", "<f8", (3,)),
    ("basis_t", "<f8", (3,)), ("i0", "<i8"), ("j0", "<i8"), ("angle_deg", "<i4"), ("span_s", "<i4"),
    ("span_t", "<i4"), ("area", "<i4"), ("n_masked", "<i4"), ("n_valid", "<i4"), ("n", "<i4"),
    ("n_outside", "<i4"), ("n_cells_raw", "<i4"), ("n_cells", "<i4"), ("frame", "<i4"), ("plane", "<i4"),
    ("label", "<i4"), ("flags", "<u4"), ("reserved", "<i4", (4,))])
VALID, OUT_OF_RANGE, NO_PLANE, EMPTY, CLIPPED = 1, 2, 4, 8, 16
F32, F64 = np.float32, np.float64
FLOATS = ("side", "fill", "corner", "basis_s", "basis_t")
H_ALL = (-1048576.0, 1048576.0)

_K = np.arange(90)
DIR_C = np.rint(16384.0 * np.cos(np.radians(_K))).astype(np.int64)
DIR_S = np.rint(16384.0 * np.sin(np.radians(_K))).astype(np.int64)


def basis(normal):
    """(e_s, e_t) float64 (3,) each of a unit normal, or None when one of them is not finite."""
    nx, ny, nz = (F64(v) for v in normal)
    with np.errstate(all="ignore"):
        if np.abs(nx) <= np.abs(ny):
            a, b, c = F64(1.0) - nx * nx, -(nx * ny), -(nx * nz)
        else:
            a, b, c = -(nx * ny), F64(1.0) - ny * ny, -(ny * nz)
        ln = np.sqrt((a * a + b * b) + c * c)
        es = np.array([a / ln, b / ln, c / ln], F64)
        et = np.array([ny * es[2] - nz * es[1], nz * es[0] - nx * es[2], nx * es[1] - ny * es[0]], F64)
    if not (np.isfinite(es).all() and np.isfinite(et).all()):
        return None
    return es, et


def cells(d, conf, lab, Q, plane, es, et, label, xs, ys, xe, ye, cell, h_range, min_disp, conf_min):
    """(masked, valid, member bool (rh, rw), si, ti int64 (rh, rw), meaningful on members)."""
    masked, valid, member, hf = LR.heights(d, conf, lab, Q, plane, label, xs, ys, xe, ye, min_disp, conf_min)
    yy, xx = np.mgrid[ys:ye + 1, xs:xe + 1]
    with np.errstate(all="ignore"):
        xyz = RR.reproject(Q, xx, yy, d[ys:ye + 1, xs:xe + 1].astype(F64))
        X, Y, Z = (xyz[..., i].astype(F64) for i in range(3))
        member = member & (F32(h_range[0]) <= hf) & (hf <= F32(h_range[1]))
        s = (es[0] * X + es[1] * Y) + es[2] * Z
        t = (et[0] * X + et[1] * Y) + et[2] * Z
        qs, qt = s / F64(F32(cell)), t / F64(F32(cell))
        member = member & (np.abs(qs) < F64(2.0 ** 30)) & (np.abs(qt) < F64(2.0 ** 30))
        qs, qt = np.where(member, qs, 0.0), np.where(member, qt, 0.0)
    return masked, valid, member, np.floor(qs).astype(np.int64), np.floor(qt).astype(np.int64)


def kept_cells(count, support):
    """The support rule on an integer grid of counts: the bool grid of kept cells."""
    Gi, Gj = count.shape
    pad = np.zeros((Gi + 2, Gj + 2), np.int64)
    pad[1:-1, 1:-1] = count
    nb = sum(pad[a:a + Gi, b:b + Gj] for a in range(3) for b in range(3))
    return (count >= 1) & (nb >= support)


def rectangle(ii, jj):
    """The minimum-area direction over the kept cells (ii, jj int64): (k, U0, U1, V0, V1)."""
    best = None
    for k in range(90):
        c, s = int(DIR_C[k]), int(DIR_S[k])
        p, r = c * ii + s * jj, c * jj - s * ii
        U0, U1, V0, V1 = int(p.min()), int(p.max()) + c + s, int(r.min()) - s, int(r.max()) + c
        A = (U1 - U0) * (V1 - V0)
        if best is None or A < best[0]:
            best = (A, k, U0, U1, V0, V1)
    return best[1:]


def _canon(v):
    v = np.asarray(v, F64).copy()
    v[np.isnan(v)] = np.nan  # numpy's NaN is the canonical quiet NaN
    return v


def footprint(disp, planes, regions, Q, labels=None, conf=None, cell=4.0, grid=512, support=4, h_range=None,
              min_disp=-1.0, conf_min=0.0):
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
    h_range = H_ALL if h_range is None else h_range
    qs = LR.queries(regions)
    cellf = F64(F32(cell))
    out = np.zeros(len(qs), DTYPE)
    for k, (f, x0, y0, x1, y1, pi, label) in enumerate(qs.tolist()):
        r = out[k]
        for name in FLOATS:
            r[name] = np.nan
        r["frame"], r["plane"], r["label"], r["angle_deg"] = f, pi, label, -1
        if not RR.in_range((f, x0, y0, x1, y1), W, H, F) or not -1 <= label <= 255 or (label >= 0 and labels is None):
            r["flags"] = OUT_OF_RANGE
            continue
        xs, xe, ys, ye = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        r["area"] = (xe - xs + 1) * (ye - ys + 1)
        b = basis(planes[pi]["normal"]) if 0 <= pi < len(planes) and bool(planes[pi]["flags"] & PR.OK) else None
        if b is None:
            r["flags"] = NO_PLANE
            continue
        es, et = b
        masked, valid, member, si, ti = cells(d[f], conf[f] if conf is not None else None,
                                              labels[f] if labels is not None else None, Q, planes[pi], es, et, label,
                                              xs, ys, xe, ye, cell, h_range, min_disp, conf_min)
        r["n_masked"], r["n_valid"], r["n"] = int(masked.sum()), int(valid.sum()), int(member.sum())
        if r["n"] == 0:
            r["flags"] = EMPTY
            continue
        si, ti = si[member], ti[member]
        i0, j0 = int(si.min()), int(ti.min())
        r["i0"], r["j0"] = i0, j0
        r["span_s"] = min(int(si.max()) - i0 + 1, 2 ** 31 - 1)
        r["span_t"] = min(int(ti.max()) - j0 + 1, 2 ** 31 - 1)
        inside = (si - i0 < grid) & (ti - j0 < grid)
        r["n_outside"] = int((~inside).sum())
        clipped = CLIPPED if r["n_outside"] else 0
        # the grid up to the spans: every cell beyond them, inside the grid or not, counts 0
        count = np.zeros((min(grid, int(r["span_s"])), min(grid, int(r["span_t"]))), np.int64)
        np.add.at(count, (si[inside] - i0, ti[inside] - j0), 1)
        keep = kept_cells(count, support)
        r["n_cells_raw"], r["n_cells"] = int((count >= 1).sum()), int(keep.sum())
        if r["n_cells"] == 0:
            r["flags"] = EMPTY | clipped
            continue
        ii, jj = np.nonzero(keep)
        kk, U0, U1, V0, V1 = rectangle(ii.astype(np.int64), jj.astype(np.int64))
        c, s = int(DIR_C[kk]), int(DIR_S[kk])
        n, off = np.asarray(planes[pi]["normal"], F64), F64(planes[pi]["offset"])
        with np.errstate(all="ignore"):
            du, dv = F64(U1 - U0) / F64(16384.0), F64(V1 - V0) / F64(16384.0)
            r["angle_deg"] = kk
            r["side"] = _canon([du * cellf, dv * cellf])
            r["fill"] = _canon(F64(r["n_cells"]) / (du * dv))
            ch, sh = F64(c) / F64(16384.0), F64(s) / F64(16384.0)
            for x, (U, V) in enumerate(((U0, V0), (U1, V0), (U1, V1), (U0, V1))):
                a, bb = F64(U) / F64(16384.0), F64(V) / F64(16384.0)
                gi, gj = ch * a - sh * bb, sh * a + ch * bb
                S, T = (F64(i0) + gi) * cellf, (F64(j0) + gj) * cellf
                r["corner"][x] = _canon((S * es + T * et) - off * n)
        r["basis_s"], r["basis_t"] = es, et
        r["flags"] = VALID | clipped
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_footprints_equal(got, want):
    """Doubles as bit patterns (every NaN the canonical one), integers exactly."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = a != b
        assert not bad.any(), (name, np.argwhere(bad)[:4], got[name][bad][:4], want[name][bad][:4])


# ---- the scene: a rectangular plate over a tilted floor, seen through a window of the reference view
def scene_q(Q):
    """Q of the 320 x 240 window at (480, 250) of the calibration's 1280 x 720 view."""
    Qw = np.array(Q, F64)
    Qw[0, 3] += 480.0
    Qw[1, 3] += 250.0
    return Qw


def box_scene(Q, L=300.0, Wd=200.0, ang=25.0, H=240, W=320, sigma=0.15, holes=0.20, outliers=0.05, seed=3):
    """The floor: normal ~ (0.05, -cos 50, -sin 50) through P0 = (0, 0, 1200) mm.  The box top: an
    L x Wd mm rectangle on the parallel plane 150 mm nearer the camera, centred at
    P0 + 150 n - 20 e_s - 90 e_t and turned by `ang` degrees from e_s towards e_t; only its top
    face is cast (no side faces).  Q is the window's (scene_q).  Disparity Q[2][3] / (Q[3][2] * Z)
    with Gaussian noise on the 1/16 px grid, holes (-1) and uniform outliers in [1, 100).  Returns
    (disp float32 (1, H, W), truth (H, W): 0 floor, 1 box, -1 on holes and outliers, info dict)."""
    rng = np.random.default_rng(seed)
    n = np.array([0.05, -np.cos(np.radians(50.0)), -np.sin(np.radians(50.0))])
    n /= np.linalg.norm(n)
    P0 = np.array([0.0, 0.0, 1200.0])
    es, et = basis(n)
    C = P0 + 150.0 * n - 20.0 * es - 90.0 * et
    ca, sa = np.cos(np.radians(ang)), np.sin(np.radians(ang))
    ax, bx = ca * es + sa * et, -sa * es + ca * et
    f = Q[2, 3]
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.stack([xx + Q[0, 3], yy + Q[1, 3], np.full((H, W), f)], axis=-1) / f  # rays with Z = 1
    tb = np.dot(n, C) / (D @ n)  # the top's plane
    Pb = D * tb[..., None]
    box = (np.abs((Pb - C) @ ax) <= L / 2) & (np.abs((Pb - C) @ bx) <= Wd / 2) & (tb > 0)
    tf = np.dot(n, P0) / (D @ n)
    Z = np.where(box, tb, tf)
    d = Q[2, 3] / (Q[3, 2] * Z)
    d = np.round((d + rng.normal(0.0, sigma, (H, W))) * 16) / 16
    u = rng.random((H, W))
    truth = box.astype(np.int64)
    out = (u >= holes) & (u < holes + outliers)
    d[out] = np.round(rng.uniform(1, 100, int(out.sum())) * 16) / 16
    d[u < holes] = -1.0
    truth[u < holes + outliers] = -1
    info = dict(n=n, P0=P0, es=es, et=et, centre=C, box=box, Ztop=float(tb[box].mean()), f=float(f),
                tilt_cos=float(abs(n[2])))
    return d.astype(F32)[None], truth, info
