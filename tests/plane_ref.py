"""numpy restatement of the plane fit's definition (include/sdr/sdr.h, "the ruler against a
surface"): exact integer moments as Python ints, the solve, the statistics and the 3-D plane as
np.float64 scalars in the order the definition names, and the point query on top of
ruler_ref.sample.  A pixel's residual is one rounded float64 operation after another, written
elementwise over the region's pixels (a whole-frame fit would otherwise take the suite seconds);
the sums over pixels are integers, so their order does not matter."""
import numpy as np

import ruler_ref as RR

DTYPE = np.dtype([
    ("coef", "<f8", (3,)), ("normal", "<f8", (3,)), ("offset", "<f8"), ("centroid", "<f8", (3,)),
    ("rms_px", "<f8"), ("max_abs_px", "<f4"), ("x0", "<i4"), ("y0", "<i4"), ("frame", "<i4"),
    ("area", "<i4"), ("n_valid", "<i4"), ("n_inliers", "<i4"), ("fits", "<i4"), ("flags", "<u4"),
    ("reserved", "<i4")])
DIST_DTYPE = np.dtype([("p", "<f4", (3,)), ("d", "<f4"), ("distance", "<f8"), ("n", "<i4"), ("flags", "<u4")])
OK, DEGENERATE, NONFINITE, OUT_OF_RANGE = 1, 2, 4, 8
PDIST_VALID, PDIST_OUT_OF_RANGE, PDIST_NO_PLANE = 1, 2, 4
F64 = np.float64


def quantise(disp, conf, min_disp, conf_min):
    """(q int64, valid bool) of a map (H, W): the valid rule and the 1/16 px grid."""
    d = np.asarray(disp)
    with np.errstate(all="ignore"):
        if d.dtype == np.int16:
            f = d.astype(np.float32) * np.float32(0.0625)
            ok = f > np.float32(min_disp)
            q = d.astype(np.int64)
        else:
            assert d.dtype == np.float32
            ok = np.isfinite(d) & (d > np.float32(min_disp)) & (np.abs(d) < np.float32(2048))
            q = np.where(ok, np.rint(np.where(ok, d, 0).astype(np.float64) * 16.0), 0).astype(np.int64)
        if conf is not None:
            ok = ok & (conf >= np.float32(conf_min))
    return q, ok


def moments(u, v, q):
    """int64 arrays u, v, q of a pixel set -> the nine sums as Python ints (exact: the guards on
    the map's size keep every sum below 2^53)."""
    def s(a):
        return int(np.sum(a, dtype=np.int64))
    return [len(u), s(u), s(v), s(q), s(u * u), s(u * v), s(v * v), s(u * q), s(v * q)]


def residuals(fit, u, v, q):
    """r = (double)q - ((a*u + b*v) + c), one rounded float64 operation at a time."""
    a, b, c = fit
    return q.astype(F64) - ((a * u.astype(F64) + b * v.astype(F64)) + c)


def solve(m, min_inliers):
    """(a, b, c) in 1/16 px, or None when the fit is degenerate."""
    with np.errstate(all="ignore"):
        N, su, sv, sq = F64(m[0]), F64(m[1]), F64(m[2]), F64(m[3])
        cuu = N * F64(m[4]) - su * su
        cuv = N * F64(m[5]) - su * sv
        cvv = N * F64(m[6]) - sv * sv
        cuq = N * F64(m[7]) - su * sq
        cvq = N * F64(m[8]) - sv * sq
        det = cuu * cvv - cuv * cuv
        a = (cuq * cvv - cvq * cuv) / det
        b = (cvq * cuu - cuq * cuv) / det
        c = ((sq - a * su) - b * sv) / N
    if m[0] < min_inliers or not det > 0 or not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return None
    return a, b, c


def plane_at(f, u, v):
    return (f[0] * F64(u) + f[1] * F64(v)) + f[2]


def reproject(Q, x, y, d):
    """The four row sums of reprojectImageTo3D at a real-valued pixel, the point in float64."""
    Q = np.asarray(Q, F64).reshape(4, 4)
    with np.errstate(all="ignore"):
        h = []
        for i in range(4):
            s = F64(0.0) + Q[i, 0] * F64(x)
            s = s + Q[i, 1] * F64(y)
            s = s + Q[i, 2] * F64(d)
            s = s + Q[i, 3] * F64(1.0)
            h.append(s)
        return [h[0] / h[3], h[1] / h[3], h[2] / h[3]]


def fit_planes(disp, regions, Q, conf=None, iterations=3, inlier_px=1.0, min_inliers=16, min_disp=-1.0,
               conf_min=0.0):
    """disp (F, H, W) float32 or int16; regions (K, 5) {frame, x0, y0, x1, y1}: the records."""
    disp = np.asarray(disp)
    F, H, W = disp.shape
    regions = np.asarray(regions).reshape(-1, 5)
    out = np.zeros(len(regions), DTYPE)
    T = F64(np.float32(inlier_px)) * F64(16.0)
    cache = {}
    for k, reg in enumerate(regions):
        f, x0, y0, x1, y1 = (int(t) for t in reg)
        r = out[k]
        for name in ("coef", "normal", "offset", "centroid", "rms_px", "max_abs_px"):
            r[name] = np.nan
        r["x0"], r["y0"], r["frame"] = min(x0, x1), min(y0, y1), f
        if not RR.in_range(reg, W, H, F):
            r["flags"] = OUT_OF_RANGE
            continue
        xs, xe, ys, ye = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        r["area"] = (xe - xs + 1) * (ye - ys + 1)
        if f not in cache:
            cache[f] = quantise(disp[f], conf[f] if conf is not None else None, min_disp, conf_min)
        q, ok = cache[f]
        vv, uu = np.nonzero(ok[ys:ye + 1, xs:xe + 1])  # row-major; the sums do not depend on the order
        uu, vv = uu.astype(np.int64), vv.astype(np.int64)
        qq = q[ys:ye + 1, xs:xe + 1][vv, uu]
        r["n_valid"] = len(qq)
        keep, fit, m = np.ones(len(qq), bool), None, None
        for s in range(iterations + 1):
            if s > 0:
                keep = np.abs(residuals(fit, uu, vv, qq)) <= T * F64(2 ** (iterations - s))
            m = moments(uu[keep], vv[keep], qq[keep])
            fit = solve(m, min_inliers)
            if fit is None:
                break
            r["fits"] = s + 1
        if fit is None:
            r["flags"] = DEGENERATE
            continue
        res = residuals(fit, uu, vv, qq)
        inl = res[np.abs(res) <= T]
        r["n_inliers"] = len(inl)
        if len(inl):
            e = np.rint(inl * F64(16.0)).astype(np.int64)
            see = int(np.sum(e * e, dtype=np.int64))
            r["rms_px"] = np.sqrt(F64(see) / F64(len(inl))) / F64(256.0)
            r["max_abs_px"] = np.float32(np.max(np.abs(inl)) / F64(16.0))
        a, b, c = fit
        r["coef"] = (a / F64(16.0), b / F64(16.0), c / F64(16.0))
        with np.errstate(all="ignore"):
            p0 = reproject(Q, xs, ys, plane_at(fit, 0, 0) * F64(0.0625))
            p1 = reproject(Q, xe, ys, plane_at(fit, xe - xs, 0) * F64(0.0625))
            p2 = reproject(Q, xs, ye, plane_at(fit, 0, ye - ys) * F64(0.0625))
            e1 = [p1[i] - p0[i] for i in range(3)]
            e2 = [p2[i] - p0[i] for i in range(3)]
            mx = e1[1] * e2[2] - e1[2] * e2[1]
            my = e1[2] * e2[0] - e1[0] * e2[2]
            mz = e1[0] * e2[1] - e1[1] * e2[0]
            ln = np.sqrt((mx * mx + my * my) + mz * mz)
            n = [mx / ln, my / ln, mz / ln]
            off = -((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])
            if off < 0:
                n, off = [-t for t in n], -off
            N = F64(m[0])
            cu, cv = F64(m[1]) / N, F64(m[2]) / N
            ce = reproject(Q, F64(xs) + cu, F64(ys) + cv, plane_at(fit, cu, cv) * F64(0.0625))
        if np.isfinite(n + [off] + ce).all():
            r["normal"], r["offset"], r["centroid"], r["flags"] = n, off, ce, OK
        else:
            r["flags"] = NONFINITE
    return out


def plane_distance(disp, planes, points, Q, conf=None, radius=0, min_count=1, min_disp=-1.0, conf_min=0.0):
    """points (K, 4) {frame, x, y, plane} against PLANE records: the DIST_DTYPE records."""
    d = RR.to_float(np.asarray(disp))
    F, H, W = d.shape
    points = np.asarray(points).reshape(-1, 4)
    out = np.zeros(len(points), DIST_DTYPE)
    for k, (f, x, y, pi) in enumerate(points.tolist()):
        r = out[k]
        r["p"], r["d"], r["distance"] = np.nan, np.nan, np.nan
        inside = 0 <= f < F and 0 <= x < W and 0 <= y < H
        flags = 0 if inside else PDIST_OUT_OF_RANGE
        plane_ok = 0 <= pi < len(planes) and bool(planes[pi]["flags"] & OK)
        if not plane_ok:
            flags |= PDIST_NO_PLANE
        if inside:
            xyz, dm, n, ok = RR.sample(d[f], conf[f] if conf is not None else None, Q, x, y, radius, min_count,
                                       min_disp, conf_min)
            r["p"], r["d"], r["n"] = RR.canon(xyz), dm, n
            if ok and plane_ok:
                nn, off = planes[pi]["normal"], planes[pi]["offset"]
                with np.errstate(all="ignore"):
                    r["distance"] = RR.canon(((nn[0] * F64(xyz[0]) + nn[1] * F64(xyz[1])) + nn[2] * F64(xyz[2])) + off)
                flags |= PDIST_VALID
        r["flags"] = flags
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_planes_equal(got, want):
    """Doubles and floats as bit patterns, counts and flags exactly."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = a != b
        assert not bad.any(), (name, np.argwhere(bad)[:4], got[name][bad][:4], want[name][bad][:4])


def assert_distances_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in DIST_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = _bits(a), _bits(b)
        bad = a != b
        assert not bad.any(), (name, np.argwhere(bad)[:4], got[name][bad][:4], want[name][bad][:4])
