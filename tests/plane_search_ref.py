"""numpy restatement of the plane search's definition (include/sdr/sdr.h, "the dominant planes of
a region"), on plane_ref's quantise / moments / solve / residuals / reproject.  The draws, the
hypotheses, the scores and the pick are integers (uint32 / int64 arrays whose bounds sdr.h states);
the refits and the record are plane_ref's float64 steps in the definition's order.  Besides
find_planes it exposes a round's hypothesis table and score vector (`trace`), so that tests can
choose their inputs by condition."""
import numpy as np

import plane_ref as PR
import ruler_ref as RR

ROUND_DTYPE = np.dtype([("hypothesis", "<i4"), ("score", "<i4"), ("voids", "<i4"), ("stop", "<u4")])
RAN, NO_HYPOTHESIS, LOW_SCORE, REFIT_DEGENERATE, FEW_INLIERS, NOT_RUN = range(6)
F64 = np.float64


def mix(x):
    """The definition's mix() on uint32 (scalars or arrays)."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def hypothesis_table(q, free, r, M, seed):
    """q, free: (rh, rw) of the region.  Returns dict(A, B, C, D int64 (M,), void bool (M,),
    pts int64 (M, 3, 3) {u, v, q}); a void hypothesis has A = B = C = D = 0."""
    rh, rw = free.shape
    area = rh * rw
    h = np.arange(M, dtype=np.uint64)
    key = mix(mix(np.uint64((seed ^ ((0x9E3779B9 * (r + 1)) & 0xFFFFFFFF)) & 0xFFFFFFFF)) ^ h)
    pts = np.zeros((M, 3, 3), np.int64)
    found = np.ones(M, bool)
    for j in range(3):
        got = np.zeros(M, bool)
        for t in range(16):
            x = mix(key ^ np.uint64(16 * j + t))
            p = ((x * np.uint64(area)) >> np.uint64(32)).astype(np.int64)
            v, u = p // rw, p % rw
            take = ~got & free[v, u]
            pts[take, j, 0], pts[take, j, 1], pts[take, j, 2] = u[take], v[take], q[v[take], u[take]]
            got |= take
        found &= got
    d1, d2 = pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0]
    A = d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1]
    B = d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2]
    C = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    void = ~found | (C == 0)
    A, B, C = (np.where(void, 0, t) for t in (A, B, C))
    D = A * pts[:, 0, 0] + B * pts[:, 0, 1] + C * pts[:, 0, 2]
    return dict(A=A, B=B, C=C, D=D, void=void, pts=pts)


def integer_residuals(tab, h, u, v, q):
    """A*u + B*v + C*q - D of hypothesis h at int64 pixel arrays."""
    return tab["A"][h] * u + tab["B"][h] * v + tab["C"][h] * q - tab["D"][h]


def score_vector(tab, u, v, q, Tq):
    """Scores of the table's hypotheses over the free pixels (u, v, q int64 arrays); void: 0."""
    M = len(tab["A"])
    out = np.zeros(M, np.int64)
    live = np.nonzero(~tab["void"])[0]
    step = max(1, (1 << 22) // max(len(u), 1))
    for i in range(0, len(live), step):
        hh = live[i:i + step]
        e = (tab["A"][hh, None] * u[None] + tab["B"][hh, None] * v[None] + tab["C"][hh, None] * q[None]
             - tab["D"][hh, None])
        out[hh] = (np.abs(e) <= Tq * np.abs(tab["C"][hh, None])).sum(axis=1)
    return out


def pick(tab, scores):
    """(winner or -1, its score, voids)."""
    voids = int(tab["void"].sum())
    if voids == len(scores):
        return -1, 0, voids
    s = np.where(tab["void"], -1, scores)
    h = int(np.argmax(s))  # the first of the maxima: the lowest index
    return h, int(s[h]), voids


def _empty_record(r, reg, area, flags):
    f, x0, y0, x1, y1 = (int(t) for t in reg)
    for name in ("coef", "normal", "offset", "centroid", "rms_px", "max_abs_px"):
        r[name] = np.nan
    r["x0"], r["y0"], r["frame"], r["area"], r["flags"] = min(x0, x1), min(y0, y1), f, area, flags


def _fill_record(r, Q, xs, ys, xe, ye, fit, m, res_inl):
    """plane_ref.fit_planes' statistics, coefficients and 3-D plane for one record."""
    r["n_inliers"] = len(res_inl)
    if len(res_inl):
        e = np.rint(res_inl * F64(16.0)).astype(np.int64)
        see = int(np.sum(e * e, dtype=np.int64))
        r["rms_px"] = np.sqrt(F64(see) / F64(len(res_inl))) / F64(256.0)
        r["max_abs_px"] = np.float32(np.max(np.abs(res_inl)) / F64(16.0))
    a, b, c = fit
    r["coef"] = (a / F64(16.0), b / F64(16.0), c / F64(16.0))
    with np.errstate(all="ignore"):
        p0 = PR.reproject(Q, xs, ys, PR.plane_at(fit, 0, 0) * F64(0.0625))
        p1 = PR.reproject(Q, xe, ys, PR.plane_at(fit, xe - xs, 0) * F64(0.0625))
        p2 = PR.reproject(Q, xs, ye, PR.plane_at(fit, 0, ye - ys) * F64(0.0625))
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
        ce = PR.reproject(Q, F64(xs) + cu, F64(ys) + cv, PR.plane_at(fit, cu, cv) * F64(0.0625))
    if np.isfinite(n + [off] + ce).all():
        r["normal"], r["offset"], r["centroid"], r["flags"] = n, off, ce, PR.OK
    else:
        r["flags"] = PR.NONFINITE


def find_planes(disp, region, Q, conf=None, max_planes=4, hypotheses=256, seed=0, iterations=3, inlier_px=1.0,
                min_inliers=64, min_disp=-1.0, conf_min=0.0, trace=None):
    """disp (F, H, W) float32 or int16, region {frame, x0, y0, x1, y1}.  Returns (planes DTYPE
    (max_planes,), count, rounds ROUND_DTYPE (max_planes,), labels uint8 (H, W)).  trace: a list
    that receives a dict(table, scores, winner, u, v, q) a round that reached its pick."""
    disp = np.asarray(disp)
    F, H, W = disp.shape
    reg = np.asarray(region).reshape(5)
    planes = np.zeros(max_planes, PR.DTYPE)
    rounds = np.zeros(max_planes, ROUND_DTYPE)
    rounds["hypothesis"], rounds["stop"] = -1, NOT_RUN
    labels = np.full((H, W), 255, np.uint8)
    f, x0, y0, x1, y1 = (int(t) for t in reg)
    if not RR.in_range(reg, W, H, F):
        for r in planes:
            _empty_record(r, reg, 0, PR.OUT_OF_RANGE)
        return planes, 0, rounds, labels
    xs, xe, ys, ye = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    area = (xe - xs + 1) * (ye - ys + 1)
    q, ok = PR.quantise(disp[f], conf[f] if conf is not None else None, min_disp, conf_min)
    q, free = q[ys:ye + 1, xs:xe + 1], ok[ys:ye + 1, xs:xe + 1].copy()
    lab = labels[ys:ye + 1, xs:xe + 1]
    T = F64(np.float32(inlier_px)) * F64(16.0)
    Tq = int(np.floor(T))
    M = hypotheses

    def stop(r, h, score, voids, code):
        for rec in planes[r:]:
            _empty_record(rec, reg, area, PR.DEGENERATE)
        rounds[r] = (h, score, voids, code)
        return planes, r, rounds, labels

    for r in range(max_planes):
        tab = hypothesis_table(q, free, r, M, seed)
        vv, uu = np.nonzero(free)
        uu, vv = uu.astype(np.int64), vv.astype(np.int64)
        qq = q[vv, uu]
        scores = score_vector(tab, uu, vv, qq, Tq)
        h, score, voids = pick(tab, scores)
        if trace is not None:
            trace.append(dict(table=tab, scores=scores, winner=h, u=uu, v=vv, q=qq))
        if h < 0:
            return stop(r, -1, 0, voids, NO_HYPOTHESIS)
        if score < min_inliers:
            return stop(r, h, score, voids, LOW_SCORE)
        A, B, C, D = (int(tab[k][h]) for k in "ABCD")
        fit = (-F64(A) / F64(C), -F64(B) / F64(C), F64(D) / F64(C))
        m = None
        for k in range(1, iterations + 1):
            keep = np.abs(PR.residuals(fit, uu, vv, qq)) <= T * F64(2 ** (iterations - k))
            m = PR.moments(uu[keep], vv[keep], qq[keep])
            fit = PR.solve(m, min_inliers)
            if fit is None:
                return stop(r, h, score, voids, REFIT_DEGENERATE)
        res = PR.residuals(fit, uu, vv, qq)
        inl = np.abs(res) <= T
        if int(inl.sum()) < min_inliers:
            return stop(r, h, score, voids, FEW_INLIERS)
        rec = planes[r]
        _empty_record(rec, reg, area, 0)
        rec["n_valid"], rec["fits"] = len(qq), iterations + 1
        _fill_record(rec, Q, xs, ys, xe, ye, fit, m, res[inl])
        lab[vv[inl], uu[inl]] = r
        free[vv[inl], uu[inl]] = False
        rounds[r] = (h, score, voids, RAN)
    return planes, max_planes, rounds, labels


def three_surface_scene(H=240, W=320, seed=11, sigma=0.15, outliers=0.05, holes=0.20, dtype=np.float32):
    """The issue's scene, scaled to (H, W) from its 240 x 320 layout: floor d = 20 + 0.02x + 0.10y
    for y >= 110/240 H; box d = 55 + 0.01x - 0.02y on x in [90, 250)/320 W, y in [60, 190)/240 H;
    wall d = 12 - 0.03x elsewhere (the box lies over both); noise on the 1/16 grid, uniform
    outliers in [1, 100), holes (-1).  Returns (disp (1, H, W), truth (H, W) in {0 floor, 1 box,
    2 wall}, -1 on holes and outliers, the three (a, b, c))."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    coefs = [(0.02, 0.10, 20.0), (0.01, -0.02, 55.0), (-0.03, 0.0, 12.0)]
    surf = np.full((H, W), 2)
    surf[ys >= (110 * H) // 240] = 0
    bx0, bx1, by0, by1 = (90 * W) // 320, (250 * W) // 320, (60 * H) // 240, (190 * H) // 240
    surf[by0:by1, bx0:bx1] = 1
    d = np.zeros((H, W))
    for i, (a, b, c) in enumerate(coefs):
        d = np.where(surf == i, c + a * xs + b * ys, d)
    d = np.round((d + rng.normal(0.0, sigma, (H, W))) * 16) / 16
    u = rng.random((H, W))
    truth = surf.copy()
    out = (u >= holes) & (u < holes + outliers)
    d[out] = np.round(rng.uniform(1, 100, int(out.sum())) * 16) / 16
    d[u < holes] = -1.0
    truth[u < holes + outliers] = -1
    if dtype == np.int16:
        return np.where(u < holes, -16, np.rint(d * 16)).astype(np.int16)[None], truth, coefs
    return d.astype(np.float32)[None], truth, coefs


def rounds_table(r):
    """Rounds as an int64 (n, 4) table {hypothesis, score, voids, stop}, from ROUND_DTYPE records or
    from the device's int32 (n, 4) tensor."""
    r = np.asarray(r)
    if r.dtype.names:
        return np.stack([r[n].astype(np.int64) for n in ROUND_DTYPE.names], axis=1)
    return r.reshape(-1, 4).astype(np.int64)


def assert_rounds_equal(got, want):
    got, want = rounds_table(got), rounds_table(want)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
