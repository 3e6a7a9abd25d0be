"""numpy restatement of the ruler's definition (include/sdr/sdr.h, "the ruler"): the windowed lower
median, the segment walk, cv::norm of the Vec3f difference, the depth profile and the XYZ-map mode.
Plain loops; every float operation is written in the precision the definition names."""
import numpy as np

DTYPE = np.dtype([
    ("p0", "<f4", (3,)), ("p1", "<f4", (3,)), ("d0", "<f4"), ("d1", "<f4"), ("distance", "<f8"),
    ("n0", "<i4"), ("n1", "<i4"), ("path_samples", "<i4"), ("path_valid", "<i4"),
    ("max_gap", "<i4"), ("z_min", "<f4"), ("z_max", "<f4"), ("max_dz", "<f4"), ("flags", "<u4"),
    ("reserved", "<i4")])
P0_VALID, P1_VALID, OUT_OF_RANGE, TRUNCATED = 1, 2, 4, 8
NAN32 = np.float32(np.nan)


def canon(a):
    """Every NaN the ruler computes is the canonical quiet NaN (sdr.h): a computed NaN's sign
    differs between machines (x86 makes it negative)."""
    a = np.asarray(a)
    return np.where(np.isnan(a), a.dtype.type(np.nan), a)


def to_float(disp):
    """float32 as is; int16 as (float)v * 0.0625f."""
    d = np.asarray(disp)
    if d.dtype == np.int16:
        return d.astype(np.float32) * np.float32(0.0625)
    assert d.dtype == np.float32
    return d


def reproject(Q, x, y, d):
    """reprojectImageTo3D's pixel (handleMissing off): float64 row sums from 0 in order, the
    homogeneous coordinates rounded to float32, times 1 / w in float64, rounded to float32.
    x, y, d: scalars or arrays (d float64)."""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    d = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        h = []
        for i in range(4):
            s = np.float64(0.0) + Q[i, 0] * x
            s = s + Q[i, 1] * y
            s = s + Q[i, 2] * d
            s = s + Q[i, 3] * np.float64(1.0)
            h.append(s)
        ia = np.float64(1.0) / h[3]
        out = [(h[i].astype(np.float32).astype(np.float64) * ia).astype(np.float32) for i in range(3)]
    return np.stack(out, axis=-1)


def lower_median(values):
    """Element (n - 1) // 2 of the values in ascending order (ties keep their order: equal values
    such as -0.0 and 0.0 are told apart by position only)."""
    v = np.asarray(values, np.float32)
    order = np.argsort(v, kind="stable")
    return v[order[(len(v) - 1) // 2]]


def valid_mask(win, conf, min_disp, conf_min):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(win) & (win > np.float32(min_disp))
        if conf is not None:
            ok &= conf >= np.float32(conf_min)  # NaN compares false
    return ok


def sample(disp, conf, Q, x, y, r, min_count, min_disp, conf_min):
    """disp float32 (H, W), conf float32 (H, W) or None -> (xyz float32[3], d_med, n, valid)."""
    H, W = disp.shape
    ys, ye = max(y - r, 0), min(y + r, H - 1)
    xs, xe = max(x - r, 0), min(x + r, W - 1)
    win = disp[ys:ye + 1, xs:xe + 1].reshape(-1)
    cw = conf[ys:ye + 1, xs:xe + 1].reshape(-1) if conf is not None else None
    ok = valid_mask(win, cw, min_disp, conf_min)
    n = int(ok.sum())
    if n < min_count:
        return np.full(3, NAN32), NAN32, n, False
    d = lower_median(win[ok])
    xyz = reproject(Q, x, y, np.float64(d))
    return xyz, d, n, bool(np.isfinite(xyz).all())


def rdiv(a, b):
    assert b > 0
    return (2 * a + b) // (2 * b)  # Python's // floors


def walk(x0, y0, x1, y1):
    """The pixels of the segment, P0 first."""
    n = max(abs(x1 - x0), abs(y1 - y0)) + 1
    if n == 1:
        return [(x0, y0)]
    return [(x0 + rdiv(i * (x1 - x0), n - 1), y0 + rdiv(i * (y1 - y0), n - 1)) for i in range(n)]


def distance(p0, p1):
    """cv::norm(Vec3f - Vec3f): the difference in float32, the squares summed in float64."""
    with np.errstate(all="ignore"):
        s = np.float64(0.0)
        for i in range(3):
            df = np.float32(p0[i]) - np.float32(p1[i])
            v = np.float64(df)
            s = s + v * v
        return np.sqrt(s)


def in_range(seg, W, H, F):
    f, x0, y0, x1, y1 = (int(v) for v in seg)
    return 0 <= f < F and 0 <= x0 < W and 0 <= x1 < W and 0 <= y0 < H and 0 <= y1 < H


def out_of_range_record():
    r = np.zeros((), DTYPE)
    for k in ("p0", "p1", "d0", "d1", "distance", "z_min", "z_max", "max_dz"):
        r[k] = np.nan
    r["flags"] = OUT_OF_RANGE
    return r


def measure(disp, segs, Q, conf=None, radius=0, min_count=1, min_disp=-1.0, conf_min=0.0,
            profile=False, profile_cap=0, profile_buf=None):
    """disp (F, H, W) float32 or int16; segs (K, 5).  Returns the records; profile_buf
    (K, profile_cap, 4) float32, when given with profile, is written in place."""
    disp = to_float(disp)
    F, H, W = disp.shape
    segs = np.asarray(segs).reshape(-1, 5)
    out = np.zeros(len(segs), DTYPE)
    for k, seg in enumerate(segs):
        if not in_range(seg, W, H, F):
            out[k] = out_of_range_record()
            continue
        f, x0, y0, x1, y1 = (int(v) for v in seg)
        cf = conf[f] if conf is not None else None
        pts = walk(x0, y0, x1, y1)
        n = len(pts)

        def at(i):
            return sample(disp[f], cf, Q, pts[i][0], pts[i][1], radius, min_count, min_disp, conf_min)

        r = out[k]
        flags = 0
        ends = []
        for e, i in enumerate((0, n - 1)):
            xyz, d, cnt, ok = at(i)
            r["p%d" % e], r["d%d" % e], r["n%d" % e] = canon(xyz), d, cnt
            flags |= (P0_VALID, P1_VALID)[e] if ok else 0
            ends.append((xyz, ok))
        r["distance"] = canon(distance(ends[0][0], ends[1][0])) if ends[0][1] and ends[1][1] else np.nan
        r["z_min"] = r["z_max"] = r["max_dz"] = np.nan
        if profile:
            write = profile_buf is not None
            if write and n > profile_cap:
                flags |= TRUNCATED
            valid = 0
            gap = run = 0
            zmin = zmax = dz = None
            zprev = None
            for i in range(n):
                xyz, d, _, ok = at(i)
                if write and i < profile_cap:
                    profile_buf[k, i] = (xyz[0], xyz[1], xyz[2], d) if ok else (np.nan,) * 4
                if not ok:
                    run += 1
                    gap = max(gap, run)
                    continue
                run = 0
                valid += 1
                z = np.float32(xyz[2])
                zmin = z if zmin is None else min(zmin, z)
                zmax = z if zmax is None else max(zmax, z)
                if zprev is not None:
                    with np.errstate(all="ignore"):
                        step = np.abs(np.float32(z - zprev))
                    dz = step if dz is None else max(dz, step)
                zprev = z
            r["path_samples"], r["path_valid"], r["max_gap"] = n, valid, gap
            if valid >= 1:
                r["z_min"], r["z_max"] = zmin, zmax
            if valid >= 2:
                r["max_dz"] = dz
        r["flags"] = flags
    return out


def measure_xyz(xyz, segs):
    """xyz (F, H, W, 3) float32: the reference's onMouseMeasure."""
    F, H, W, _ = xyz.shape
    segs = np.asarray(segs).reshape(-1, 5)
    out = np.zeros(len(segs), DTYPE)
    for k, seg in enumerate(segs):
        if not in_range(seg, W, H, F):
            out[k] = out_of_range_record()
            continue
        f, x0, y0, x1, y1 = (int(v) for v in seg)
        r = out[k]
        r["p0"], r["p1"] = xyz[f, y0, x0], xyz[f, y1, x1]
        r["d0"] = r["d1"] = r["z_min"] = r["z_max"] = r["max_dz"] = np.nan
        r["n0"] = r["n1"] = 1
        r["distance"] = canon(distance(xyz[f, y0, x0], xyz[f, y1, x1]))
        r["flags"] = (P0_VALID if np.isfinite(xyz[f, y0, x0]).all() else 0) | \
                     (P1_VALID if np.isfinite(xyz[f, y1, x1]).all() else 0)
    return out


def csv_text(image_index, segs, records, header=True):
    """save_csvFile's bytes: setw(4) lands on cv::Point's "[" and on "\\n"."""
    s = "Image, First_point,   Second_point, Distance\n" if header else ""
    for idx, seg, r in zip(image_index, np.asarray(segs).reshape(-1, 5), records):
        s += "%d, [%d, %d],    [%d, %d], %.5f cm   \n" % (idx, seg[1], seg[2], seg[3], seg[4],
                                                          float(r["distance"]) / 10)
    return s


FLOAT_BITS = ("p0", "p1", "d0", "d1")
FLOAT_VALUES = ("z_min", "z_max", "max_dz")
INTS = ("n0", "n1", "path_samples", "path_valid", "max_gap", "flags", "reserved")


def assert_records_equal(got, want):
    """Exact: float fields as bit patterns (NaNs included), distance as a double bit pattern;
    z_min / z_max / max_dz as values with NaN == NaN (the minimum of +0 and -0 is either)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    for k in FLOAT_BITS:
        a, b = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        assert (a == b).all(), (k, np.argwhere(a != b)[:4], got[k][a != b][:4], want[k][a != b][:4],
                                [hex(v) for v in a[a != b][:4]], [hex(v) for v in b[a != b][:4]])
    a, b = np.ascontiguousarray(got["distance"]).view(np.uint64), np.ascontiguousarray(want["distance"]).view(np.uint64)
    bad = a != b
    assert not bad.any(), ("distance", np.argwhere(bad)[:4], got["distance"][bad][:4], want["distance"][bad][:4])
    for k in FLOAT_VALUES:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def assert_profile_equal(got, want):
    """Profile rows as bit patterns."""
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = a != b
    assert not bad.any(), (np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
