"""The clearance of two labelled things without a device: the structures' layout and defaults, every
host guard of the C ABI, the Python surface's argument checks, the restatement
(tests/clearance_ref.py) against plain Python loops, its identities and refusals, and the feature's
scene (the gap between a box top and a hemisphere on a tilted floor) measured with the restatements
only."""
import ctypes

import numpy as np
import pytest

import clearance_ref as CR
import footprint_ref as FR
import objects_ref as OR
import plane_ref as PR
import plane_search_ref as SR
import relief_ref as LR
import ruler_ref as RR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib, pipeline
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import CLEARANCE_DTYPE

Q = S.REFERENCE_Q
EYE = np.eye(4)
F32, F64 = np.float32, np.float64


def test_struct_layout_and_defaults():
    Qy, P, C = _lib.ClearanceQuery, _lib.ClearanceParams, _lib.Clearance
    assert (ctypes.sizeof(Qy), ctypes.sizeof(P), ctypes.sizeof(C)) == (32, 64, 128)
    assert CLEARANCE_DTYPE.itemsize == 128
    assert [(n, getattr(Qy, n).offset) for n, _ in Qy._fields_] == [
        ("frame", 0), ("x0", 4), ("y0", 8), ("x1", 12), ("y1", 16), ("plane", 20), ("label_a", 24), ("label_b", 28)]
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("min_disp", 0), ("conf_min", 4), ("h_lo", 8), ("h_hi", 12), ("radius", 16), ("min_count", 20),
        ("reserved", 24)]
    want = [("distance", 0), ("along", 8), ("across", 16), ("p_a", 24), ("p_b", 36), ("d_a", 48), ("d_b", 52),
            ("xa", 56), ("ya", 60), ("xb", 64), ("yb", 68), ("area", 72), ("n_a", 76), ("n_b", 80), ("m_a", 84),
            ("m_b", 88), ("frame", 92), ("plane", 96), ("label_a", 100), ("label_b", 104), ("flags", 108),
            ("reserved", 112)]
    assert [(n, getattr(C, n).offset) for n, _ in C._fields_] == want
    assert [(n, CLEARANCE_DTYPE.fields[n][1]) for n in CLEARANCE_DTYPE.names] == want
    assert CR.DTYPE == CLEARANCE_DTYPE
    assert (sdr.CLEARANCE_VALID, sdr.CLEARANCE_OUT_OF_RANGE, sdr.CLEARANCE_NO_PLANE, sdr.CLEARANCE_EMPTY) == (1, 2, 4, 8)
    assert (CR.VALID, CR.OUT_OF_RANGE, CR.NO_PLANE, CR.EMPTY) == (1, 2, 4, 8)
    assert _lib.CLEARANCE_MAX_QUERIES == 64 == CR.MAX_QUERIES
    L = _lib.lib()
    assert L.sdr_abi_version() == 4
    p = P(9.0, 9.0, 9.0, 9.0, 9, 9, (ctypes.c_int32 * 10)(*[9] * 10))
    L.sdr_clearance_params_default(ctypes.byref(p))
    assert (p.min_disp, p.conf_min, p.h_lo, p.h_hi, p.radius, p.min_count) == (-1.0, 0.0, -1048576.0, 1048576.0, 0, 1)
    assert list(p.reserved) == [0] * 10
    L.sdr_clearance_params_default(None)
    # the measurement hook: one knob, anything else refused; no device needed
    assert L.sdr_clearance_debug_knob(_lib.DEBUG_CLEARANCE_PRUNE, 0) == 0
    assert L.sdr_clearance_debug_knob(_lib.DEBUG_CLEARANCE_PRUNE, 1) == 0
    assert L.sdr_clearance_debug_knob(0, 1) == -1 and L.sdr_clearance_debug_knob(2, 1) == -1


def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F = 8, 6, 2

    def params(lo=-10.0, hi=10.0, radius=0, mc=1, res=(0,) * 10):
        return _lib.ClearanceParams(-1.0, 0.0, lo, hi, radius, mc, (ctypes.c_int32 * 10)(*res))

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, lab=ptr, q=Qc, par=params(), planes=ptr, P=2, qs=ptr,
            K=1, out=ptr):
        return L.sdr_clearance_device(disp, typ, stride, fs, w, h, f, None, lab, q, ctypes.byref(par) if par else None,
                                      planes, P, qs, K, out, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, lab=ptr, q=Qc, par=params(), planes=ptr, P=2, qs=ptr,
             K=1, out=ptr):
        return L.sdr_clearance(disp, typ, stride, fs, w, h, f, None, lab, q, ctypes.byref(par) if par else None,
                               planes, P, qs, K, out)

    nan = float("nan")
    for fn in (dev, host):
        # what the relief refuses
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(qs=None) == -1 and fn(out=None) == -1 and fn(planes=None) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        assert fn(typ=2) == -1 and fn(typ=-1) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1 and fn(h=8193, fs=W * 8193) == -1
        assert fn(w=8192, stride=8192, h=4096, fs=8192 * 4096) == -1  # 2^25 pixels
        assert fn(P=-1) == -1 and fn(K=-1) == -1
        # the clearance's own
        assert fn(lab=None) == -1 and fn(lab=None, K=0, qs=None, out=None) == -1
        assert fn(K=CR.MAX_QUERIES + 1) == -1 and fn(K=1 << 20) == -1
        assert fn(par=params(lo=nan)) == -1 and fn(par=params(hi=nan)) == -1 and fn(par=params(lo=1.0, hi=0.5)) == -1
        for radius in (-1, 5, 100):
            assert fn(par=params(radius=radius)) == -1, radius
        for mc in (0, -1):
            assert fn(par=params(mc=mc)) == -1, mc
        for i in range(10):
            assert fn(par=params(res=tuple(int(j == i) for j in range(10)))) == -1
        assert L.sdr_last_error()
        # no query: nothing to do, and no device call
        assert fn(K=0, qs=None, out=None) == 0
    # (what passes the guards goes on to the device: the GPU tests)


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    z = np.zeros((4, 4), np.float32)
    lab = np.zeros((4, 4), np.uint8)
    pl = np.zeros(1, sdr.PLANE_DTYPE)
    pair = [(0, 0, 0, 3, 3, 0, 0, 1)]
    with pytest.raises(sdr.SDRError):
        r.clearance(np.zeros((4, 4), np.float64), pl, pair, lab)
    for bad in ([(0, 0, 3, 3)], [(0,) * 7], [(0,) * 9], [(0.5, 0, 0, 3, 3, 0, 0, 1)]):
        with pytest.raises(sdr.SDRError):
            r.clearance(z, pl, bad, lab)
    with pytest.raises(sdr.SDRError):
        r.clearance(z, pl, pair, None)
    with pytest.raises(sdr.SDRError):
        r.clearance(z, pl, pair, lab, conf=np.zeros((3, 4), np.float32))
    with pytest.raises(sdr.SDRError):
        r.clearance(z, pl, pair, np.zeros((4, 4), np.int32))
    with pytest.raises(sdr.SDRError):
        r.clearance(z, pl, pair, np.zeros((3, 4), np.uint8))
    for kw in (dict(h_range=(1.0, 0.0)), dict(h_range=(float("nan"), 1.0))):
        with pytest.raises(sdr.SDRError):
            r.clearance(z, pl, pair, lab, **kw)
    for bad in (sdr.Ruler(Q, radius=5), sdr.Ruler(Q, radius=-1), sdr.Ruler(Q, min_count=0)):
        with pytest.raises(sdr.SDRError):
            bad.clearance(z, pl, pair, lab)
    with pytest.raises(sdr.SDRError):
        r.clearance_device(z, pl, pair, lab)
    with pytest.raises(RuntimeError, match="without ruler="):
        pipeline.LiveLoop.clearance(type("L", (), {"ruler": None})(), None, None, None, None)
    assert sdr.as_clearance_queries([]).shape == (0, 8)
    assert sdr.as_clearance_queries((0, 1, 2, 3, 4, 5, 6, 7)).tolist() == [[0, 1, 2, 3, 4, 5, 6, 7]]


# ---- the restatement ----
def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """With Q the identity and this record, a pixel's point is (x, y, d) and hf is d."""
    p = np.zeros(1, PR.DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def loops(d, lab, plane, Qm, rect, la, lb, radius, min_count, h_range):
    """The definition in plain Python loops on one float32 frame: (n_a, n_b, m_a, m_b, the best
    (s, ip, iq) or None, the sets' points as {index: (xyz, d_med)})."""
    xs, ys, xe, ye = rect
    rw, rh = xe - xs + 1, ye - ys + 1
    n = np.asarray(plane["normal"], F64)
    off = F64(plane["offset"])
    member = {}
    for label in (la, lb):
        m = set()
        for v in range(rh):
            for u in range(rw):
                x, y = xs + u, ys + v
                dd = d[y, x]
                if lab[y, x] != label or not np.isfinite(dd) or not dd > F32(-1.0):
                    continue
                with np.errstate(all="ignore"):
                    xyz = RR.reproject(Qm, x, y, F64(dd))
                    h = ((n[0] * F64(xyz[0]) + n[1] * F64(xyz[1])) + n[2] * F64(xyz[2])) + off
                    hf = F32(h) + F32(0.0)
                if np.isfinite(xyz).all() and abs(hf) < F32(1048576.0) and F32(h_range[0]) <= hf <= F32(h_range[1]):
                    m.add((v, u))
        member[label] = m
    pts = {}
    for label in (la, lb):
        out = {}
        for (v, u) in sorted(member[label]):
            vals = [d[ys + b, xs + a] for b in range(max(v - radius, 0), min(v + radius, rh - 1) + 1)
                    for a in range(max(u - radius, 0), min(u + radius, rw - 1) + 1) if (b, a) in member[label]]
            if len(vals) < min_count:
                continue
            dm = RR.lower_median(vals)
            with np.errstate(all="ignore"):
                xyz = RR.reproject(Qm, xs + u, ys + v, F64(dm))
            if np.isfinite(xyz).all():
                out[v * rw + u] = (xyz, dm)
        pts[label] = out
    best = None
    for ip in sorted(pts[la]):
        for iq in sorted(pts[lb]):
            p, q = pts[la][ip][0], pts[lb][iq][0]
            with np.errstate(all="ignore"):
                v = [F64(F32(q[c]) - F32(p[c])) for c in range(3)]
                s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
            if best is None or s < best[0]:  # ascending (ip, iq): the first of equal s stays
                best = (s, ip, iq)
    return len(member[la]), len(member[lb]), len(pts[la]), len(pts[lb]), best, pts


def random_case(rng, H, W, i16):
    """Coarse disparities (many ties, also among pairs), two labels and a third, holes."""
    d = rng.integers(8, 14, (H, W)).astype(F32) * F32(0.5)
    d[rng.random((H, W)) < 0.2] = -1.0
    lab = rng.choice(np.array([0, 1, 255], np.uint8), (H, W), p=[0.4, 0.4, 0.2])
    return ((d * 16).astype(np.int16) if i16 else d), lab


def test_restatement_against_plain_loops():
    rng = np.random.default_rng(23)
    for trial in range(18):
        H, W = int(rng.integers(3, 21)), int(rng.integers(3, 25))
        i16 = bool(trial % 2)
        disp, lab = random_case(rng, H, W, i16)
        radius, mc = trial % 3, int(rng.integers(1, 4))
        x0, x1 = sorted(rng.integers(0, W, 2).tolist())
        y0, y1 = sorted(rng.integers(0, H, 2).tolist())
        Qm = EYE if trial % 3 else Q
        pl = flat_plane() if trial % 3 else flat_plane(700.0)
        hr = (4.5, 6.5) if trial % 3 == 1 else (-1e5, 1e5)
        got = CR.clearance(disp[None], pl, [(0, x1, y0, x0, y1, 0, 0, 1)], Qm, lab, radius=radius, min_count=mc,
                           h_range=hr)[0]
        na, nb, ma, mb, best, pts = loops(RR.to_float(disp), lab, pl[0], Qm, (x0, y0, x1, y1), 0, 1, radius, mc, hr)
        assert (got["n_a"], got["n_b"], got["m_a"], got["m_b"]) == (na, nb, ma, mb), trial
        assert got["area"] == (x1 - x0 + 1) * (y1 - y0 + 1)
        if best is None:
            assert got["flags"] == CR.EMPTY and got["xa"] == -1 and np.isnan(got["distance"])
            continue
        rw = x1 - x0 + 1
        s, ip, iq = best
        assert got["flags"] == CR.VALID
        assert (got["xa"], got["ya"], got["xb"], got["yb"]) == (x0 + ip % rw, y0 + ip // rw, x0 + iq % rw, y0 + iq // rw)
        assert got["distance"] == np.sqrt(s)
        assert np.array_equal(got["p_a"], pts[0][ip][0]) and np.array_equal(got["p_b"], pts[1][iq][0])
        assert got["d_a"] == pts[0][ip][1] and got["d_b"] == pts[1][iq][1]


def test_identities():
    rng = np.random.default_rng(6)
    for trial in range(8):
        H, W = int(rng.integers(6, 21)), int(rng.integers(6, 25))
        # distinct disparities on a fine grid: no two pairs tie
        d = (rng.permutation(H * W).reshape(H, W).astype(F32) * F32(0.03125) + F32(40.0))
        d[rng.random((H, W)) < 0.15] = -1.0
        lab = rng.integers(0, 2, (H, W)).astype(np.uint8)
        pl = flat_plane(1500.0, (0.0, -0.6, -0.8))
        whole = (0, 0, 0, W - 1, H - 1, 0)
        for radius, mc in ((0, 1), (1, 2)):
            ab = CR.clearance(d[None], pl, [whole + (0, 1)], Q, lab, radius=radius, min_count=mc)[0]
            ba = CR.clearance(d[None], pl, [whole + (1, 0)], Q, lab, radius=radius, min_count=mc)[0]
            assert ab["flags"] == CR.VALID == ba["flags"]
            # swapping the labels swaps the two ends and negates along
            assert ab["distance"] == ba["distance"] and ab["across"] == ba["across"] and ab["along"] == -ba["along"]
            for a, b in (("xa", "xb"), ("ya", "yb"), ("d_a", "d_b"), ("n_a", "n_b"), ("m_a", "m_b")):
                assert ab[a] == ba[b] and ab[b] == ba[a]
            assert np.array_equal(ab["p_a"], ba["p_b"]) and np.array_equal(ab["p_b"], ba["p_a"])
            # distance^2 = along^2 + across^2, to rounding
            assert abs(ab["along"] ** 2 + ab["across"] ** 2 - ab["distance"] ** 2) <= 1e-9 * ab["distance"] ** 2
            if radius == 0:
                # the points are the members' own: the distance is the ruler's between the two pixels
                m = RR.measure(d[None], [(0, ab["xa"], ab["ya"], ab["xb"], ab["yb"])], Q)[0]
                assert np.float64(ab["distance"]).view(np.uint64) == np.float64(m["distance"]).view(np.uint64)
                assert np.array_equal(ab["p_a"], m["p0"]) and np.array_equal(ab["p_b"], m["p1"])
                # and no other pair of members is closer
                rel = LR.heights(d, None, lab, Q, pl[0], 0, 0, 0, W - 1, H - 1)[2]
                assert ab["n_a"] == int(rel.sum()) == ab["m_a"]


def test_refusal_records_of_the_restatement():
    d = np.full((2, 6, 8), 5.0, F32)
    lab = np.zeros((2, 6, 8), np.uint8)
    lab[:, :, 4:] = 1
    pl = np.concatenate([flat_plane(), flat_plane(flags=PR.DEGENERATE)])
    for row, flag, area in (((2, 0, 0, 7, 5, 0, 0, 1), CR.OUT_OF_RANGE, 0), ((0, 0, 0, 8, 5, 0, 0, 1), CR.OUT_OF_RANGE, 0),
                            ((0, 0, -1, 7, 5, 0, 0, 1), CR.OUT_OF_RANGE, 0), ((0, 0, 0, 7, 5, 0, -1, 1), CR.OUT_OF_RANGE, 0),
                            ((0, 0, 0, 7, 5, 0, 0, 256), CR.OUT_OF_RANGE, 0), ((0, 0, 0, 7, 5, 0, 1, 1), CR.OUT_OF_RANGE, 0),
                            ((0, 0, 0, 7, 5, -1, 0, 1), CR.NO_PLANE, 48), ((0, 0, 0, 7, 5, 2, 0, 1), CR.NO_PLANE, 48),
                            ((1, 7, 5, 0, 0, 1, 0, 1), CR.NO_PLANE, 48)):
        r = CR.clearance(d, pl, [row], EYE, lab)[0]
        assert r["flags"] == flag and r["area"] == area
        assert (r["frame"], r["plane"], r["label_a"], r["label_b"]) == (row[0], row[5], row[6], row[7])
        assert all(r[n] == 0 for n in ("n_a", "n_b", "m_a", "m_b")) and all(r[n] == -1 for n in CR.PIXELS)
        assert all(np.isnan(r[n]).all() for n in CR.FLOATS)
    r = CR.clearance(d, pl, [(1, 7, 5, 0, 0, 0, 0, 1)], EYE, lab)[0]
    assert r["flags"] == CR.VALID and (r["n_a"], r["n_b"]) == (24, 24) and r["distance"] == 1.0
    assert (r["xa"], r["ya"], r["xb"], r["yb"]) == (3, 0, 4, 0) and r["along"] == 0.0 and r["across"] == 1.0
    # a label no pixel carries, a band that takes one set away, a min_count no window reaches: EMPTY
    r = CR.clearance(d, pl, [(0, 0, 0, 7, 5, 0, 0, 7)], EYE, lab)[0]
    assert r["flags"] == CR.EMPTY and (r["n_a"], r["n_b"], r["m_a"], r["m_b"]) == (24, 0, 24, 0) and r["xa"] == -1
    r = CR.clearance(d, pl, [(0, 0, 0, 7, 5, 0, 0, 1)], EYE, lab, radius=1, min_count=10)[0]
    assert r["flags"] == CR.EMPTY and (r["n_a"], r["n_b"], r["m_a"], r["m_b"]) == (24, 24, 0, 0)
    r = CR.clearance(d, pl, [(0, 0, 0, 7, 5, 0, 0, 1)], EYE, lab, radius=1, min_count=9)[0]
    assert r["flags"] == CR.VALID and (r["m_a"], r["m_b"]) == (8, 8) and r["distance"] == 3.0  # columns 1-2 and 5-6


# ---- the scene: the box top and the hemisphere of objects_ref.two_object_scene on the found floor ----
def scene():
    Qw = FR.scene_q(Q)
    d, truth, info = OR.two_object_scene(Qw)
    H, W = truth.shape
    planes, count, _, plab = SR.find_planes(d, (0, 0, 0, W - 1, H - 1), Qw, max_planes=3, hypotheses=256,
                                            min_inliers=1000, seed=0)
    floor_i = int(np.argmax([((plab == i) & (truth == 0)).sum() for i in range(count)]))
    objs, scan, lab, _ = OR.find_objects(d, planes, (0, 0, 0, W - 1, H - 1, floor_i, -1), Qw, h_range=(10.0, 1000.0),
                                         max_diff=1.0, connectivity=8, min_pixels=64)
    box_k, ball_k = (int(np.argmax([((lab == k) & (truth == t)).sum() for k in range(scan["count"])])) for t in (1, 2))
    return Qw, d, truth, info, planes, floor_i, lab, box_k, ball_k


def scene_truth(Qw, info, radius=60.0):
    """The noise-free gap: the smallest distance between a pixel's point on the box top and a
    pixel's point on the hemisphere at least 10 mm above the floor, from the scene's geometry in
    double.  Returns (the distance, the two points)."""
    H, W = info["box"].shape
    n, P0, C, Cs = info["n"], info["P0"], info["centre"], info["sphere"]
    f = Qw[2, 3]
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.stack([xx + Qw[0, 3], yy + Qw[1, 3], np.full((H, W), f)], axis=-1) / f  # rays with Z = 1
    Pb = (D * (np.dot(n, C) / (D @ n))[..., None])[info["box"]]
    a2, b2, c2 = (D * D).sum(-1), D @ Cs, float(Cs @ Cs) - radius * radius
    with np.errstate(all="ignore"):
        ts = (b2 - np.sqrt(b2 * b2 - a2 * c2)) / a2
    Ps = (D * ts[..., None])[info["ball"]]
    Ps = Ps[(Ps - P0) @ n >= 10.0]
    dist = np.sqrt(((Pb[:, None, :] - Ps[None, :, :]) ** 2).sum(-1))
    i, j = np.unravel_index(int(np.argmin(dist)), dist.shape)
    return float(dist[i, j]), Pb[i], Ps[j]


def test_gap_between_the_two_objects_on_the_found_floor():
    """Measured here (printed below), truth 122.16 mm (the noise-free minimum over the clean box
    pixels and the clean hemisphere pixels at least 10 mm above the floor): radius 0 / min_count 1
    gives 114.51 mm (error -7.65 mm: the minimum over noisy pixel pairs is biased low), radius 2 /
    min_count 9 gives 120.93 mm (error -1.22 mm) against a bound of 8.16 mm; both ends lie on their true
    objects, (158, 43) on the box and (192, 70) on the hemisphere; 3429 of the box's 3445 members and
    2055 of the hemisphere's 2065 have a point.

    Why 8.16 mm where the issue's estimate says about 7 mm: the form is the issue's,
    2 * (spacing + 3 * sigma_z / sqrt(min_count)), but each end's term is taken at that end's own
    depth from the scene instead of one common Z, and sigma_z grows with Z^2.  The box end lies at
    Z = 1083 mm (spacing Z / f = 1.62 mm, sigma_z = 2.19 mm: a term of 3.80 mm), the hemisphere end
    at Z = 1181 mm (1.76 mm, 2.60 mm: 4.36 mm), 8.16 mm together; the formula at the nearer Z alone
    gives 7.61 mm, at the farther 8.72 mm, and about 7 mm (7.25) needs Z = 1050 mm, nearer
    than either end.  The measured error passes at any of them."""
    Qw, d, truth, info, planes, floor_i, lab, box_k, ball_k = scene()
    H, W = truth.shape
    want, Tb, Ts = scene_truth(Qw, info)
    # the bound from the scene: each end lies within a pixel spacing Z / f and 3 sigma of the sample's
    # depth noise of the true closest point, sigma_z = sigma_d * Z / d reduced by sqrt(min_count);
    # the two ends' terms add up (2 * (spacing + 3 sigma_z / sqrt(min_count)) at one common Z)
    f, sigma_d, mc = Qw[2, 3], 0.15, 9
    bound = 0.0
    for Z in (Tb[2], Ts[2]):
        disp = f / (Qw[3, 2] * Z)
        bound += Z / f + 3.0 * (sigma_d * Z / abs(disp)) / np.sqrt(mc)
    pair = [(0, 0, 0, W - 1, H - 1, floor_i, box_k, ball_k)]
    raw = CR.clearance(d, planes, pair, Qw, lab, radius=0, min_count=1)[0]
    med = CR.clearance(d, planes, pair, Qw, lab, radius=2, min_count=mc)[0]
    print("truth %.2f mm; radius 0 / min_count 1: %.2f mm (error %+.2f); radius 2 / min_count %d: %.2f mm (error %+.2f), "
          "bound %.2f mm; ends (%d, %d) -> (%d, %d); along %.2f across %.2f; points %d of %d and %d of %d"
          % (want, raw["distance"], raw["distance"] - want, mc, med["distance"], med["distance"] - want, bound,
             med["xa"], med["ya"], med["xb"], med["yb"], med["along"], med["across"], med["m_a"], med["n_a"],
             med["m_b"], med["n_b"]))
    assert raw["flags"] == CR.VALID and med["flags"] == CR.VALID
    assert abs(med["distance"] - want) <= bound
    assert truth[med["ya"], med["xa"]] == 1 and truth[med["yb"], med["xb"]] == 2
    assert abs(med["distance"] - want) < abs(raw["distance"] - want)
    # the two parts are the distance's, and the points are the record's own
    assert abs(np.hypot(med["along"], med["across"]) - med["distance"]) < 1e-6
    assert abs(np.linalg.norm(med["p_b"].astype(F64) - med["p_a"].astype(F64)) - med["distance"]) < 1e-3
    assert med["m_a"] <= med["n_a"] and med["m_b"] <= med["n_b"]
