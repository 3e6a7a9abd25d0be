"""The footprint without a device: the structures' layout and defaults, the direction table, every
host guard of the C ABI, the Python surface's argument checks, identities and refusals of the
restatement, and the feature's scenes (a box top over a tilted floor at three sizes and angles)
measured with the restatements only."""
import ctypes

import numpy as np
import pytest

import footprint_ref as FR
import plane_ref as PR
import plane_search_ref as SR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib, pipeline
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import FOOTPRINT_DTYPE

Q = S.REFERENCE_Q
EYE = np.eye(4)


def test_struct_layout_and_defaults():
    P, R = _lib.FootprintParams, _lib.Footprint
    assert (ctypes.sizeof(P), ctypes.sizeof(R), FOOTPRINT_DTYPE.itemsize) == (64, 256, 256)
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("min_disp", 0), ("conf_min", 4), ("cell", 8), ("h_lo", 12), ("h_hi", 16), ("grid", 20), ("support", 24),
        ("reserved", 28)]
    want = [("side", 0), ("fill", 16), ("corner", 24), ("basis_s", 120), ("basis_t", 144), ("i0", 168), ("j0", 176),
            ("angle_deg", 184), ("span_s", 188), ("span_t", 192), ("area", 196), ("n_masked", 200), ("n_valid", 204),
            ("n", 208), ("n_outside", 212), ("n_cells_raw", 216), ("n_cells", 220), ("frame", 224), ("plane", 228),
            ("label", 232), ("flags", 236), ("reserved", 240)]
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == want
    assert [(n, FOOTPRINT_DTYPE.fields[n][1]) for n in FOOTPRINT_DTYPE.names] == want
    assert FR.DTYPE == FOOTPRINT_DTYPE
    assert (sdr.FOOTPRINT_VALID, sdr.FOOTPRINT_OUT_OF_RANGE, sdr.FOOTPRINT_NO_PLANE, sdr.FOOTPRINT_EMPTY,
            sdr.FOOTPRINT_CLIPPED) == (1, 2, 4, 8, 16)
    assert (FR.VALID, FR.OUT_OF_RANGE, FR.NO_PLANE, FR.EMPTY, FR.CLIPPED) == (1, 2, 4, 8, 16)
    L = _lib.lib()
    assert L.sdr_abi_version() == 4
    p = P(9.0, 9.0, 9.0, 9.0, 9.0, 9, 9, (ctypes.c_int32 * 9)(*[9] * 9))
    L.sdr_footprint_params_default(ctypes.byref(p))
    assert (p.min_disp, p.conf_min, p.cell, p.h_lo, p.h_hi, p.grid, p.support) == (
        -1.0, 0.0, 4.0, -1048576.0, 1048576.0, 512, 4)
    assert list(p.reserved) == [0] * 9
    L.sdr_footprint_params_default(None)


def test_direction_table():
    L = _lib.lib()
    c, s = ctypes.c_int32(), ctypes.c_int32()
    tab = []
    for k in range(90):
        assert L.sdr_footprint_direction(k, ctypes.byref(c), ctypes.byref(s)) == 0
        tab.append((c.value, s.value))
    assert tab == list(zip(FR.DIR_C.tolist(), FR.DIR_S.tolist()))
    assert tab[0] == (16384, 0) and tab[60][0] == 8192 and tab[45][0] == tab[45][1] and tab[30][1] == 8192
    assert all(tab[k] == tab[90 - k][::-1] for k in range(1, 90))
    # unit vectors: the length to about 3e-5, its square to about 6e-5
    err = np.abs((FR.DIR_C ** 2 + FR.DIR_S ** 2) / 2.0 ** 28 - 1.0)
    assert err.max() < 7e-5
    for k in (-1, 90):
        assert L.sdr_footprint_direction(k, ctypes.byref(c), ctypes.byref(s)) == -1
    assert L.sdr_footprint_direction(0, None, ctypes.byref(s)) == -1
    assert L.sdr_footprint_direction(0, ctypes.byref(c), None) == -1


def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F = 8, 6, 2

    def params(cell=4.0, lo=-1048576.0, hi=1048576.0, grid=512, support=4, res=(0,) * 9):
        return _lib.FootprintParams(-1.0, 0.0, cell, lo, hi, grid, support, (ctypes.c_int32 * 9)(*res))

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), planes=ptr, P=2, qs=ptr, K=3,
            out=ptr):
        return L.sdr_plane_footprint_device(disp, typ, stride, fs, w, h, f, None, None, q,
                                            ctypes.byref(par) if par else None, planes, P, qs, K, out, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), planes=ptr, P=2, qs=ptr, K=3,
             out=ptr):
        return L.sdr_plane_footprint(disp, typ, stride, fs, w, h, f, None, None, q,
                                     ctypes.byref(par) if par else None, planes, P, qs, K, out)

    nan, inf = float("nan"), float("inf")
    for fn in (dev, host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(qs=None) == -1 and fn(out=None) == -1 and fn(planes=None) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        assert fn(typ=2) == -1 and fn(typ=-1) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1 and fn(h=8193, fs=W * 8193) == -1
        assert fn(w=8192, stride=8192, h=4096, fs=8192 * 4096) == -1  # 2^25 pixels
        assert fn(K=-1) == -1 and fn(P=-1) == -1
        for cell in (nan, inf, -inf, 0.0, -4.0, 0.0624, 65537.0):
            assert fn(par=params(cell=cell)) == -1, cell
        for grid in (15, 0, -1, 1025):
            assert fn(par=params(grid=grid)) == -1, grid
        for support in (0, -1, 256):
            assert fn(par=params(support=support)) == -1, support
        assert fn(par=params(lo=nan)) == -1 and fn(par=params(hi=nan)) == -1 and fn(par=params(lo=1.0, hi=0.5)) == -1
        for i in range(9):
            assert fn(par=params(res=tuple(int(j == i) for j in range(9)))) == -1
        assert L.sdr_last_error()
        # K == 0 is SDR_OK with no launch, the other arguments passing the guards, the limits included
        assert fn(K=0, qs=None, out=None) == 0
        assert fn(K=0, qs=None, out=None, P=0, planes=None) == 0
        assert fn(K=0, par=params(cell=0.0625, grid=16, support=1, lo=-inf, hi=inf)) == 0
        assert fn(K=0, par=params(cell=65536.0, grid=1024, support=255, lo=3.0, hi=3.0)) == 0


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    z = np.zeros((4, 4), np.float32)
    pl = np.zeros(1, sdr.PLANE_DTYPE)
    reg = [(0, 0, 0, 3, 3, 0, -1)]
    with pytest.raises(sdr.SDRError):
        r.footprint(np.zeros((4, 4), np.float64), pl, reg)
    for bad in ([(0, 0, 3, 3)], [(0,) * 8], [(0.5, 0, 0, 3, 3)]):
        with pytest.raises(sdr.SDRError):
            r.footprint(z, pl, bad)
    with pytest.raises(sdr.SDRError):
        r.footprint(z, pl, reg, conf=np.zeros((3, 4), np.float32))
    with pytest.raises(sdr.SDRError):
        r.footprint(z, pl, reg, labels=np.zeros((4, 4), np.int32))
    with pytest.raises(sdr.SDRError):
        r.footprint(z, pl, reg, labels=np.zeros((3, 4), np.uint8))
    for kw in (dict(cell=0.0), dict(cell=float("nan")), dict(cell=1e6), dict(grid=15), dict(grid=1025),
               dict(grid=32.5), dict(support=0), dict(support=256), dict(support=1.5), dict(h_range=(1.0, 0.0)),
               dict(h_range=(float("nan"), 1.0))):
        with pytest.raises(sdr.SDRError):
            r.footprint(z, pl, reg, **kw)
    with pytest.raises(sdr.SDRError):
        r.footprint_device(z, pl, reg)
    with pytest.raises(RuntimeError, match="without ruler="):
        pipeline.LiveLoop.footprint(type("L", (), {"ruler": None})(), None, None, None)
    rec = np.zeros(2, FOOTPRINT_DTYPE)
    rec["side"] = [(3.0, 5.0), (7.0, 2.0)]
    length, width = sdr.footprint_length_width(rec)
    assert length.tolist() == [5.0, 7.0] and width.tolist() == [3.0, 2.0]


def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """A hand-made record: with Q the identity XYZ is (x, y, d), e_s the X axis, e_t the Y axis:
    s = x, t = y, h = d + offset."""
    p = np.zeros(1, PR.DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def planted(H, W, pts, d=5.0):
    """A (1, H, W) map of holes (-1) with disparity d at the (x, y) of pts."""
    m = np.full((1, H, W), -1.0, np.float32)
    for x, y in pts:
        m[0, y, x] = d
    return m


def rect_pts(x0, y0, x1, y1):
    return [(x, y) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]


def test_basis_of_the_restatement():
    es, et = FR.basis((0.0, 0.0, 1.0))
    assert es.tolist() == [1.0, 0.0, 0.0] and et.tolist() == [0.0, 1.0, 0.0]
    es, et = FR.basis((1.0, 0.0, 0.0))  # |nx| > |ny|: the Y axis
    assert es.tolist() == [0.0, 1.0, 0.0] and et.tolist() == [0.0, 0.0, 1.0]
    rng = np.random.default_rng(2)
    for _ in range(20):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        es, et = FR.basis(n)
        M = np.stack([es, et, n])
        assert np.allclose(M @ M.T, np.eye(3), atol=1e-12) and np.linalg.det(M) > 0.999
    assert FR.basis((np.nan, 0.0, 1.0)) is None and FR.basis((np.inf, 0.0, 0.0)) is None


def test_identities_on_planted_maps():
    pl = flat_plane()
    H, W = 30, 48
    whole = [(0, 0, 0, W - 1, H - 1, 0, -1)]
    kw = dict(cell=1.0, support=1, grid=64)
    # a filled axis-aligned pixel rectangle: angle 0, sides its width and height in pixels, fill 1
    m = planted(H, W, rect_pts(7, 4, 7 + 22, 4 + 12))
    r = FR.footprint(m, pl, whole, EYE, **kw)[0]
    assert r["flags"] == FR.VALID and r["angle_deg"] == 0 and r["side"].tolist() == [23.0, 13.0] and r["fill"] == 1.0
    assert (r["i0"], r["j0"], r["span_s"], r["span_t"]) == (7, 4, 23, 13)
    assert (r["n"], r["n_cells"], r["n_cells_raw"], r["n_outside"]) == (23 * 13, 23 * 13, 23 * 13, 0)
    # the corners are points of the plane Z = 0 (h = d + offset = 0 needs offset = -5) at its corners
    assert r["corner"].tolist() == [[7, 4, 0], [30, 4, 0], [30, 17, 0], [7, 17, 0]]
    r5 = FR.footprint(m, flat_plane(-5.0), whole, EYE, **kw)[0]
    assert r5["corner"].tolist() == [[7, 4, 5], [30, 4, 5], [30, 17, 5], [7, 17, 5]]
    assert r5["basis_s"].tolist() == [1, 0, 0] and r5["basis_t"].tolist() == [0, 1, 0]
    # one member; all members in one cell: a 1 x 1-cell square
    for pts, cell in (([(9, 11)], 1.0), (rect_pts(8, 8, 11, 11), 4.0)):
        r = FR.footprint(planted(H, W, pts), pl, whole, EYE, cell=cell, support=1, grid=16)[0]
        assert r["flags"] == FR.VALID and r["angle_deg"] == 0 and r["side"].tolist() == [cell, cell]
        assert r["n_cells"] == 1 and r["fill"] == 1.0 and r["n"] == len(pts)
    # members on exact cell boundaries, negative s: floor, not truncation (Q moves x by -20)
    Qs = np.eye(4)
    Qs[0, 3] = -20.0
    r = FR.footprint(planted(H, W, [(17, 3), (18, 3), (19, 3), (20, 3), (21, 3)]), pl, whole, Qs, cell=2.0, support=1,
                     grid=16)[0]
    assert (r["i0"], r["j0"], r["span_s"], r["n_cells"]) == (-2, 1, 3, 3)  # s = -3, -2, -1, 0, 1: cells -2, -1, -1, 0, 0
    assert r["side"].tolist() == [6.0, 2.0] and r["corner"][0].tolist() == [-4.0, 2.0, 0.0]
    # grid = 16 on a 40-pixel-wide set: CLIPPED, the members beyond column 16 outside
    m = planted(H, W, rect_pts(2, 5, 41, 8))
    r = FR.footprint(m, pl, whole, EYE, cell=1.0, support=1, grid=16)[0]
    assert r["flags"] == FR.VALID | FR.CLIPPED and r["n_outside"] == 24 * 4 and r["span_s"] == 40
    assert r["side"].tolist() == [16.0, 4.0] and r["n"] == 160
    # support = 9 removes an isolated 2 x 2 block and keeps a filled interior
    m = planted(H, W, rect_pts(2, 2, 3, 3) + rect_pts(10, 10, 19, 17))
    r = FR.footprint(m, pl, whole, EYE, cell=1.0, support=9, grid=32)[0]
    assert r["n_cells_raw"] == 4 + 80 and r["n_cells"] == 8 * 6 and r["side"].tolist() == [8.0, 6.0]
    assert r["corner"][0].tolist() == [11.0, 11.0, 0.0]
    r1 = FR.footprint(m, pl, whole, EYE, cell=1.0, support=1, grid=32)[0]
    assert r1["n_cells"] == 84 and r1["side"][0] * r1["side"][1] > 4 * 48  # the block widens the rectangle
    # h_lo / h_hi exclude by height (h = d): the 9.0 block leaves
    m[0, 2:4, 2:4] = 9.0
    r = FR.footprint(m, pl, whole, EYE, cell=1.0, support=1, grid=32, h_range=(4.0, 6.0))[0]
    assert r["n"] == 80 and r["n_valid"] == 84 and r["side"].tolist() == [10.0, 8.0]
    r = FR.footprint(m, pl, whole, EYE, cell=1.0, support=1, grid=32, h_range=(9.0, 9.0))[0]
    assert r["n"] == 4 and r["side"].tolist() == [2.0, 2.0]
    # a square turned by 45 degrees (a diamond of cells): the search finds 45
    pts = [(24 + a, 15 + b) for a in range(-9, 10) for b in range(-9, 10) if abs(a) + abs(b) <= 9]
    r = FR.footprint(planted(H, W, pts), pl, whole, EYE, cell=1.0, support=1, grid=32)[0]
    assert r["angle_deg"] == 45 and abs(r["side"][0] - r["side"][1]) < 1e-9
    assert abs(r["side"][0] - 20 * 11585 / 16384) < 1e-9


def test_identities_on_random_maps():
    rng = np.random.default_rng(5)
    for trial in range(6):
        H, W = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        d = rng.uniform(20, 90, (1, H, W)).astype(np.float32)
        d[rng.random((1, H, W)) < 0.3] = -1.0
        lab = rng.integers(0, 3, (H, W)).astype(np.uint8)
        for label in (-1, 1):
            r = FR.footprint(d, flat_plane(), [(0, 0, 0, W - 1, H - 1, 0, label)], EYE, labels=lab, cell=1.0,
                             support=1, grid=64)[0]
            mem = (d[0] > -1.0) & ((lab == label) | (label < 0))
            ys, xs = np.nonzero(mem)
            assert r["flags"] == FR.VALID and r["n"] == r["n_cells"] == r["n_cells_raw"] == mem.sum()
            assert (r["i0"], r["j0"]) == (xs.min(), ys.min())
            assert (r["span_s"], r["span_t"]) == (xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
            assert r["side"][0] * r["side"][1] <= r["span_s"] * r["span_t"] * (1 + 1e-4)  # angle 0 is a candidate
            assert 0 < r["fill"] <= 1.0 + 1e-4
            # every member pixel's square lies inside the rectangle
            c, s = FR.DIR_C[r["angle_deg"]] / 16384.0, FR.DIR_S[r["angle_deg"]] / 16384.0
            o = r["corner"][0][:2]
            for gx, gy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                px, py = xs + gx - o[0], ys + gy - o[1]
                u, v = c * px + s * py, -s * px + c * py
                assert u.min() > -1e-3 and u.max() < r["side"][0] + 1e-3
                assert v.min() > -1e-3 and v.max() < r["side"][1] + 1e-3


def test_refusals_of_the_restatement():
    d = np.full((2, 6, 8), 5.0, np.float32)
    pl = np.concatenate([flat_plane(), flat_plane(flags=PR.DEGENERATE), flat_plane(normal=(np.nan, 0, 1))])
    regs = [(2, 0, 0, 7, 5, 0, -1), (0, 0, 0, 8, 5, 0, -1), (0, 0, 0, 7, 5, 0, 3), (0, 0, 0, 7, 5, 0, 256),
            (0, 0, 0, 7, 5, -1, -1), (0, 0, 0, 7, 5, 3, -1), (0, 0, 0, 7, 5, 1, -1), (0, 0, 0, 7, 5, 2, -1),
            (1, 7, 5, 0, 0, 0, -1)]
    r = FR.footprint(d, pl, regs, EYE, min_disp=-3e38, cell=1.0, grid=16, support=1)
    assert r["flags"].tolist() == [FR.OUT_OF_RANGE] * 4 + [FR.NO_PLANE] * 4 + [FR.VALID]
    assert r["area"].tolist() == [0] * 4 + [48] * 5 and r["n"].tolist() == [0] * 8 + [48]
    assert np.isnan(r["side"][:8]).all() and r["side"][8].tolist() == [8.0, 6.0]
    assert r["angle_deg"].tolist() == [-1] * 8 + [0]
    assert r["frame"].tolist() == [q[0] for q in regs] and r["label"].tolist() == [q[6] for q in regs]
    e = FR.footprint(np.full((1, 6, 8), -1.0, np.float32), pl, [(0, 0, 0, 7, 5, 0, -1)], EYE)[0]
    assert e["flags"] == FR.EMPTY and e["n_masked"] == 48 and e["n_valid"] == 0 and np.isnan(e["fill"])
    # members, but no cell with enough support: EMPTY with the counts as found
    e = FR.footprint(planted(6, 8, [(1, 1), (5, 4)]), pl, [(0, 0, 0, 7, 5, 0, -1)], EYE, cell=1.0, support=2,
                     grid=16)[0]
    assert e["flags"] == FR.EMPTY and (e["n"], e["n_cells_raw"], e["n_cells"]) == (2, 2, 0)
    assert (e["i0"], e["j0"], e["span_s"], e["span_t"]) == (1, 1, 5, 4) and np.isnan(e["corner"]).all()


# ---- the scenes: a box top over a tilted floor in a 320 x 240 window of the reference view, 20 %
# holes, 5 % outliers, sigma 0.15 px; searched with max_planes=3, hypotheses=256, min_inliers=1000,
# seed=0; the footprint of the box label on the found floor at cell 4 mm, support 4, grid 512 ----
BOXES = [(300.0, 200.0, 25.0), (250.0, 250.0, 40.0), (320.0, 120.0, 5.0)]
CELL = 4.0


@pytest.mark.parametrize("L,Wd,ang", BOXES)
def test_box_length_and_width_on_the_found_floor(L, Wd, ang):
    """Measured here (printed below), length x width at the angle, fill, against the truth:
    300 x 200 at 25: 310.73 x 212.89 at 25, fill 0.922, bound 21.57 mm (support 1: 503.72 x 436.41 at 4);
    250 x 250 at 40: 262.18 x 261.97 at 40, fill 0.928, bound 21.81 mm (support 1: 498.17 x 449.92 at 1);
    320 x 120 at 5: 328.20 x 130.26 at 5, fill 0.921, bound 20.61 mm (support 1: 503.72 x 436.41 at 4).
    The bound on a side's error is 2 * (cell + p + 3 * sigma): p the larger spacing of neighbouring
    pixels on the box top, Z / f divided by the cosine of the tilt, sigma the in-plane shift of a
    point whose disparity moves by one standard deviation of the noise, dZ = Z^2 * Q32 / Q23 * 0.15
    times the in-plane part of the optical axis, both at the top's farthest depth: a side's two
    ends each lie within a cell, a pixel spacing and three sigma of the true edge."""
    Qw = FR.scene_q(Q)
    d, truth, info = FR.box_scene(Qw, L, Wd, ang)
    H, W = truth.shape
    box = info["box"]
    # conditions, before anything else
    assert not (box[0].any() or box[-1].any() or box[:, 0].any() or box[:, -1].any())
    planes, count, _, labels = SR.find_planes(d, (0, 0, 0, W - 1, H - 1), Qw, max_planes=3, hypotheses=256,
                                              min_inliers=1000, seed=0)
    assert count == 2
    floor_i, box_i = (int(np.argmax([((labels == i) & (truth == s)).sum() for i in range(2)])) for s in (0, 1))
    assert {floor_i, box_i} == {0, 1}
    whole = [(0, 0, 0, W - 1, H - 1, floor_i, box_i)]
    r = FR.footprint(d, planes, whole, Qw, labels=labels, cell=CELL, grid=512, support=4)[0]
    r1 = FR.footprint(d, planes, whole, Qw, labels=labels, cell=CELL, grid=512, support=1)[0]
    assert r["flags"] == FR.VALID and r["n_outside"] == 0 and r1["n_outside"] == 0

    Zfar = float(_top_depth(info, Qw, H, W)[box].max())  # the top's farthest depth
    p = (Zfar / info["f"]) / info["tilt_cos"]
    sigma = (Zfar * Zfar * Qw[3, 2] / Qw[2, 3] * 0.15) * np.sqrt(1.0 - info["tilt_cos"] ** 2)
    bound = 2.0 * (CELL + p + 3.0 * sigma)

    def errors(rec):
        k = int(rec["angle_deg"])
        # side[0] lies along angle k; the box's L side along ang (mod 180): pair the sides by the angle
        dk = (k - ang) % 180.0
        along = min(dk, 180.0 - dk) <= 45.0
        s0, s1 = (L, Wd) if along else (Wd, L)
        da = (k - ang) % 90.0
        return abs(rec["side"][0] - s0), abs(rec["side"][1] - s1), min(da, 90.0 - da)

    e0, e1, ea = errors(r)
    f0, f1, fa = errors(r1)
    print("box %.0f x %.0f at %.0f: %.2f x %.2f at %d, fill %.3f, cells %d of %d raw, errors %.2f %.2f mm, bound %.2f mm "
          "(p %.2f sigma %.2f); support 1: %.2f x %.2f at %d, fill %.3f"
          % (L, Wd, ang, max(r["side"]), min(r["side"]), r["angle_deg"], r["fill"], r["n_cells"], r["n_cells_raw"],
             e0, e1, bound, p, sigma, max(r1["side"]), min(r1["side"]), r1["angle_deg"], r1["fill"]))
    assert e0 <= bound and e1 <= bound
    assert ea <= 2.0
    assert r["fill"] > 0.8
    # the reason the support rule exists: the stray labelled pixels break support 1
    assert max(f0, f1) > bound


def _top_depth(info, Qw, H, W):
    """Z of the box top's plane along each pixel's ray."""
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.stack([xx + Qw[0, 3], yy + Qw[1, 3], np.full((H, W), info["f"])], axis=-1) / info["f"]
    return np.dot(info["n"], info["centre"]) / (D @ info["n"])
