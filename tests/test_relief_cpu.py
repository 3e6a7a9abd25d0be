"""The relief without a device: the structures' layout and defaults, every host guard of the C ABI,
the Python surface's argument checks, identities of the restatement on random maps, and the issue's
scene (a slanted box on a floor in front of a wall) measured with the restatements only."""
import ctypes

import numpy as np
import pytest

import plane_ref as PR
import plane_search_ref as SR
import relief_ref as LR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib, pipeline
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import RELIEF_DTYPE, as_relief_queries

Q = S.REFERENCE_Q


def test_struct_layout_and_defaults():
    Qy, P, R = _lib.ReliefQuery, _lib.ReliefParams, _lib.Relief
    assert (ctypes.sizeof(Qy), ctypes.sizeof(P), ctypes.sizeof(R), RELIEF_DTYPE.itemsize) == (32, 64, 128, 128)
    assert [(n, getattr(Qy, n).offset) for n, _ in Qy._fields_] == [
        ("frame", 0), ("x0", 4), ("y0", 8), ("x1", 12), ("y1", 16), ("plane", 20), ("label", 24), ("reserved", 28)]
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("min_disp", 0), ("conf_min", 4), ("band", 8), ("nq", 12), ("permille", 16), ("reserved", 48)]
    want = [("q", 0), ("h_min", 32), ("h_max", 36), ("mean", 40), ("mean_above", 48), ("sum256", 56),
            ("sum256_above", 64), ("area", 72), ("n_masked", 76), ("n_valid", 80), ("n", 84), ("n_above", 88),
            ("n_below", 92), ("n_rejected", 96), ("frame", 100), ("plane", 104), ("label", 108), ("flags", 112),
            ("reserved", 116)]
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == want
    assert [(n, RELIEF_DTYPE.fields[n][1]) for n in RELIEF_DTYPE.names] == want
    assert LR.DTYPE == RELIEF_DTYPE
    assert (sdr.RELIEF_VALID, sdr.RELIEF_OUT_OF_RANGE, sdr.RELIEF_NO_PLANE, sdr.RELIEF_EMPTY) == (1, 2, 4, 8)
    assert (LR.VALID, LR.OUT_OF_RANGE, LR.NO_PLANE, LR.EMPTY) == (1, 2, 4, 8)
    L = _lib.lib()
    assert L.sdr_abi_version() == 4
    p = P(9.0, 9.0, 9.0, 9, (ctypes.c_int32 * 8)(*[9] * 8), (ctypes.c_int32 * 4)(*[9] * 4))
    L.sdr_relief_params_default(ctypes.byref(p))
    assert (p.min_disp, p.conf_min, p.band, p.nq) == (-1.0, 0.0, 0.0, 3)
    assert list(p.permille) == [50, 500, 950, 0, 0, 0, 0, 0] and list(p.reserved) == [0] * 4
    L.sdr_relief_params_default(None)


def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F = 8, 6, 2

    def params(band=0.0, nq=3, pm=(50, 500, 950), res=(0, 0, 0, 0)):
        pm = tuple(pm) + (0,) * (8 - len(pm))
        return _lib.ReliefParams(-1.0, 0.0, band, nq, (ctypes.c_int32 * 8)(*pm), (ctypes.c_int32 * 4)(*res))

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), planes=ptr, P=2, qs=ptr, K=3,
            out=ptr):
        return L.sdr_plane_relief_device(disp, typ, stride, fs, w, h, f, None, None, q,
                                         ctypes.byref(par) if par else None, planes, P, qs, K, out, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), planes=ptr, P=2, qs=ptr, K=3,
             out=ptr):
        return L.sdr_plane_relief(disp, typ, stride, fs, w, h, f, None, None, q, ctypes.byref(par) if par else None,
                                  planes, P, qs, K, out)

    for fn in (dev, host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(qs=None) == -1 and fn(out=None) == -1 and fn(planes=None) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        assert fn(typ=2) == -1 and fn(typ=-1) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1 and fn(h=8193, fs=W * 8193) == -1
        assert fn(w=8192, stride=8192, h=4096, fs=8192 * 4096) == -1  # 2^25 pixels
        assert fn(K=-1) == -1 and fn(P=-1) == -1
        assert fn(par=params(nq=-1)) == -1 and fn(par=params(nq=9)) == -1
        assert fn(par=params(pm=(50, 1001, 950))) == -1 and fn(par=params(pm=(-1, 500, 950))) == -1
        assert fn(par=params(nq=8, pm=(0, 1, 2, 3, 4, 5, 6, 1001))) == -1
        for band in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert fn(par=params(band=band)) == -1, band
        for i in range(4):
            assert fn(par=params(res=tuple(int(j == i) for j in range(4)))) == -1
        assert L.sdr_last_error()
        # K == 0 is SDR_OK with no launch, the other arguments passing the guards; an entry past nq
        # is ignored
        assert fn(K=0, qs=None, out=None) == 0
        assert fn(K=0, qs=None, out=None, P=0, planes=None) == 0
        assert fn(K=0, par=params(nq=2, pm=(50, 500, 5000))) == 0
        assert fn(K=0, par=params(nq=0, pm=(-7,))) == 0


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    z = np.zeros((4, 4), np.float32)
    pl = np.zeros(1, sdr.PLANE_DTYPE)
    reg = [(0, 0, 0, 3, 3, 0, -1)]
    with pytest.raises(sdr.SDRError):
        r.relief(np.zeros((4, 4), np.float64), pl, reg)
    for bad in ([(0, 0, 3, 3)], [(0,) * 8], [(0.5, 0, 0, 3, 3)]):
        with pytest.raises(sdr.SDRError):
            r.relief(z, pl, bad)
    with pytest.raises(sdr.SDRError):
        r.relief(z, pl, reg, conf=np.zeros((3, 4), np.float32))
    with pytest.raises(sdr.SDRError):
        r.relief(z, pl, reg, labels=np.zeros((4, 4), np.int32))
    with pytest.raises(sdr.SDRError):
        r.relief(z, pl, reg, labels=np.zeros((3, 4), np.uint8))
    for kw in (dict(quantiles=range(9)), dict(quantiles=(1001,)), dict(quantiles=(-1,)), dict(quantiles=(0.5,)),
               dict(band=-1.0), dict(band=float("nan")), dict(band=float("inf"))):
        with pytest.raises(sdr.SDRError):
            r.relief(z, pl, reg, **kw)
    with pytest.raises(sdr.SDRError):
        r.relief_device(z, pl, reg)
    with pytest.raises(RuntimeError, match="without ruler="):
        pipeline.LiveLoop.relief(type("L", (), {"ruler": None})(), None, None, None)
    assert as_relief_queries([]).shape == (0, 8)
    assert as_relief_queries((1, 2, 3, 4, 5)).tolist() == [[1, 2, 3, 4, 5, 0, -1, 0]]
    assert as_relief_queries([(1, 2, 3, 4, 5, 6)]).tolist() == [[1, 2, 3, 4, 5, 6, -1, 0]]
    assert as_relief_queries([(1, 2, 3, 4, 5, 6, 7)]).tolist() == [[1, 2, 3, 4, 5, 6, 7, 0]]
    assert LR.queries([(1, 2, 3, 4, 5)]).tolist() == [[1, 2, 3, 4, 5, 0, -1]]


def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """A hand-made record: with Q the identity, h is Z + offset = the disparity + offset."""
    p = np.zeros(1, PR.DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def test_identities_on_random_maps():
    rng = np.random.default_rng(5)
    for trial in range(6):
        H, W = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        d = rng.uniform(20, 90, (1, H, W)).astype(np.float32)
        d[rng.random((1, H, W)) < 0.2] = -1.0
        d[rng.random((1, H, W)) < 0.05] = np.nan
        lab = rng.integers(0, 3, (H, W)).astype(np.uint8)
        conf = rng.random((1, H, W)).astype(np.float32)
        planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1)], Q, iterations=0, min_inliers=3)
        assert planes["flags"][0] == PR.OK
        band = float(rng.uniform(0, 30))
        for label in (-1, 1):
            r = LR.relief(d, planes, [(0, 0, 0, W - 1, H - 1, 0, label)], Q, labels=lab, conf=conf,
                          quantiles=(0, 1000, 500), band=band, conf_min=0.3)[0]
            assert r["flags"] == LR.VALID and r["area"] == H * W
            m, v, mem, hf = LR.heights(d[0], conf[0], lab, Q, planes[0], label, 0, 0, W - 1, H - 1, conf_min=0.3)
            s = np.sort(hf[mem])
            assert r["q"][0] == r["h_min"] == s[0] and r["q"][1] == r["h_max"] == s[-1]
            assert r["q"][2] == s[(r["n"] - 1) // 2] and np.isnan(r["q"][3:]).all()
            assert r["n_above"] + r["n_below"] <= r["n"] == len(s)
            assert r["n_rejected"] == r["n_valid"] - r["n"] and r["n_valid"] <= r["n_masked"] <= r["area"]
            assert r["n_masked"] == (H * W if label < 0 else int((lab == 1).sum()))
            assert r["h_min"] <= r["mean"] <= r["h_max"]
            assert r["sum256"] == int(np.rint(s.astype(np.float64) * 256).astype(np.int64).sum())


def test_refusals_of_the_restatement():
    d = np.full((2, 6, 8), 5.0, np.float32)
    I = np.eye(4)
    pl = np.concatenate([flat_plane(), flat_plane(flags=PR.DEGENERATE)])
    regs = [(2, 0, 0, 7, 5, 0, -1), (0, 0, 0, 8, 5, 0, -1), (0, 0, 0, 7, 5, 0, 3), (0, 0, 0, 7, 5, 0, 256),
            (0, 0, 0, 7, 5, -1, -1), (0, 0, 0, 7, 5, 2, -1), (0, 0, 0, 7, 5, 1, -1), (1, 7, 5, 0, 0, 0, -1)]
    r = LR.relief(d, pl, regs, I, min_disp=-3e38)
    assert r["flags"].tolist() == [LR.OUT_OF_RANGE] * 4 + [LR.NO_PLANE] * 3 + [LR.VALID]
    assert r["area"].tolist() == [0] * 4 + [48] * 4 and r["n"].tolist() == [0] * 7 + [48]
    assert np.isnan(r["mean"][:7]).all() and r["mean"][7] == 5.0 and (r["q"][7][:3] == 5.0).all()
    assert r["frame"].tolist() == [q[0] for q in regs] and r["label"].tolist() == [q[6] for q in regs]
    e = LR.relief(np.full((1, 6, 8), -1.0, np.float32), pl, [(0, 0, 0, 7, 5, 0, -1)], I)[0]
    assert e["flags"] == LR.EMPTY and e["n_masked"] == 48 and e["n_valid"] == 0 and np.isnan(e["h_min"])


# ---- the scene of the issue: a slanted box on a floor in front of a wall, 320 x 240, 20 % holes,
# 5 % outliers; searched with max_planes=4, min_inliers=1000, seed=0 ----
def plane_from_coef(coef, W, H):
    """The 3-D plane of d = a*x + b*y + c by the plane fit's construction (its three anchors)."""
    a, b, c = coef
    F64 = np.float64
    p0 = PR.reproject(Q, 0, 0, F64(c))
    p1 = PR.reproject(Q, W - 1, 0, F64(a * (W - 1) + c))
    p2 = PR.reproject(Q, 0, H - 1, F64(b * (H - 1) + c))
    n = np.cross(np.subtract(p1, p0), np.subtract(p2, p0))
    n = n / np.linalg.norm(n)
    off = -float(np.dot(n, p0))
    if off < 0:
        n, off = -n, -off
    return flat_plane(off, n)


@pytest.fixture(scope="module")
def scene():
    d, truth, coefs = SR.three_surface_scene()
    H, W = truth.shape
    planes, count, _, labels = SR.find_planes(d, (0, 0, 0, W - 1, H - 1), Q, max_planes=4, hypotheses=256,
                                              min_inliers=1000, seed=0)
    assert count == 3
    idx = [int(np.argmax([((labels == i) & (truth == s)).sum() for i in range(3)])) for s in range(3)]
    return d, truth, coefs, planes, labels, idx[0], idx[1]  # floor, box


def test_box_height_above_the_found_floor(scene):
    """Measured here (printed below): the box label against the found floor, n 15789, heights 71.3 ..
    491.4 mm, quantiles 5 / 50 / 95 % 178.5 / 283.989 / 385.1 mm; the same median on the noise-free
    scene with the true coefficients and the true mask 284.033 mm: error 0.043 mm.  400 single-pixel
    lookups in the box rectangle: 79 not finite, median |error| 1.09 mm, largest 2676 mm.  The
    rectangle's mean without the mask 228.1 mm (its median 283.31 mm), the label's 283.07 mm: 55 mm
    apart, against a tenth of the 5-95 % spread, 20.7 mm."""
    d, truth, coefs, planes, labels, floor, box = scene
    H, W = truth.shape
    ys, xs = np.nonzero(truth == 1)
    # the box rectangle of the scene's layout (truth is -1 on its holes and outliers)
    x0, x1, y0, y1 = 90, 249, 60, 189
    assert x0 <= xs.min() and xs.max() <= x1 and y0 <= ys.min() and ys.max() <= y1
    rect = (0, x0, y0, x1, y1)
    # the box's label over the whole frame, and the box rectangle without the label
    got = LR.relief(d, planes, [(0, 0, 0, W - 1, H - 1, floor, box), rect + (floor, -1)], Q, labels=labels,
                    quantiles=(50, 500, 950))
    r, bare = got[0], got[1]
    assert r["flags"] == LR.VALID and r["n"] == planes[box]["n_inliers"] and r["n_rejected"] == 0

    # the noise-free scene (the surfaces' disparities, not rounded to the 1/16 px grid), the true
    # floor coefficients, the true mask (the scene's truth map: the box without its holes and outliers)
    _, surf, _ = SR.three_surface_scene(sigma=0.0, outliers=0.0, holes=0.0)
    gy, gx = np.mgrid[0:H, 0:W]
    clean = np.zeros((H, W))
    for i, (a, b, c) in enumerate(coefs):
        clean = np.where(surf == i, c + a * gx + b * gy, clean)
    clean = clean.astype(np.float32)[None]
    true_floor = plane_from_coef(coefs[0], W, H)
    t = LR.relief(clean, true_floor, [(0, 0, 0, W - 1, H - 1, 0, 1)], Q, labels=(truth == 1).astype(np.uint8),
                  quantiles=(50, 500, 950))[0]
    assert t["flags"] == LR.VALID and t["n"] == int((truth == 1).sum())
    err = abs(float(r["q"][1]) - float(t["q"][1]))

    # 400 seeded single-pixel lookups in the rectangle against the found floor, each against the
    # noise-free height of its own pixel
    rng = np.random.default_rng(0)
    px, py = rng.integers(x0, x1 + 1, 400), rng.integers(y0, y1 + 1, 400)
    pts = np.stack([np.zeros(400, np.int64), px, py, np.full(400, floor)], axis=1)
    single = PR.plane_distance(d, planes, pts, Q)["distance"]
    _, _, _, hclean = LR.heights(clean[0], None, None, Q, true_floor[0], -1, x0, y0, x1, y1)
    serr = np.abs(single - hclean[py - y0, px - x0].astype(np.float64))
    finite = np.isfinite(single)
    smed, smax = float(np.median(serr[finite])), float(np.max(serr[finite]))

    spread = float(r["q"][2]) - float(r["q"][0])
    print("box over floor: n %d heights %.1f .. %.1f mm, q5 %.1f q50 %.3f q95 %.1f, mean %.2f"
          % (r["n"], r["h_min"], r["h_max"], r["q"][0], r["q"][1], r["q"][2], r["mean"]))
    print("noise-free median %.3f mm: error %.3f mm" % (t["q"][1], err))
    print("400 single lookups: %d not finite, median |error| %.2f mm, largest %.0f mm"
          % (int((~finite).sum()), smed, smax))
    print("unmasked rectangle: median %.2f mean %.1f mm against %.2f mm masked; spread / 10 = %.1f mm"
          % (bare["q"][1], bare["mean"], r["mean"], spread / 10))
    assert err < smed / 4
    assert abs(float(bare["mean"]) - float(r["mean"])) > spread / 10
