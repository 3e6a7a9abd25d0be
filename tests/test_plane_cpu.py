"""The plane fit without a GPU: the numpy restatement of its definition (tests/plane_ref.py) against
known answers and a noisy scene with holes and outliers, the C structs' layout, the parameter
defaults and the host-side argument guards."""
import ctypes

import numpy as np
import pytest

import plane_ref as PR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import PLANE_DISTANCE_DTYPE, PLANE_DTYPE

Q = S.REFERENCE_Q


# ---- struct layout ----
PLANE_OFFSETS = dict(coef=0, normal=24, offset=48, centroid=56, rms_px=80, max_abs_px=88, x0=92, y0=96,
                     frame=100, area=104, n_valid=108, n_inliers=112, fits=116, flags=120, reserved=124)
DIST_OFFSETS = dict(p=0, d=12, distance=16, n=24, flags=28)


def test_struct_layout_and_defaults():
    assert ctypes.sizeof(_lib.PlaneParams) == 32
    assert ctypes.sizeof(_lib.Plane) == 128 and PLANE_DTYPE.itemsize == 128
    assert ctypes.sizeof(_lib.PlaneQuery) == 16
    assert ctypes.sizeof(_lib.PlaneDistance) == 32 and PLANE_DISTANCE_DTYPE.itemsize == 32
    assert PR.DTYPE == PLANE_DTYPE and PR.DIST_DTYPE == PLANE_DISTANCE_DTYPE
    for name, off in PLANE_OFFSETS.items():
        assert getattr(_lib.Plane, name).offset == off and PLANE_DTYPE.fields[name][1] == off, name
    for name, off in DIST_OFFSETS.items():
        assert getattr(_lib.PlaneDistance, name).offset == off and PLANE_DISTANCE_DTYPE.fields[name][1] == off, name
    assert [(n, getattr(_lib.PlaneParams, n).offset) for n, _ in _lib.PlaneParams._fields_] == [
        ("iterations", 0), ("min_inliers", 4), ("inlier_px", 8), ("min_disp", 12), ("conf_min", 16), ("reserved", 20)]
    assert (sdr.PLANE_OK, sdr.PLANE_DEGENERATE, sdr.PLANE_NONFINITE, sdr.PLANE_OUT_OF_RANGE) == (1, 2, 4, 8)
    assert (sdr.PDIST_VALID, sdr.PDIST_OUT_OF_RANGE, sdr.PDIST_NO_PLANE) == (1, 2, 4)
    assert (PR.OK, PR.DEGENERATE, PR.NONFINITE, PR.OUT_OF_RANGE) == (1, 2, 4, 8)
    L = _lib.lib()
    assert L.sdr_abi_version() == 4
    p = _lib.PlaneParams(9, 9, 9.0, 9.0, 9.0, (ctypes.c_int32 * 3)(9, 9, 9))
    L.sdr_plane_params_default(ctypes.byref(p))
    assert (p.iterations, p.min_inliers, p.inlier_px, p.min_disp, p.conf_min) == (3, 16, 1.0, -1.0, 0.0)
    assert list(p.reserved) == [0, 0, 0]
    L.sdr_plane_params_default(None)


# ---- host-side guards: every refusal comes before any device call ----
def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F, K = 8, 6, 2, 3

    def params(it=3, mi=16, px=1.0):
        return _lib.PlaneParams(it, mi, px, -1.0, 0.0)

    def fit_dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), regs=ptr, k=K, out=ptr):
        return L.sdr_fit_planes_device(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                       regs, k, out, None)

    def fit_host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=params(), regs=ptr, k=K, out=ptr):
        return L.sdr_fit_planes(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                regs, k, out)

    for fn in (fit_dev, fit_host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(regs=None) == -1 and fn(out=None) == -1 and fn(k=-1) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        assert fn(typ=2) == -1 and fn(typ=-1) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1 and fn(h=8193, fs=W * 8193) == -1
        assert fn(w=8192, stride=8192, h=4096, fs=8192 * 4096) == -1  # 2^25 pixels
        assert fn(par=params(it=9)) == -1 and fn(par=params(it=-1)) == -1
        assert fn(par=params(mi=2)) == -1
        for px in (0.0, -1.0, float("nan"), 65.0, float("inf")):
            assert fn(par=params(px=px)) == -1, px
        assert L.sdr_last_error()
        assert fn(k=0, regs=None, out=None) == 0  # K == 0: SDR_OK, nothing launched

    rp = _lib.RulerParams(0, 1, -1.0, 0.0, 0, 0)

    def dist_dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=rp, planes=ptr, np_=2, qs=ptr, k=K,
                 out=ptr):
        return L.sdr_plane_distance_device(disp, typ, stride, fs, w, h, f, None, q,
                                           ctypes.byref(par) if par else None, planes, np_, qs, k, out, None)

    def dist_host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=rp, planes=ptr, np_=2, qs=ptr, k=K,
                  out=ptr):
        return L.sdr_plane_distance(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                    planes, np_, qs, k, out)

    for fn in (dist_dev, dist_host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(qs=None) == -1 and fn(out=None) == -1 and fn(k=-1) == -1
        assert fn(planes=None) == -1 and fn(np_=-1) == -1
        assert fn(w=0) == -1 and fn(stride=W - 1) == -1 and fn(typ=2) == -1
        assert fn(w=8193, stride=8193, fs=8193 * H) == -1
        assert fn(par=_lib.RulerParams(5, 1, -1.0, 0.0, 0, 0)) == -1
        assert fn(par=_lib.RulerParams(0, 0, -1.0, 0.0, 0, 0)) == -1
        assert fn(k=0, qs=None, out=None) == 0
        assert fn(k=0, qs=None, out=None, planes=None, np_=0) == 0


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    with pytest.raises(sdr.SDRError):
        r.fit_plane(np.zeros((4, 4), np.float64), [(0, 0, 3, 3)])
    with pytest.raises(sdr.SDRError):
        r.fit_plane(np.zeros((4, 4), np.float32), [(0, 0, 3)])
    with pytest.raises(sdr.SDRError):
        r.fit_plane(np.zeros((4, 4), np.float32), [(0, 0, 3, 3)], iterations=9)
    with pytest.raises(sdr.SDRError):
        r.plane_distance(np.zeros((4, 4), np.float32), np.zeros(1, PLANE_DTYPE), [(0, 0)])
    assert r.fit_plane(np.zeros((4, 4), np.float32), []).shape == (0,)
    assert r.plane_distance(np.zeros((4, 4), np.float32), np.zeros(0, PLANE_DTYPE), []).shape == (0,)


# ---- the restatement against known answers ----
def grid_plane(H, W, c=30.0, a=0.125, b=-0.0625):
    ys, xs = np.mgrid[0:H, 0:W]
    return (c + a * xs + b * ys).astype(np.float32)[None]


def test_on_grid_plane_is_exact():
    d = grid_plane(48, 64)
    regs = [(0, 5, 7, 50, 40), (0, 0, 0, 63, 47)]
    for it in (0, 3):
        for rec, (_, x0, y0, x1, y1) in zip(PR.fit_planes(d, regs, Q, iterations=it), regs):
            assert rec["flags"] == PR.OK and rec["fits"] == it + 1
            assert rec["coef"][0] == 0.125 and rec["coef"][1] == -0.0625
            assert rec["coef"][2] == 30.0 + 0.125 * x0 - 0.0625 * y0
            assert rec["rms_px"] == 0.0 and rec["max_abs_px"] == 0.0
            assert rec["n_valid"] == rec["n_inliers"] == rec["area"] == (x1 - x0 + 1) * (y1 - y0 + 1)
            assert (rec["x0"], rec["y0"], rec["frame"]) == (x0, y0, 0)
            n, off = rec["normal"], rec["offset"]
            assert abs(np.dot(n, n) - 1.0) < 1e-15 and off >= 0
            # points of the plane, reprojected in double, lie on the 3-D plane
            worst = 0.0
            for (x, y) in ((x0, y0), (x1, y1), (x0 + 3, y1 - 2), ((x0 + x1) / 2, (y0 + y1) / 2)):
                p = PR.reproject(Q, x, y, 30.0 + 0.125 * x - 0.0625 * y)
                worst = max(worst, abs(float(np.dot(n, p) + off)))
            assert worst < 1e-9, worst
            assert abs(float(np.dot(n, rec["centroid"]) + off)) < 1e-9
    # int16 input of the same plane: the same record
    d16 = np.rint(d * 16).astype(np.int16)
    PR.assert_planes_equal(PR.fit_planes(d16, regs, Q), PR.fit_planes(d, regs, Q))


def robust_scene(seed=7, holes=0.30, outliers=0.15):
    rng = np.random.default_rng(seed)
    H, W = 360, 640
    ys, xs = np.mgrid[0:H, 0:W]
    d = 30.0 + 0.02 * xs - 0.035 * ys + rng.normal(0.0, 0.25, (H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    u = rng.random((H, W))
    d[u < holes] = -1.0
    out = (u >= holes) & (u < holes + outliers)
    d[out] = rng.uniform(1, 80, int(out.sum())).astype(np.float32)
    return d[None]


def test_robust_scene_needs_the_schedule():
    """30 % holes and 15 % uniform outliers in [1, 80): the scheduled refits recover the plane to
    |da|, |db| <= 1e-4 px/px and |dc| <= 0.02 px; the plain fit is off by more than a pixel."""
    d = robust_scene()
    reg = [(0, 100, 60, 420, 300)]
    c_true = 30.0 + 0.02 * 100 - 0.035 * 60
    r3 = PR.fit_planes(d, reg, Q, iterations=3, inlier_px=1.0)[0]
    err = (abs(r3["coef"][0] - 0.02), abs(r3["coef"][1] + 0.035), abs(r3["coef"][2] - c_true))
    print("iterations 3: |da| %.3g |db| %.3g |dc| %.3g inliers %d of %d" % (*err, r3["n_inliers"], r3["n_valid"]))
    assert r3["flags"] == PR.OK and r3["fits"] == 4
    assert err[0] <= 1e-4 and err[1] <= 1e-4 and err[2] <= 0.02, err
    r0 = PR.fit_planes(d, reg, Q, iterations=0, inlier_px=1.0)[0]
    print("iterations 0: |dc| %.3g inliers %d" % (abs(r0["coef"][2] - c_true), r0["n_inliers"]))
    assert r0["flags"] == PR.OK and r0["fits"] == 1
    assert abs(r0["coef"][2] - c_true) > 1.0
    assert r0["n_inliers"] < r3["n_inliers"] // 4


def test_corner_order_and_sign_rule():
    rng = np.random.default_rng(3)
    d = grid_plane(40, 50) + (rng.integers(-8, 9, (1, 40, 50)) / 16).astype(np.float32)
    d[rng.random(d.shape) < 0.2] = -1.0
    a = PR.fit_planes(d, [(0, 4, 6, 33, 29)], Q)
    for reg in ((0, 33, 29, 4, 6), (0, 33, 6, 4, 29), (0, 4, 29, 33, 6)):
        PR.assert_planes_equal(PR.fit_planes(d, [reg], Q), a)
    assert a[0]["flags"] == PR.OK and a[0]["offset"] >= 0
    # a surface behind the camera (negative disparities) keeps its orientation, one in front is
    # flipped: either way the camera origin is on the non-negative side
    neg = PR.fit_planes(np.where(d > 0, -d, np.float32(-1000.0)), [(0, 4, 6, 33, 29)], Q, min_disp=-100.0)
    assert neg[0]["flags"] == PR.OK and neg[0]["offset"] >= 0
    assert np.sign(neg[0]["normal"][2]) == -np.sign(a[0]["normal"][2]) or neg[0]["normal"][2] == 0
    assert a[0]["centroid"][2] > 0 > neg[0]["centroid"][2]
    # the angle helper: a plane against itself, and against one tilted by a known slope
    assert sdr.plane_angle_deg(a[0], a[0]) == 0.0
    flat = PR.fit_planes(np.full((1, 20, 20), 40.0, np.float32), [(0, 0, 0, 19, 19)], Q)[0]
    assert abs(flat["normal"][2]) == 1.0 and 0.0 < sdr.plane_angle_deg(a[0], flat) < 90.0


def test_degenerate_and_out_of_range():
    d = grid_plane(20, 30)
    recs = PR.fit_planes(d, [(0, 3, 3, 3, 12), (0, 3, 3, 12, 3), (0, 2, 2, 4, 4), (1, 0, 0, 5, 5), (0, 0, 0, 30, 5),
                             (0, 0, 0, 9, 9)], Q, min_inliers=10)
    assert recs["flags"].tolist() == [PR.DEGENERATE, PR.DEGENERATE, PR.DEGENERATE, PR.OUT_OF_RANGE,
                                      PR.OUT_OF_RANGE, PR.OK]
    assert recs["n_valid"].tolist() == [10, 10, 9, 0, 0, 100] and recs["fits"].tolist() == [0, 0, 0, 0, 0, 4]
    assert recs["area"].tolist() == [10, 10, 9, 0, 0, 100]
    for r in recs[:5]:
        assert np.isnan(r["coef"]).all() and np.isnan(r["normal"]).all() and np.isnan(r["rms_px"])
        assert np.isnan(r["max_abs_px"]) and r["n_inliers"] == 0
    # a chain that runs out of inliers stops where it does
    rng = np.random.default_rng(5)
    noisy = (rng.uniform(1, 80, (1, 20, 30)) * 16).round().astype(np.float32) / 16
    r = PR.fit_planes(noisy, [(0, 0, 0, 29, 19)], Q, iterations=8, inlier_px=0.0625, min_inliers=200)[0]
    assert r["flags"] == PR.DEGENERATE and 1 <= r["fits"] < 9 and np.isnan(r["coef"]).all()


def test_point_query_restatement():
    d = grid_plane(30, 40)
    planes = PR.fit_planes(d, [(0, 2, 2, 37, 27), (0, 5, 5, 5, 9)], Q)
    assert planes["flags"].tolist() == [PR.OK, PR.DEGENERATE]
    d[0, 10, 10] += 4.0  # 4 px nearer than the plane
    pts = [(0, 10, 10, 0), (0, 20, 15, 0), (0, 20, 15, 1), (0, 20, 15, 2), (0, 20, 15, -1), (0, 40, 0, 0),
           (1, 0, 0, 0), (0, 0, 30, 5)]
    out = PR.plane_distance(d, planes, pts, Q)
    assert out["flags"].tolist() == [1, 1, 4, 4, 4, 2, 2, 2 | 4]
    assert out["distance"][0] > 1.0 and abs(out["distance"][1]) < 1e-3  # float XYZ against a double plane
    assert np.isnan(out["distance"][2:]).all() and np.isnan(out["p"][5:]).all() and (out["n"][5:] == 0).all()
    assert np.array_equal(out["p"][2], out["p"][1]) and out["d"][2] == d[0, 15, 20]
