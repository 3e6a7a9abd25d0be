"""GPU: the plane fit and the point-to-plane distance (sdr_fit_planes*, sdr_plane_distance*,
csrc/sdr_plane.hip) through every layer, exact against the numpy restatement (tests/plane_ref.py):
doubles and floats as bit patterns, counts and flags exactly."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

import plane_ref as PR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import _lib  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import PLANE_DISTANCE_DTYPE, PLANE_DTYPE, as_queries, as_segments  # noqa: E402
from stereo_depth_ruler_amd.sgbm import _Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def make_scene(rng, F, H, W, holes=0.2, outliers=0.1, weird=0.02, sigma=0.25):
    """A tilted plane a frame with noise on the 1/16 px grid, `holes` of the pixels -1, `outliers`
    uniform in [1, 80), a few NaN / inf / 0 / -0 / 2048."""
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.empty((F, H, W), np.float32)
    for f in range(F):
        a, b = rng.uniform(-0.1, 0.1, 2)
        d[f] = np.round((rng.uniform(20, 50) + a * xs + b * ys + rng.normal(0, sigma, (H, W))) * 16) / 16
    u = rng.random((F, H, W))
    d[u < holes] = -1.0
    pick = (u >= holes) & (u < holes + outliers)
    d[pick] = (np.floor(rng.uniform(1, 80, int(pick.sum())) * 16) / 16).astype(np.float32)
    pick = (u >= holes + outliers) & (u < holes + outliers + weird)
    d[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2048.0], np.float32), int(pick.sum()))
    return d


def to_s16(d):
    return np.nan_to_num(d * 16, nan=-16.0, posinf=32767.0, neginf=-32768.0).clip(-32768, 32767).astype(np.int16)


def random_regions(rng, K, F, H, W):
    return np.stack([rng.integers(0, F, K), rng.integers(0, W, K), rng.integers(0, H, K),
                     rng.integers(0, W, K), rng.integers(0, H, K)], axis=1).astype(np.int32)


def fit_device(disp, regs, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0, **kw):
    r = sdr.Ruler(Qm, min_disp=min_disp, conf_min=conf_min)
    d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    rec = r.fit_plane_device(d, regs, conf=c, **kw)
    torch.cuda.synchronize()
    return rec.cpu().numpy().reshape(-1).view(PLANE_DTYPE)


def check_fit(disp, regs, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0, **kw):
    """Device records == the restatement's."""
    regs = as_segments(regs)
    got = fit_device(disp, regs, conf=conf, Qm=Qm, min_disp=min_disp, conf_min=conf_min, **kw)
    want = PR.fit_planes(disp, regs, Qm, conf=conf, min_disp=min_disp, conf_min=conf_min, **kw)
    PR.assert_planes_equal(got, want)
    return got


# ---- borders and tiny shapes ----
@pytest.mark.parametrize("H, W", [(5, 7), (24, 40)])
def test_borders_and_tiny_shapes(H, W):
    rng = np.random.default_rng(H)
    disp = make_scene(rng, 1, H, W, holes=0.1, outliers=0.05)
    x1, y1 = W - 1, H - 1
    regs = [(0, 0, 0, 1, 1), (0, x1 - 1, y1 - 1, x1, y1), (0, 0, y1 - 1, 1, y1),    # 2 x 2 in three corners
            (0, 0, 0, x1, 0), (0, 0, y1, x1, y1), (0, 2, 2, 2, 2),                 # N x 1 rows, a single pixel
            (0, 0, 0, 0, y1), (0, x1, 0, x1, y1),                                  # 1 x N columns
            (0, 0, 0, x1, y1), (0, x1, y1, 0, 0), (0, x1, 0, 0, y1), (0, 0, y1, x1, 0)]  # the map, corners in every order
    for it in (0, 2):
        got = check_fit(disp, regs, iterations=it, min_inliers=3, inlier_px=1.0)
        assert (got["flags"][3:8] == PR.DEGENERATE).all() and (got["flags"] & PR.OUT_OF_RANGE == 0).all()
        PR.assert_planes_equal(got[9:], np.repeat(got[8:9], 3))
        assert got["area"].tolist()[:3] == [4, 4, 4] and got["area"][8] == H * W


# ---- validity ----
def test_validity_plants():
    H, W = 9, 30
    ys, xs = np.mgrid[0:H, 0:W]
    d = (30.0 + 0.125 * xs - 0.0625 * ys).astype(np.float32)[None]
    c = np.full((1, H, W), 100.0, np.float32)
    d[0, 1, 1:7] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2048.0], np.float32)
    d[0, 3, 2:5] = 7.0                                                       # equal to min_disp below
    d[0, 5, 3], d[0, 5, 4] = np.float32(2047.9375), np.float32(-2047.9375)  # the largest magnitudes on the grid
    c[0, 7, 10], c[0, 7, 11], c[0, 7, 12], c[0, 7, 13] = 50.0, np.float32(49.999), np.nan, np.float32(50.001)
    regs = [(0, 0, 0, W - 1, H - 1), (0, 0, 0, 8, 8), (0, 8, 6, 16, 8)]
    got = check_fit(d, regs, conf=c, min_disp=7.0, conf_min=50.0, min_inliers=3)
    # NaN, +-inf, 0, -0 (<= 7), 2048, three sevens, -2047.9375, and the confidences 49.999 and NaN
    assert got["n_valid"][0] == H * W - (6 + 3 + 1 + 2)
    got = check_fit(d, regs, conf=c, min_disp=-1.0, conf_min=50.0, min_inliers=3)
    assert got["n_valid"][0] == H * W - (4 + 1 + 2)  # 0 and -0 are valid now, the sevens too
    got = check_fit(d, regs, min_disp=-3000.0, min_inliers=3, iterations=1)
    assert got["n_valid"][0] == H * W - 4            # the non-finite values and 2048
    # conf_min plays no part without a confidence map; a NaN conf_min with one rejects everything
    check_fit(d, regs, conf_min=float("nan"), min_inliers=3)
    got = check_fit(d, regs, conf=c, conf_min=float("nan"), min_inliers=3)
    assert (got["n_valid"] == 0).all() and (got["flags"] == PR.DEGENERATE).all()
    # the int16 map: -32768 and 32767 are ordinary values, v * 0.0625 == min_disp is rejected
    d16 = to_s16(d)
    d16[0, 5, 3], d16[0, 5, 4], d16[0, 3, 2:5] = 32767, -32768, 112
    got = check_fit(d16, regs, conf=c, min_disp=7.0, conf_min=50.0, min_inliers=3)
    assert got["n_valid"][0] == int(((d16[0] > 112) & ~(c[0] < 50.0) & ~np.isnan(c[0])).sum())


def test_too_few_valid_values_and_none():
    rng = np.random.default_rng(2)
    disp = np.full((1, 20, 30), -1.0, np.float32)
    ys, xs = np.nonzero(rng.random((20, 30)) < 0.05)
    disp[0, ys, xs] = 40.0 + 0.25 * xs
    n = len(xs)
    regs = [(0, 0, 0, 29, 19), (0, 0, 0, 3, 3)]
    got = check_fit(disp, regs, min_inliers=n + 1)
    assert got["n_valid"][0] == n and got["flags"][0] == PR.DEGENERATE and got["fits"][0] == 0
    got = check_fit(disp, regs, min_inliers=3, iterations=1)
    assert got["flags"][0] == PR.OK
    got = check_fit(np.full((1, 20, 30), -1.0, np.float32), regs)
    assert (got["n_valid"] == 0).all() and (got["flags"] == PR.DEGENERATE).all() and np.isnan(got["coef"]).all()


# ---- residuals exactly on the band ----
def test_residuals_on_the_band():
    """An on-grid plane and quadruples of planted pixels +-delta that leave the least-squares plane
    where it is (their sum and first moments vanish), delta exactly the final band T, T + 1/16, the
    scheduled band 2T and 2T + 1/16: |r| <= band includes the equality."""
    H, W = 41, 61
    ys, xs = np.mgrid[0:H, 0:W]
    base = (30.0 + 0.125 * xs - 0.0625 * ys).astype(np.float32)
    for T in (1.0, 0.5):
        d = base.copy()
        deltas = (T, T + 0.0625, 2 * T, 2 * T + 0.0625)
        for i, delta in enumerate(deltas):
            s, t = 3 + 5 * i, 2 + 4 * i
            for sx, sy in ((-1, -1), (1, 1), (-1, 1), (1, -1)):
                d[20 + sy * t, 30 + sx * s] += np.float32(delta * sx * sy)
        for it in (0, 1, 2):
            got = check_fit(d[None], [(0, 0, 0, W - 1, H - 1)], iterations=it, inlier_px=T, min_inliers=3)[0]
            assert got["coef"].tolist() == [0.125, -0.0625, 30.0] and got["flags"] == PR.OK
            assert got["n_inliers"] == H * W - 12 and got["max_abs_px"] == np.float32(T)
        d16 = np.rint(d * 16).astype(np.int16)[None]
        g16 = check_fit(d16, [(0, 0, 0, W - 1, H - 1)], iterations=2, inlier_px=T, min_inliers=3)[0]
        assert g16["n_inliers"] == H * W - 12


# ---- slices ----
@pytest.fixture(scope="module")
def frame():
    """One 360 x 640 scene, its whole-frame restatement computed once."""
    rng = np.random.default_rng(7)
    disp = make_scene(rng, 1, 360, 640, holes=0.3, outliers=0.15, weird=0.01)
    regs = as_segments([(0, 0, 0, 639, 359), (0, 101, 60, 227, 154)])  # 230400 and 127 x 95 pixels: no slice multiple
    return disp, regs, PR.fit_planes(disp, regs, Q)


def test_whole_frame_and_mid_size_region(frame):
    disp, regs, want = frame
    got = fit_device(disp, regs)
    PR.assert_planes_equal(got, want)
    assert (got["flags"] == PR.OK).all() and got["area"].tolist() == [230400, 127 * 95] and (got["fits"] == 4).all()
    # the result does not depend on what else the launch holds, nor on the order of the regions
    PR.assert_planes_equal(fit_device(disp, regs[::-1].copy()), want[::-1])
    PR.assert_planes_equal(fit_device(to_s16(disp), regs[1:], iterations=1),
                           PR.fit_planes(to_s16(disp), regs[1:], Q, iterations=1))


def test_many_regions_in_one_launch(frame):
    disp = frame[0][:, :96, :128]
    rng = np.random.default_rng(8)
    regs = random_regions(rng, 65, 1, 96, 128)
    regs[0] = (0, 0, 0, 127, 95)      # 6 slices exactly
    regs[1] = (0, 1, 0, 127, 95)      # 127 x 96
    regs[2] = (0, 5, 5, 6, 6)
    regs[3] = (0, 128, 0, 3, 3)       # out of range
    regs[4] = (1, 0, 0, 3, 3)
    regs[5] = (0, 0, -1, 3, 3)
    got = check_fit(disp, regs, min_inliers=8)
    assert (got["flags"][3:6] == PR.OUT_OF_RANGE).all() and (got["area"][3:6] == 0).all()
    assert np.isnan(got["coef"][3:6]).all() and (got["flags"] == PR.OK).sum() >= 40
    one = check_fit(disp, regs[7:8], min_inliers=8)  # K = 1
    PR.assert_planes_equal(one, got[7:8])


def test_more_regions_than_one_grid_holds():
    """65 540 regions: the sweeps are launched in chunks of the grid's y extent (65 535)."""
    rng = np.random.default_rng(16)
    disp = make_scene(rng, 2, 12, 16, weird=0.0)
    uniq = as_segments([(0, 0, 0, 15, 11), (1, 2, 1, 12, 9), (0, 16, 0, 1, 1), (1, 3, 3, 3, 8)])
    regs = np.ascontiguousarray(np.tile(uniq, (16385, 1)))
    got = fit_device(disp, regs, iterations=1, inlier_px=4.0, min_inliers=6)
    want = PR.fit_planes(disp, uniq, Q, iterations=1, inlier_px=4.0, min_inliers=6)
    assert want["flags"].tolist() == [PR.OK, PR.OK, PR.OUT_OF_RANGE, PR.DEGENERATE]
    PR.assert_planes_equal(got, np.tile(want, 16385))


def test_no_regions_writes_nothing():
    disp = torch.zeros((2, 4, 4), dtype=torch.float32, device=dev())
    out = torch.full((4, 128), 0x5A, dtype=torch.uint8, device=dev())
    p = _lib.PlaneParams(3, 16, 1.0, -1.0, 0.0)
    check(lib().sdr_fit_planes_device(disp.data_ptr(), 0, 4, 16, 4, 4, 2, None, _Q(Q), ctypes.byref(p), None, 0,
                                      out.data_ptr(), None))
    rp = _lib.RulerParams(0, 1, -1.0, 0.0, 0, 0)
    check(lib().sdr_plane_distance_device(disp.data_ptr(), 0, 4, 16, 4, 4, 2, None, _Q(Q), ctypes.byref(rp),
                                          out.data_ptr(), 4, None, 0, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert (out == 0x5A).all()
    r = sdr.Ruler(Q)
    assert r.fit_plane(disp, []).shape == (0,) and r.fit_plane_device(disp, []).shape == (0, 128)
    assert r.plane_distance(disp, np.zeros(0, PLANE_DTYPE), []).shape == (0,)


# ---- inputs ----
@pytest.mark.parametrize("iterations", [0, 1, 3, 8])
@pytest.mark.parametrize("i16", [False, True])
def test_frames_strides_conf_and_iterations(iterations, i16):
    rng = np.random.default_rng(9)
    F, H, W = 3, 33, 47
    disp = make_scene(rng, F, H, W)
    if i16:
        disp = to_s16(disp)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    regs = random_regions(rng, 12, F, H, W)
    regs[:3] = [(0, 0, 0, W - 1, H - 1), (1, W - 1, H - 1, 0, 0), (2, 3, 30, 40, 2)]
    kw = dict(iterations=iterations, inlier_px=0.75, min_inliers=6)
    got = check_fit(disp, regs, **kw)
    # (the int16 map's 32767s pull fit 0 far enough that one short chain runs out of inliers)
    assert len(set(regs[:, 0].tolist())) == 3 and (got["flags"][:3] == PR.OK).sum() >= 2
    with_conf = check_fit(disp, regs, conf=conf, conf_min=60.0, **kw)
    assert (with_conf["n_valid"][:3] < got["n_valid"][:3]).all()
    # rows and frames padded: the same records
    pad = torch.full((F, H + 2, W + 5), -7, dtype=torch.int16 if i16 else torch.float32, device=dev())
    pad[:, :H, :W] = torch.from_numpy(disp).to(dev())
    view = pad[:, :H, :W]
    assert view.stride(1) == W + 5 and view.stride(0) == (H + 2) * (W + 5)
    rec = sdr.Ruler(Q).fit_plane_device(view, regs, **kw)
    torch.cuda.synchronize()
    PR.assert_planes_equal(rec.cpu().numpy().reshape(-1).view(PLANE_DTYPE), got)


# ---- the 3-D plane ----
def test_nonfinite_plane_keeps_the_coefficients():
    """A Q whose last row is zero makes every h3 zero: normal, offset and centroid NaN, flag
    NONFINITE, the coefficients and statistics intact."""
    rng = np.random.default_rng(10)
    disp = make_scene(rng, 1, 30, 40, weird=0.0)
    Qz = np.array(Q)
    Qz[3] = 0.0
    regs = [(0, 0, 0, 39, 29), (0, 4, 4, 30, 20)]
    got = check_fit(disp, regs, Qm=Qz, min_inliers=6)
    ok = check_fit(disp, regs, min_inliers=6)
    assert (got["flags"] == PR.NONFINITE).all() and (ok["flags"] == PR.OK).all()
    for k in ("normal", "offset", "centroid"):
        assert np.isnan(got[k]).all()
        assert (np.ascontiguousarray(got[k]).view(np.uint64) == 0x7FF8000000000000).all()  # canonical
    for k in ("coef", "rms_px", "max_abs_px", "n_inliers", "n_valid", "fits"):
        assert np.array_equal(got[k], ok[k]), k


def test_sign_rule_flips_and_keeps():
    rng = np.random.default_rng(11)
    disp = make_scene(rng, 1, 30, 40, weird=0.0)
    front = check_fit(disp, [(0, 2, 2, 37, 27)], min_inliers=6)[0]
    back = check_fit(np.where(disp > 0, -disp, np.float32(-1000.0)), [(0, 2, 2, 37, 27)], min_disp=-100.0,
                     min_inliers=6)[0]
    assert front["flags"] == PR.OK and back["flags"] == PR.OK
    assert front["offset"] >= 0 and back["offset"] >= 0
    assert front["centroid"][2] > 0 > back["centroid"][2]
    # the negated map's surface is the point mirror of the other: e1 x e2 is the same vector for both,
    # so exactly one of the two was flipped
    assert np.allclose(back["normal"], -front["normal"], rtol=0, atol=1e-9)
    assert abs(back["offset"] - front["offset"]) <= 1e-9 * front["offset"]


# ---- queries ----
def query_device(r, disp, planes, pts, conf=None):
    d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    out = r.plane_distance_device(d, planes, pts, conf=c)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-1).view(PLANE_DISTANCE_DTYPE)


@pytest.mark.parametrize("radius, min_count", [(0, 1), (2, 3)])
def test_point_queries(radius, min_count):
    rng = np.random.default_rng(12)
    F, H, W = 2, 30, 44
    disp = make_scene(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    regs = as_segments([(0, 0, 0, W - 1, H - 1), (1, 5, 5, 40, 25), (0, 3, 3, 3, 20), (0, W, 0, 1, 1)])
    kw = dict(min_disp=-1.0, conf_min=40.0)
    planes = check_fit(disp, regs, conf=conf, min_inliers=6, **kw)
    assert planes["flags"].tolist() == [PR.OK, PR.OK, PR.DEGENERATE, PR.OUT_OF_RANGE]
    K = 200
    pts = np.stack([rng.integers(0, F, K), rng.integers(0, W, K), rng.integers(0, H, K),
                    rng.integers(0, 4, K)], axis=1).astype(np.int32)
    pts[:8] = [(0, 0, 0, 0), (1, W - 1, H - 1, 1), (0, 5, 5, 4), (0, 5, 5, -1), (2, 0, 0, 0), (0, W, 0, 0),
               (0, 0, -1, 1), (-1, 0, 0, 7)]
    r = sdr.Ruler(Q, radius=radius, min_count=min_count, **kw)
    got = query_device(r, disp, planes, pts, conf=conf)
    want = PR.plane_distance(disp, planes, pts, Q, conf=conf, radius=radius, min_count=min_count, **kw)
    PR.assert_distances_equal(got, want)
    assert got["flags"][2:8].tolist() == [4, 4, 2, 2, 2, 2 | 4]
    assert (got["flags"] & PR.PDIST_VALID).sum() >= 40
    # int16 maps, and the host ABI
    d16 = to_s16(disp)
    PR.assert_distances_equal(query_device(r, d16, planes, pts, conf=conf),
                              PR.plane_distance(d16, planes, pts, Q, conf=conf, radius=radius, min_count=min_count, **kw))
    PR.assert_distances_equal(r.plane_distance(disp, planes, pts, conf=conf), want)
    # (K, 3) points are on frame 0
    f0 = pts[pts[:, 0] == 0]
    PR.assert_distances_equal(r.plane_distance(disp, planes, f0[:, 1:]), r.plane_distance(disp, planes, f0))


def test_fit_and_queries_chain_on_one_stream():
    """The records tensor of fit_plane_device feeds plane_distance_device on the same stream with
    no host round trip: one copy-out of 32 bytes a query at the end."""
    rng = np.random.default_rng(13)
    H, W = 40, 60
    disp = make_scene(rng, 1, H, W)
    regs = as_segments([(0, 0, 0, W - 1, H - 1), (0, 10, 10, 30, 30)])
    pts = as_queries([(0, int(x), int(y), int(p)) for x, y, p in
                      zip(rng.integers(0, W, 64), rng.integers(0, H, 64), rng.integers(0, 3, 64))])
    r = sdr.Ruler(Q, radius=1, min_count=2)
    d = torch.from_numpy(disp).to(dev())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    planes_t = r.fit_plane_device(d, regs, stream=side, min_inliers=6)
    out_t = r.plane_distance_device(d, planes_t, pts, stream=side)
    side.synchronize()
    planes = planes_t.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    PR.assert_planes_equal(planes, PR.fit_planes(disp, regs, Q, min_inliers=6))
    PR.assert_distances_equal(out_t.cpu().numpy().reshape(-1).view(PLANE_DISTANCE_DTYPE),
                              PR.plane_distance(disp, planes, pts, Q, radius=1, min_count=2))


# ---- hypothesis ----
@settings(max_examples=hyp_examples(30), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(1, 64), W=st.integers(1, 64), iterations=st.integers(0, 8), min_inliers=st.integers(3, 40),
       inlier_q=st.integers(1, 64), with_conf=st.booleans(), i16=st.booleans(), seed=st.integers(0, 2 ** 31 - 1))
def test_hypothesis_random_scenes(H, W, iterations, min_inliers, inlier_q, with_conf, i16, seed):
    rng = np.random.default_rng(seed)
    F = int(rng.integers(1, 3))
    disp = make_scene(rng, F, H, W, holes=float(rng.uniform(0, 0.6)), outliers=float(rng.uniform(0, 0.3)),
                      sigma=float(rng.uniform(0, 1.0)))
    if i16:
        disp = to_s16(disp)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32) if with_conf else None
    regs = random_regions(rng, int(rng.integers(1, 7)), F, H, W)
    if rng.random() < 0.3:
        regs[0, int(rng.integers(0, 5))] = int(rng.choice([-1, 100]))
    planes = check_fit(disp, regs, conf=conf, conf_min=float(rng.uniform(0, 200)), iterations=iterations,
                       inlier_px=inlier_q / 8.0, min_inliers=min_inliers)
    pts = np.stack([rng.integers(0, F, 6), rng.integers(-1, W + 1, 6), rng.integers(-1, H + 1, 6),
                    rng.integers(-1, len(regs) + 1, 6)], axis=1).astype(np.int32)
    radius = int(rng.integers(0, 5))
    r = sdr.Ruler(Q, radius=radius, min_count=2)
    PR.assert_distances_equal(query_device(r, disp, planes, pts, conf=conf),
                              PR.plane_distance(disp, planes, pts, Q, conf=conf, radius=radius, min_count=2))


# ---- the host ABI ----
def test_host_abi_equals_device_abi():
    rng = np.random.default_rng(14)
    F, H, W = 2, 27, 45
    disp = make_scene(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    regs = random_regions(rng, 20, F, H, W)
    regs[3] = (F, 0, 0, 5, 5)
    kw = dict(iterations=2, inlier_px=1.5, min_inliers=5)
    got = check_fit(disp, regs, conf=conf, conf_min=30.0, **kw)
    r = sdr.Ruler(Q, conf_min=30.0)
    PR.assert_planes_equal(r.fit_plane(disp, regs, conf=conf, **kw), got)
    wide = np.full((F, H, W + 3), np.nan, np.float32)  # a strided host map
    wide[:, :, :W] = disp
    PR.assert_planes_equal(r.fit_plane(wide[:, :, :W], regs, conf=conf, **kw), got)
    d16 = to_s16(disp)
    PR.assert_planes_equal(r.fit_plane(d16, regs, **kw), fit_device(d16, regs, conf_min=30.0, **kw))
    # the tensor form of fit_plane() downloads the same records
    t = r.fit_plane(torch.from_numpy(disp).to(dev()), regs, conf=torch.from_numpy(conf).to(dev()), **kw)
    PR.assert_planes_equal(t, got)


# ---- end to end ----
def test_live_loop_fit_plane_on_the_frame_stream():
    """LiveLoop.fit_plane / plane_distance run on the frame's stream right after the frame; the
    records equal Ruler.fit_plane on the downloaded disparity and confidence."""
    from stereo_depth_ruler_amd.pipeline import LiveLoop
    from stereo_depth_ruler_amd.rectify import StereoRectifier

    sbs = S.sbs_bgr_frame(96, 400, 80, seed=21)
    H, W = sbs.shape[0], sbs.shape[1] // 2
    K = np.array([[700.0, 0, W / 2], [0, 700.0, H / 2], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    cfg = types.SimpleNamespace(imageSize=(W, H), cameraMatrixLeft=K, cameraMatrixRight=K, distCoeffsLeft=None,
                                distCoeffsRight=None, R1=np.eye(3), R2=np.eye(3), P1=P, P2=P)
    rect = StereoRectifier(cfg)
    frame = torch.from_numpy(sbs[None]).to(dev())
    plain = LiveLoop(rect, Q, 1)
    with pytest.raises(RuntimeError):
        plain.fit_plane([(0, 0, 5, 5)], torch.cuda.current_stream(dev()))
    plain.close()
    loop = LiveLoop(rect, Q, 1, ruler=dict(radius=1, min_count=2, conf_min=100.0))
    regs = as_segments([(0, 0, 0, loop.w2 - 1, loop.h2 - 1), (0, 20, 5, 120, 40), (0, 150, 30, 60, 10)])
    pts = as_queries([(0, 30, 10, 0), (0, 100, 30, 1), (0, 70, 20, 2), (0, 10, 10, 3)])
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        planes_t = loop.fit_plane(regs, side, iterations=2, inlier_px=2.0, min_inliers=8)
        out_t = loop.plane_distance(planes_t, pts, side)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    planes = planes_t.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    PR.assert_planes_equal(planes, loop.ruler.fit_plane(disp, regs, conf=conf, iterations=2, inlier_px=2.0,
                                                        min_inliers=8))
    PR.assert_planes_equal(planes, PR.fit_planes(disp, regs, Q, conf=conf, iterations=2, inlier_px=2.0,
                                                 min_inliers=8, min_disp=loop.ruler.min_disp, conf_min=100.0))
    PR.assert_distances_equal(out_t.cpu().numpy().reshape(-1).view(PLANE_DISTANCE_DTYPE),
                              PR.plane_distance(disp, planes, pts, Q, conf=conf, radius=1, min_count=2,
                                                min_disp=loop.ruler.min_disp, conf_min=100.0))
    assert planes["n_valid"][0] > 0
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()


# ---- the C++ facade ----
def test_cpp_facade_plane(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::fit_plane and plane_distance give Python's records as
    bytes (tests/cpp/facade_plane.cpp)."""
    exe = tmp_path / "facade_plane"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_plane.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    rng = np.random.default_rng(15)
    H, W, K, NQ, radius, mc = 29, 43, 9, 24, 1, 2
    disp = make_scene(rng, 1, H, W)
    conf = rng.uniform(0, 255, (1, H, W)).astype(np.float32)
    regs = random_regions(rng, K, 1, H, W)
    regs[0] = (0, 0, 0, W - 1, H - 1)
    regs[1] = (0, W, 0, 2, 2)
    pts = np.stack([np.zeros(NQ, np.int64), rng.integers(0, W, NQ), rng.integers(0, H, NQ),
                    rng.integers(-1, K + 1, NQ)], axis=1).astype(np.int32)
    disp[0].tofile(tmp_path / "disp.bin")
    conf[0].tofile(tmp_path / "conf.bin")
    regs.tofile(tmp_path / "regs.bin")
    pts.tofile(tmp_path / "pts.bin")
    np.asarray(Q, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), str(K), str(NQ), str(radius), str(mc), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "single_equal=1" in res.stdout and "bad_iterations_code=-1" in res.stdout
    r = sdr.Ruler(Q, radius=radius, min_count=mc, conf_min=10.0)
    want = fit_device(disp, regs, conf=conf, conf_min=10.0, iterations=2, inlier_px=1.5, min_inliers=6)
    assert (tmp_path / "planes.bin").read_bytes() == want.tobytes()
    wd = query_device(r, disp, want, pts, conf=conf)
    assert (tmp_path / "dist.bin").read_bytes() == wd.tobytes()
