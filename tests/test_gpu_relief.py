"""GPU: the relief (sdr_plane_relief*, csrc/sdr_relief.hip) through every layer, every record
compared bit for bit with the numpy restatement (tests/relief_ref.py)."""
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
import plane_search_ref as SR  # noqa: E402
import relief_ref as LR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import PLANE_DTYPE, RELIEF_DTYPE, as_relief_queries  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q
EYE = np.eye(4)
SLICE = 2048  # pixels a workgroup of the sweeps (csrc/sdr_region.hpp, kRegionSlice)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def to_s16(d):
    return np.nan_to_num(d * 16, nan=-16.0, posinf=32767.0, neginf=-32768.0).clip(-32768, 32767).astype(np.int16)


def records(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(-1).view(RELIEF_DTYPE)


def check_relief(disp, planes, regions, labels=None, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0,
                 quantiles=(50, 500, 950), band=0.0):
    """Device records == the restatement's, on every bit."""
    r = sdr.Ruler(Qm, min_disp=min_disp, conf_min=conf_min)
    d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev()) if labels is not None else None
    got = records(r.relief_device(d, planes, regions, labels=lab, conf=c, quantiles=quantiles, band=band))
    want = LR.relief(disp, planes, regions, Qm, labels=labels, conf=conf, quantiles=quantiles, band=band,
                     min_disp=min_disp, conf_min=conf_min)
    LR.assert_reliefs_equal(got, want)
    return got


def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """With Q the identity and this record, hf is the float disparity itself (+0 for -0)."""
    p = np.zeros(1, PLANE_DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def planted(bits, H, W):
    """A (1, H, W) float map from uint32 bit patterns, repeated to fill it."""
    b = np.resize(np.asarray(bits, np.uint32), H * W)
    return b.view(np.float32).reshape(1, H, W).copy()


ALL8 = (0, 125, 250, 375, 500, 625, 750, 1000)


# ---- planted keys ----
def test_planted_keys_through_the_three_passes():
    rng = np.random.default_rng(1)
    pl = flat_plane()
    kw = dict(Qm=EYE, min_disp=-3e38)
    base = np.uint32(0x42280000)  # 42.0
    for H, W in ((8, 8), (48, 64)):
        reg = [(0, 0, 0, W - 1, H - 1)]
        # all equal: every quantile in one bin through all three passes
        got = check_relief(planted([base], H, W), pl, reg, quantiles=ALL8, **kw)
        assert (got["q"][0] == 42.0).all() and got["h_min"][0] == got["h_max"][0] == 42.0 and got["n"][0] == H * W
        # the lowest 10 bits only, the middle 11 bits only
        low = planted(base | rng.integers(0, 1024, H * W).astype(np.uint32), H, W)
        got = check_relief(low, pl, reg, quantiles=ALL8, **kw)
        assert len(set((np.ascontiguousarray(got["q"][0]).view(np.uint32) >> 10).tolist())) == 1
        mid = planted(base | (rng.integers(0, 2048, H * W).astype(np.uint32) << 10), H, W)
        check_relief(mid, pl, reg, quantiles=ALL8, **kw)
        # around zero: negatives, -0.0, +0.0, positives
        z = rng.normal(0, 3, H * W).astype(np.float32)
        z[::7], z[1::7] = -0.0, 0.0
        got = check_relief(z.reshape(1, H, W), pl, reg, quantiles=ALL8, band=1.5, **kw)
        assert got["n"][0] == H * W and got["h_min"][0] < 0 < got["h_max"][0]
        assert 0 < got["n_above"][0] and 0 < got["n_below"][0] and got["n_above"][0] + got["n_below"][0] < H * W
        zeros = planted([0x80000000, 0x00000000, 0x80000000], H, W)  # -0 becomes +0: one key
        got = check_relief(zeros, pl, reg, quantiles=(0, 500, 1000), **kw)
        assert np.ascontiguousarray(got["q"][0][:3]).view(np.uint32).tolist() == [0, 0, 0]
        assert np.ascontiguousarray(got["h_min"]).view(np.uint32)[0] == 0 and got["sum256"][0] == 0
        # denormals of either sign
        den = planted(np.concatenate([rng.integers(1, 1 << 23, 40), rng.integers(1, 1 << 23, 40) | (1 << 31)]), H, W)
        got = check_relief(den, pl, reg, quantiles=ALL8, **kw)
        assert got["n"][0] == H * W and 0 < abs(got["q"][0][3]) < 1.2e-38
        # two, and all eight, quantiles in one first-pass bin (42.0 .. 42.01: the top 11 bits agree)
        near = (42.0 + rng.random(H * W) * 0.01).astype(np.float32).reshape(1, H, W)
        check_relief(near, pl, reg, quantiles=(400, 600), **kw)
        got = check_relief(near, pl, reg, quantiles=ALL8, **kw)
        assert len(set((np.ascontiguousarray(got["q"][0]).view(np.uint32) >> 21).tolist())) == 1
        # repeated and unsorted permille; no quantile at all
        wide = (rng.normal(0, 1e4, H * W) * rng.choice([1e-6, 1.0, 50.0], H * W)).astype(np.float32).reshape(1, H, W)
        got = check_relief(wide, pl, reg, quantiles=(950, 50, 950, 0, 500, 500, 1000, 50), **kw)
        assert got["q"][0][0] == got["q"][0][2] and got["q"][0][1] == got["q"][0][7]
        got = check_relief(wide, pl, reg, quantiles=(), **kw)
        assert np.isnan(got["q"][0]).all() and got["flags"][0] == LR.VALID and np.isfinite(got["mean"][0])


def test_planted_limits_and_invalid_values():
    pl = flat_plane()
    H, W = 8, 16
    d = np.full((1, H, W), 3.0, np.float32)
    d[0, 0, :6] = np.array([1048575.9375, 1048576.0, -1048575.9375, -1048576.0, 2e6, -3e7], np.float32)
    d[0, 1, :4] = np.array([np.inf, -np.inf, np.nan, -np.nan], np.float32)
    reg = [(0, 0, 0, W - 1, H - 1)]
    got = check_relief(d, pl, reg, Qm=EYE, min_disp=-3e38, quantiles=(0, 1000))
    assert got["n_valid"][0] == H * W - 4 and got["n_rejected"][0] == 4 and got["n"][0] == H * W - 8
    assert got["h_max"][0] == np.float32(1048575.9375) and got["h_min"][0] == np.float32(-1048575.9375)
    assert got["q"][0][0] == got["h_min"][0] and got["q"][0][1] == got["h_max"][0]
    # an offset moves 1048575.9375 onto the limit and -1048576 inside it; a non-finite plane rejects
    # every pixel
    got = check_relief(d, flat_plane(0.0625), reg, Qm=EYE, min_disp=-3e38, quantiles=(0, 1000))
    assert got["n_rejected"][0] == 4 and got["h_min"][0] == np.float32(-1048575.9375)
    assert got["h_max"][0] == np.float32(3.0625)
    got = check_relief(d, flat_plane(np.inf), reg, Qm=EYE, min_disp=-3e38)
    assert got["flags"][0] == LR.EMPTY and got["n_valid"][0] == H * W - 4 == got["n_rejected"][0]
    # min_disp itself is invalid (strict)
    got = check_relief(d, pl, reg, Qm=EYE, min_disp=3.0)
    assert got["n_valid"][0] == 3


# ---- shapes and edges ----
def ramp_scene(rng, F, H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    d = (30.0 + 0.05 * xs - 0.03 * ys)[None] + rng.normal(0, 0.4, (F, H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    d[rng.random((F, H, W)) < 0.15] = -1.0
    return d


@pytest.mark.parametrize("W", [63, 64, 65])
def test_region_shapes_and_corner_orders(W):
    rng = np.random.default_rng(W)
    H = 37
    d = ramp_scene(rng, 1, H, W)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1)], Q)
    x1, y1 = W - 1, H - 1
    regs = [(0, 0, 0, 0, 0), (0, x1, y1, x1, y1), (0, 5, 7, 5, 7),           # 1 x 1
            (0, 0, 3, x1, 3), (0, 0, y1, x1, y1), (0, 4, 0, 4, y1), (0, x1, 0, x1, y1),  # 1 x N, N x 1
            (0, 0, 0, x1, y1), (0, x1, y1, 0, 0), (0, x1, 0, 0, y1), (0, 0, y1, x1, 0),  # the frame, every order
            (0, 3, 30, 50, 2), (0, 50, 2, 3, 30)]
    got = check_relief(d, planes, [r + (0, -1) for r in regs], quantiles=(0, 333, 500, 1000))
    for i in (8, 9, 10):
        assert got[i].tobytes() == got[7].tobytes()
    assert got[11].tobytes() == got[12].tobytes() and got["area"][7] == H * W and got["area"][0] == 1
    check_relief(to_s16(d), planes, [r + (0, -1) for r in regs])


def test_slice_edges_and_larger_frames():
    rng = np.random.default_rng(7)
    W, H = SLICE + 1, 3
    d = ramp_scene(rng, 1, H, W)
    planes = PR.fit_planes(d, [(0, 0, 0, 200, H - 1)], Q)
    assert planes["flags"][0] == PR.OK
    # one slice - 1, one slice, one slice + 1, in one row and in two; the frame
    regs = [(0, 0, 1, SLICE - 2, 1, 0, -1), (0, 0, 1, SLICE - 1, 1, 0, -1), (0, 0, 1, SLICE, 1, 0, -1),
            (0, 0, 0, SLICE // 2 - 1, 1, 0, -1), (0, 0, 0, SLICE // 2, 1, 0, -1), (0, 0, 0, W - 1, H - 1, 0, -1)]
    got = check_relief(d, planes, regs, quantiles=(0, 10, 500, 990, 1000))
    assert got["area"].tolist() == [SLICE - 1, SLICE, SLICE + 1, SLICE, SLICE + 2, 3 * W]
    # 320 x 240, and one 640 x 360 frame
    for Hs, Ws in ((240, 320), (360, 640)):
        disp, truth, _ = SR.three_surface_scene(Hs, Ws)
        planes = PR.fit_planes(disp, [(0, 0, (Hs * 3) // 4, Ws - 1, Hs - 1)], Q)  # the floor's lower part
        assert planes["flags"][0] == PR.OK
        lab = np.where(truth < 0, 255, truth).astype(np.uint8)
        got = check_relief(disp, planes, [(0, 0, 0, Ws - 1, Hs - 1, 0, -1), (0, 0, 0, Ws - 1, Hs - 1, 0, 1),
                                          (0, Ws // 4, Hs // 4, Ws // 2, Hs // 2, 0, 255)], labels=lab, band=25.0)
        assert got["n"][1] == int((truth == 1).sum()) and got["n"][0] > got["n"][1] > 0


# ---- records by flag ----
def test_records_by_flag():
    rng = np.random.default_rng(3)
    F, H, W = 3, 20, 30
    d = ramp_scene(rng, F, H, W)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (0, 0, 0, 0, H - 1), (1, 2, 2, W - 3, H - 3)], Q)
    assert planes["flags"].tolist() == [PR.OK, PR.DEGENERATE, PR.OK]
    lab = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    lab[:, :4] = 255
    whole = (0, 0, W - 1, H - 1)
    bad = [(3,) + whole + (0, -1), (-1,) + whole + (0, -1), (0, 0, 0, W, H - 1, 0, -1), (0, -1, 0, 3, 3, 0, -1),
           (0, 0, 0, 3, H, 0, -1), (0,) + whole + (0, 256), (0,) + whole + (0, -2)]
    got = check_relief(d, planes, bad, labels=lab)
    assert (got["flags"] == LR.OUT_OF_RANGE).all() and not got["area"].any()
    noplane = [(0,) + whole + (-1, -1), (0,) + whole + (3, -1), (0,) + whole + (1, 0)]
    got = check_relief(d, planes, noplane, labels=lab)
    assert (got["flags"] == LR.NO_PLANE).all() and (got["area"] == H * W).all() and not got["n_masked"].any()
    got = check_relief(d, planes[:0], [(0,) + whole + (0, -1)])  # no plane record at all
    assert got["flags"][0] == LR.NO_PLANE
    # a label without a label map is refused per record, the query beside it runs
    got = check_relief(d, planes, [(0,) + whole + (0, 1), (0,) + whole + (0, -1)])
    assert got["flags"].tolist() == [LR.OUT_OF_RANGE, LR.VALID]
    # label 255 (the unclaimed pixels), a label that matches nothing, all holes, one member
    holes = d.copy()
    holes[2] = -1.0
    holes[2, 5, 6] = 33.0
    regs = [(0,) + whole + (0, 255), (0,) + whole + (0, 77), (2, 0, 0, 4, 4, 0, -1), (2,) + whole + (0, -1),
            (2, 6, 5, 6, 5, 2, -1)]
    got = check_relief(holes, planes, regs, labels=lab, quantiles=(0, 500, 1000))
    assert got["flags"].tolist() == [LR.VALID, LR.EMPTY, LR.EMPTY, LR.VALID, LR.VALID]
    assert got["n_masked"].tolist() == [4 * W, 0, 25, H * W, 1] and got["n"].tolist()[2:] == [0, 1, 1]
    assert got["q"][3][0] == got["q"][3][1] == got["q"][3][2] == got["h_min"][3] == got["h_max"][3]
    # K = 0
    r = sdr.Ruler(Q)
    dt = torch.from_numpy(d).to(dev())
    assert tuple(r.relief_device(dt, planes, []).shape) == (0, 128) and r.relief(d, planes, []).shape == (0,)
    # K = 9 overlapping queries with different planes, labels and frames
    nine = [(f, x0, y0, x1, y1, p, l) for f, x0, y0, x1, y1, p, l in
            [(0, 0, 0, 29, 19, 0, -1), (1, 5, 5, 25, 15, 2, 0), (2, 29, 19, 0, 0, 0, 1), (0, 3, 3, 20, 18, 2, 2),
             (1, 0, 0, 29, 19, 0, 255), (2, 10, 0, 19, 19, 2, -1), (0, 0, 10, 29, 10, 0, 1), (1, 7, 7, 7, 7, 2, -1),
             (2, 0, 0, 29, 19, 1, -1)]]
    got = check_relief(d, planes, nine, labels=lab, band=3.0, quantiles=(100, 900))
    assert got["flags"][8] == LR.NO_PLANE and (got["flags"][:8] & (LR.VALID | LR.EMPTY)).all()


def test_more_queries_than_a_batch():
    """The queries run in batches of 256 through one scratch block: 600 of them, so that the second
    and third batch reuse what the first has left."""
    rng = np.random.default_rng(9)
    F, H, W = 2, 12, 17
    d = ramp_scene(rng, F, H, W)
    lab = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (1, 0, 0, W - 1, H - 1)], Q, min_inliers=3)
    K = 600
    regs = np.stack([rng.integers(0, F, K), rng.integers(0, W, K), rng.integers(0, H, K), rng.integers(0, W, K),
                     rng.integers(0, H, K), rng.integers(-1, 3, K), rng.integers(-1, 4, K)], axis=1)
    regs[::50, 1] = W  # a refused query here and there
    got = check_relief(d, planes, regs, labels=lab, quantiles=(0, 300, 700, 1000), band=4.0)
    assert {LR.VALID, LR.OUT_OF_RANGE, LR.NO_PLANE} <= set(got["flags"].tolist())
    assert (got["flags"][256:] == LR.VALID).sum() > 100


# ---- inputs ----
def test_inputs_strides_confidence_and_band():
    rng = np.random.default_rng(11)
    F, H, W = 2, 41, 67
    d = ramp_scene(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    conf[rng.random((F, H, W)) < 0.05] = np.nan
    planes = PR.fit_planes(d, [(1, 0, 0, W - 1, H - 1)], Q)
    regs = [(1, 0, 0, W - 1, H - 1, 0, -1), (0, 5, 5, 60, 30, 0, -1)]
    for disp in (d, to_s16(d)):
        a = check_relief(disp, planes, regs, conf=conf, conf_min=80.0, band=0.0)
        b = check_relief(disp, planes, regs, conf=conf, conf_min=80.0, band=float(abs(a["q"][0][1])) + 0.5)
        assert (a["n_valid"] < a["n_masked"]).all() and a["n_above"][0] + a["n_below"][0] >= b["n_above"][0] + b["n_below"][0]
        assert 0 < b["n_above"][0] + b["n_below"][0] < b["n"][0]
        check_relief(disp, planes, regs, conf=conf, conf_min=float("nan"))  # nothing passes: EMPTY
    # rows and frames padded
    pad = torch.full((F, H + 3, W + 9), -7.0, dtype=torch.float32, device=dev())
    pad[:, :H, :W] = torch.from_numpy(d).to(dev())
    view = pad[:, :H, :W]
    assert view.stride(1) == W + 9 and view.stride(0) == (H + 3) * (W + 9)
    r = sdr.Ruler(Q)
    LR.assert_reliefs_equal(records(r.relief_device(view, planes, regs)), LR.relief(d, planes, regs, Q))
    wide = np.full((F, H, W + 5), np.nan, np.float32)  # a strided host map
    wide[:, :, :W] = d
    LR.assert_reliefs_equal(r.relief(wide[:, :, :W], planes, regs), LR.relief(d, planes, regs, Q))


def test_reference_calibration_with_fitted_planes():
    """The real pipeline: the reference calibration's Q (tests/golden/stereo.yaml), planes fitted on
    the device, the relief of each found plane's label above each found plane."""
    from stereo_depth_ruler_amd.config import StereoConfiguration

    cfg = StereoConfiguration()
    assert cfg.loadFromFile(os.path.join(ROOT, "tests", "golden", "stereo.yaml"))
    Qc = np.asarray(cfg.Q, np.float64).reshape(4, 4)
    disp, _, _ = SR.three_surface_scene(120, 160)
    r = sdr.Ruler(Qc)
    planes, lab = r.find_planes(torch.from_numpy(disp).to(dev()), None, hypotheses=128, min_inliers=300, labels=True)
    assert len(planes) == 3
    regs = [(0, 0, 0, 159, 119, p, l) for p in range(3) for l in (0, 1, 2, -1)]
    got = check_relief(disp, planes, regs, labels=lab, Qm=Qc, band=5.0)
    assert (got["flags"] == LR.VALID).all()
    for p in range(3):  # a label's pixels are the plane's inliers, all of them valid
        assert got["n_valid"][4 * p + p] == got["n_masked"][4 * p + p] == planes["n_inliers"][p]


# ---- chaining and layers ----
def test_search_and_relief_chain_on_one_stream():
    disp, _, _ = SR.three_surface_scene(60, 80)
    r = sdr.Ruler(Q)
    d = torch.from_numpy(disp).to(dev())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(hypotheses=128, min_inliers=200, max_planes=4)
    regs = [(0, 0, 0, 79, 59, 0, 1), (0, 0, 0, 79, 59, 0, 2), (0, 0, 0, 79, 59, 1, 0), (0, 10, 10, 70, 50, 3, -1)]
    out = r.find_planes_device(d, None, stream=side, labels=True, **kw)
    rel = r.relief_device(d, out[0], regs, labels=out[3], stream=side, band=10.0)  # no synchronisation between
    side.synchronize()
    want = SR.find_planes(disp, (0, 0, 0, 79, 59), Q, **kw)
    assert want[1] == 3
    PR.assert_planes_equal(out[0].cpu().numpy().reshape(-1).view(PLANE_DTYPE), want[0])
    got = records(rel)
    LR.assert_reliefs_equal(got, LR.relief(disp, want[0], regs, Q, labels=want[3], band=10.0))
    assert got["flags"].tolist() == [LR.VALID] * 3 + [LR.NO_PLANE]  # the record past the count is not PLANE_OK


def test_host_abi_and_tensor_forms():
    rng = np.random.default_rng(14)
    F, H, W = 2, 27, 45
    d = ramp_scene(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    lab = rng.integers(0, 4, (F, H, W)).astype(np.uint8)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (1, 0, 0, W - 1, H - 1)], Q, conf=conf, conf_min=30.0)
    regs = [(1, 2, 1, W - 1, H - 2, 1, 3), (0, 0, 0, W - 1, H - 1, 0, -1), (1, 0, 0, 9, 9, 0, 2)]
    kw = dict(quantiles=(10, 990, 500, 500), band=2.0)
    want = LR.relief(d, planes, regs, Q, labels=lab, conf=conf, conf_min=30.0, **kw)
    r = sdr.Ruler(Q, conf_min=30.0)
    LR.assert_reliefs_equal(r.relief(d, planes, regs, labels=lab, conf=conf, **kw), want)       # host ABI
    LR.assert_reliefs_equal(r.relief(to_s16(d), planes, regs, labels=lab, conf=conf, **kw),
                            LR.relief(to_s16(d), planes, regs, Q, labels=lab, conf=conf, conf_min=30.0, **kw))
    t = lambda a: torch.from_numpy(a).to(dev())  # noqa: E731
    LR.assert_reliefs_equal(r.relief(t(d), planes, regs, labels=t(lab), conf=t(conf), **kw), want)  # tensors
    pt = t(np.ascontiguousarray(planes).view(np.uint8).reshape(-1, 128))
    qt = t(as_relief_queries(regs))
    LR.assert_reliefs_equal(records(r.relief_device(t(d), pt, qt, labels=lab, conf=t(conf), **kw)), want)
    LR.assert_reliefs_equal(r.relief(d, pt, regs, labels=t(lab), conf=conf, **kw), want)  # device planes, host maps
    one = sdr.Ruler(Q).relief(d[0], planes, (0, 0, 0, W - 1, H - 1))  # an (H, W) map, one tuple, the defaults
    LR.assert_reliefs_equal(one, LR.relief(d[:1], planes, [(0, 0, 0, W - 1, H - 1)], Q))


def test_live_loop_relief_on_the_frame_stream():
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
    loop = LiveLoop(rect, Q, 1, ruler=dict(radius=1, min_count=2, conf_min=100.0))
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(max_planes=3, hypotheses=96, iterations=2, inlier_px=2.0, min_inliers=30)
    w2, h2 = loop.w2, loop.h2
    regs = [(0, 0, 0, w2 - 1, h2 - 1, 0, 0), (0, 0, 0, w2 - 1, h2 - 1, 0, -1), (0, 150, 30, 60, 10, 1, 255)]
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        planes, count, _, lab = loop.find_planes(None, side, labels=True, **kw)
        rel = loop.relief(planes, regs, side, labels=lab, quantiles=(250, 750), band=50.0)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    pl = planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    got = records(rel)
    LR.assert_reliefs_equal(got, LR.relief(disp, pl, regs, Q, labels=lab.cpu().numpy(), conf=conf,
                                           quantiles=(250, 750), band=50.0, min_disp=loop.ruler.min_disp,
                                           conf_min=100.0))
    assert int(count.cpu()[0]) >= 1 and got["flags"][0] == LR.VALID and got["n_valid"][0] == pl["n_inliers"][0]
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()


def test_cpp_facade_relief(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::relief gives Python's records as bytes
    (tests/cpp/facade_relief.cpp)."""
    exe = tmp_path / "facade_relief"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_relief.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    disp, _, _ = SR.three_surface_scene(45, 61)
    rng = np.random.default_rng(15)
    H, W = disp.shape[1:]
    conf = rng.uniform(0, 255, (1, H, W)).astype(np.float32)
    disp[0].tofile(tmp_path / "disp.bin")
    conf[0].tofile(tmp_path / "conf.bin")
    np.asarray(Q, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), "4", "90", "12345", str(tmp_path)], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    r = sdr.Ruler(Q, conf_min=10.0)
    planes, lab = r.find_planes(disp, None, conf=conf, max_planes=4, hypotheses=90, seed=12345, iterations=2,
                                inlier_px=1.5, min_inliers=6, labels=True)
    n = len(planes)
    assert n >= 2 and f"planes={n} reliefs={2 * n}" in res.stdout
    assert "single_equal=1" in res.stdout and "bad_permille_code=-1" in res.stdout
    assert (tmp_path / "planes.bin").read_bytes() == planes.tobytes()
    assert (tmp_path / "labels.bin").read_bytes() == lab.tobytes()
    regs = [q for i in range(n) for q in ((0, W - 1, 0, 0, H - 1, 0, i), (0, 0, 0, W - 1, H - 1, i, -1))]
    want = LR.relief(disp, planes, regs, Q, labels=lab, conf=conf, conf_min=10.0, quantiles=(0, 250, 500, 1000),
                     band=2.5)
    assert (tmp_path / "relief.bin").read_bytes() == want.tobytes()


# ---- hypothesis ----
@settings(max_examples=hyp_examples(20), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(3, 96), W=st.integers(3, 96), with_conf=st.booleans(), with_labels=st.booleans(),
       i16=st.booleans(), nq=st.integers(0, 8), seed=st.integers(0, 2 ** 32 - 1))
def test_hypothesis_random_scenes(H, W, with_conf, with_labels, i16, nq, seed):
    rng = np.random.default_rng(seed)
    F = int(rng.integers(1, 3))
    d = ramp_scene(rng, F, H, W)
    weird = rng.random((F, H, W)) < 0.03
    d[weird] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2048.0], np.float32), int(weird.sum()))
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (F - 1, 0, 0, W // 2, H // 2)], Q, min_inliers=3)
    disp = to_s16(d) if i16 else d
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32) if with_conf else None
    lab = rng.choice(np.array([0, 1, 2, 255], np.uint8), (F, H, W)) if with_labels else None
    regs = []
    for _ in range(int(rng.integers(1, 5))):
        reg = [int(rng.integers(0, F)), int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, W)),
               int(rng.integers(0, H)), int(rng.integers(0, 2)), int(rng.choice([-1, -1, 0, 1, 255]))]
        if rng.random() < 0.4:
            reg[1:5] = [0, 0, W - 1, H - 1]
        if rng.random() < 0.15:
            reg[int(rng.integers(0, 6))] = int(rng.choice([-1, 100]))
        regs.append(tuple(reg))
    check_relief(disp, planes, regs, labels=lab, conf=conf, conf_min=float(rng.uniform(0, 200)),
                 quantiles=tuple(int(v) for v in rng.integers(0, 1001, nq)), band=float(rng.uniform(0, 40)))
