"""GPU: the ruler (sdr_measure_disp*, sdr_measure_xyz*, csrc/sdr_ruler.hip) through every layer,
exact against its numpy restatement (tests/ruler_ref.py): float fields as bit patterns, distance as
a double bit pattern, z_min / z_max / max_dz as values (ruler_ref.assert_records_equal)."""
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

import ruler_ref as RR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import _lib  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import MEASUREMENT_DTYPE, as_segments  # noqa: E402
from stereo_depth_ruler_amd.sgbm import _Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q
SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def make_map(rng, F, H, W, holes=0.2, weird=0.03):
    """Disparities in [1, 80) px on the 1/16 grid, `holes` of them -1, a few NaN / inf / 0 / -0."""
    d = (np.floor(rng.uniform(1, 80, (F, H, W)) * 16) / 16).astype(np.float32)
    u = rng.random((F, H, W))
    d[u < holes] = -1.0
    pick = (u >= holes) & (u < holes + weird)
    d[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32), int(pick.sum()))
    return d


def random_segments(rng, K, F, H, W):
    return np.stack([rng.integers(0, F, K), rng.integers(0, W, K), rng.integers(0, H, K),
                     rng.integers(0, W, K), rng.integers(0, H, K)], axis=1).astype(np.int32)


def run_device(disp, segs, conf=None, profile_cap=None, **kw):
    """Ruler(**kw) on uploaded maps -> (records, profile or None)."""
    r = sdr.Ruler(Q, **kw)
    d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    rec, prof = r.measure_device(d, segs, conf=c, profile_cap=profile_cap)
    torch.cuda.synchronize()
    rec = rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE)
    return rec, (prof.cpu().numpy() if prof is not None else None)


def check_against_ref(disp, segs, conf=None, **kw):
    """Device result == numpy restatement, records and (with profile) every profile row."""
    segs = as_segments(segs)
    got, prof = run_device(disp, segs, conf=conf, **kw)
    cap = prof.shape[1] if prof is not None else 0
    want_prof = np.full((len(segs), cap, 4), np.nan, np.float32) if prof is not None else None
    want = RR.measure(disp, segs, Q, conf=conf, radius=kw.get("radius", 0), min_count=kw.get("min_count", 1),
                      min_disp=kw.get("min_disp", -1.0), conf_min=kw.get("conf_min", 0.0),
                      profile=kw.get("profile", False), profile_cap=cap, profile_buf=want_prof)
    RR.assert_records_equal(got, want)
    if prof is not None:
        RR.assert_profile_equal(prof, want_prof)
    return got, prof


# ---- borders ----
@pytest.mark.parametrize("H, W", [(24, 40), (5, 7)])  # the second is smaller than the 9x9 window
def test_borders(H, W):
    rng = np.random.default_rng(H)
    disp = make_map(rng, 1, H, W)
    xs, ys = (0, W // 2, W - 1), (0, H // 2, H - 1)
    pts = [(x, y) for x in xs for y in ys]  # the four corners, the four edge centres, the middle
    segs = [(0, a[0], a[1], b[0], b[1]) for a in pts for b in pts]
    for r in (4, 1):
        got, _ = check_against_ref(disp, segs, radius=r, min_count=1, profile=True)
        assert (got["flags"] & RR.OUT_OF_RANGE == 0).all()
    # the window is clipped, never wrapped: the corner's count is at most the clipped area
    got, _ = run_device(disp, [(0, 0, 0, W - 1, H - 1)], radius=4)
    assert got["n0"][0] <= min(5, H) * min(5, W) and got["n1"][0] <= min(5, H) * min(5, W)


# ---- validity ----
def test_validity_plants():
    H, W = 9, 30
    d = np.full((1, H, W), -1.0, np.float32)
    c = np.full((1, H, W), 100.0, np.float32)
    # windows (r = 1) centred at y = 4: x = 2 none valid, 6 one, 10 two, 14 non-finite only,
    # 18 values equal to min_disp, 22 confidences around conf_min, 26 a -0.0 and a 0
    d[0, 4, 6] = 33.5
    d[0, 3, 9], d[0, 5, 11] = 20.0, 60.0
    d[0, 3:6, 13:16] = np.array([[np.nan, np.inf, -np.inf]] * 3, np.float32)
    d[0, 3:6, 17:20] = 7.0
    d[0, 4, 21], d[0, 4, 22], d[0, 4, 23] = 30.0, 31.0, 32.0
    c[0, 4, 21], c[0, 4, 22], c[0, 4, 23] = 50.0, np.float32(49.999), np.nan
    d[0, 4, 25], d[0, 4, 27] = -0.0, 0.0
    cx = (2, 6, 10, 14, 18, 22, 26)
    segs = [(0, a, 4, b, 4) for a in cx for b in cx]
    for mc in (1, 2, 3):
        got, _ = check_against_ref(d, segs, conf=c, radius=1, min_count=mc, min_disp=7.0, conf_min=50.0,
                                   profile=True)
    got, _ = check_against_ref(d, segs, conf=c, radius=1, min_count=1, min_disp=-1.0, conf_min=50.0)
    by = {(s[1], s[3]): g for s, g in zip(segs, got)}
    assert by[(2, 2)]["n0"] == 0 and by[(6, 6)]["n0"] == 1 and by[(10, 10)]["n0"] == 2 and by[(14, 14)]["n0"] == 0
    assert by[(18, 18)]["n0"] == 9 and by[(22, 22)]["n0"] == 1 and by[(22, 22)]["d0"] == 30.0
    assert by[(6, 10)]["flags"] == 3 and by[(10, 10)]["d0"] == 20.0  # the lower of two
    # d = 0 with REFERENCE_Q: w = 0, the point is not finite, so it is invalid and the distance NaN
    z = by[(26, 6)]
    assert z["n0"] == 2 and z["d0"] == 0 and z["flags"] == RR.P1_VALID and np.isnan(z["distance"])
    # conf_min plays no part without a confidence map, even a NaN one; with a map it rejects all
    gn, _ = check_against_ref(d, segs, radius=1, min_count=1, conf_min=float("nan"))
    assert {(s[1], s[3]): g for s, g in zip(segs, gn)}[(6, 10)]["flags"] == 3
    gn, _ = check_against_ref(d, segs, conf=c, radius=1, min_count=1, conf_min=float("nan"))
    assert (gn["n0"] == 0).all()
    got7, _ = check_against_ref(d, segs, radius=1, min_count=1, min_disp=7.0)
    assert {(s[1], s[3]): g for s, g in zip(segs, got7)}[(18, 18)]["n0"] == 0  # d == min_disp is rejected


def test_computed_nans_are_canonical():
    """0 * inf in the reprojection (x = 0, d = 0, Q[0][3] = 0) makes a NaN whose sign depends on
    the machine; the record holds the canonical quiet NaN, bit for bit."""
    Qc = np.array(Q)
    Qc[0, 3] = 0.0
    d = np.zeros((1, 3, 3), np.float32)
    d[0, 2, 2] = 30.0
    segs = as_segments([(0, 0, 0, 1, 1), (0, 0, 1, 2, 2), (0, 2, 2, 0, 2)])
    r = sdr.Ruler(Qc, profile=True)
    rec, prof = r.measure_device(torch.from_numpy(d).to(dev()), segs)
    torch.cuda.synchronize()
    got = rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE)
    want_prof = np.full(tuple(prof.shape), np.nan, np.float32)
    want = RR.measure(d, segs, Qc, profile=True, profile_cap=prof.shape[1], profile_buf=want_prof)
    RR.assert_records_equal(got, want)
    RR.assert_profile_equal(prof.cpu().numpy(), want_prof)
    bits = np.ascontiguousarray(got["p0"]).view(np.uint32)
    assert np.isnan(got["p0"][0][0]) and bits[0][0] == 0x7FC00000
    assert np.array_equal(np.ascontiguousarray(r.measure(d, segs)[0]["p0"]).view(np.uint32), bits)  # host ABI


# ---- profile ----
def test_profile_segments():
    rng = np.random.default_rng(3)
    H, W = 40, 70
    disp = make_map(rng, 1, H, W, holes=0.3)
    segs = [(0, 5, 5, 5, 5),                       # zero length
            (0, 3, 7, 60, 7), (0, 60, 7, 3, 7),    # horizontal
            (0, 9, 2, 9, 38), (0, 9, 38, 9, 2),    # vertical
            (0, 2, 2, 36, 36), (0, 36, 36, 2, 2),  # diagonal and reversed
            (0, 36, 2, 2, 36), (0, 2, 36, 36, 2),  # anti-diagonal and reversed
            (0, 10, 0, 14, 39), (0, 14, 39, 10, 0),  # steep
            (0, 0, 20, 69, 17), (0, 69, 17, 0, 20),  # shallow
            (0, 0, 0, 69, 39), (0, 1, 0, 3, 1)]
    for r, mc in ((0, 1), (2, 3)):
        got, prof = check_against_ref(disp, segs, radius=r, min_count=mc, profile=True)
        assert got["path_samples"].tolist() == [max(abs(s[3] - s[1]), abs(s[4] - s[2])) + 1 for s in segs]
        # swapping the endpoints walks the same pixels in reverse
        for a, b in ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12)):
            for k in ("path_valid", "max_gap", "z_min", "z_max", "max_dz", "distance"):
                assert np.array_equal(got[k][a], got[k][b], equal_nan=True), (k, a)
            n = got["path_samples"][a]
            assert np.array_equal(prof[a, :n], prof[b, :n][::-1], equal_nan=True)


def test_profile_long_row_and_gaps():
    """701 samples cross the block's 512-sample chunk; invalid runs sit at the start, in the middle,
    across the chunk boundary and at the end, and consecutive valid samples straddle the boundary."""
    rng = np.random.default_rng(4)
    disp = make_map(rng, 1, 6, 701, holes=0.1, weird=0.0)
    disp[0, 2, :37] = -1.0
    disp[0, 2, 240:300] = -1.0
    disp[0, 2, 500:523] = -1.0
    disp[0, 2, 690:] = -1.0
    disp[0, 4, :] = -1.0
    disp[0, 4, 511], disp[0, 4, 512], disp[0, 4, 600] = 10.0, 30.0, 20.0
    disp[0, 5, :] = -1.0
    segs = [(0, 0, 2, 700, 2), (0, 700, 2, 0, 2), (0, 0, 4, 700, 4), (0, 0, 5, 700, 5), (0, 0, 0, 700, 5),
            (0, 100, 2, 620, 2)]
    got, _ = check_against_ref(disp, segs, radius=0, min_count=1, profile=True)
    assert got["max_gap"][0] >= 60 and got["max_gap"][2] == 511 and got["path_valid"][2] == 3
    assert got["path_valid"][3] == 0 and got["max_gap"][3] == 701 and np.isnan(got["z_min"][3])
    check_against_ref(disp, segs[:3], radius=2, min_count=2, profile=True)


def test_profile_cap_and_sentinel():
    rng = np.random.default_rng(6)
    disp = make_map(rng, 1, 12, 50)
    segs = as_segments([(0, 0, 3, 49, 3), (0, 4, 4, 9, 6), (0, 7, 7, 7, 7), (0, 60, 0, 1, 1), (0, 0, 0, 29, 11)])
    cap = 30
    r = sdr.Ruler(Q, radius=1, min_count=2, profile=True)
    buf = torch.full((len(segs), cap, 4), float(SENTINEL), dtype=torch.float32, device=dev())
    rec, prof = r.measure_device(torch.from_numpy(disp).to(dev()), segs, profile_out=buf)
    torch.cuda.synchronize()
    assert prof is buf
    got = rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE)
    want_buf = np.full((len(segs), cap, 4), SENTINEL, np.float32)
    want = RR.measure(disp, segs, Q, radius=1, min_count=2, profile=True, profile_cap=cap, profile_buf=want_buf)
    RR.assert_records_equal(got, want)
    RR.assert_profile_equal(buf.cpu().numpy(), want_buf)
    assert (want_buf[0] != SENTINEL).all() and (want_buf[1, 6:] == SENTINEL).all()
    assert (want_buf[3] == SENTINEL).all()  # out of range: nothing written
    assert [int(f) & RR.TRUNCATED for f in got["flags"]] == [RR.TRUNCATED, 0, 0, 0, 0]
    # a profile without a buffer still fills the record, and never sets the truncated bit
    L = lib()
    p = _lib.RulerParams(1, 2, -1.0, 0.0, 1, 0)
    out = torch.zeros((len(segs), 80), dtype=torch.uint8, device=dev())
    sd = torch.from_numpy(segs).to(dev())
    dd = torch.from_numpy(disp).to(dev())
    check(L.sdr_measure_disp_device(dd.data_ptr(), 0, 50, 600, 50, 12, 1, None, _Q(Q), ctypes.byref(p),
                                    sd.data_ptr(), len(segs), out.data_ptr(), None, None))
    torch.cuda.synchronize()
    nobuf = out.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE)
    want["flags"] &= ~np.uint32(RR.TRUNCATED)
    RR.assert_records_equal(nobuf, want)
    # a buffer with profile_cap 0 has no rows and counts as no buffer, in the device and host ABI
    check(L.sdr_measure_disp_device(dd.data_ptr(), 0, 50, 600, 50, 12, 1, None, _Q(Q), ctypes.byref(p),
                                    sd.data_ptr(), len(segs), out.data_ptr(), buf.data_ptr(), None))
    torch.cuda.synchronize()
    RR.assert_records_equal(out.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE), want)
    hrec = np.zeros(len(segs), MEASUREMENT_DTYPE)
    hbuf = np.full(4, SENTINEL, np.float32)
    check(L.sdr_measure_disp(disp.ctypes.data, 0, 50, 600, 50, 12, 1, None, _Q(Q), ctypes.byref(p),
                             segs.ctypes.data, len(segs), hrec.ctypes.data, hbuf.ctypes.data))
    RR.assert_records_equal(hrec, want)
    assert (hbuf == SENTINEL).all()


# ---- batches ----
def test_batch_frames_strides_and_out_of_range():
    rng = np.random.default_rng(7)
    F, H, W = 3, 20, 33
    disp = make_map(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    segs = random_segments(rng, 300, F, H, W)
    bad = [(3, 0, 0, 1, 1), (-1, 0, 0, 1, 1), (0, W, 0, 1, 1), (1, 0, H, 1, 1), (2, 1, 1, -1, 1), (0, 1, 1, 1, 2 ** 30),
           (2 ** 31 - 1, 0, 0, 0, 0), (0, -2 ** 31, 0, 0, 0)]
    segs[10:10 + len(bad)] = np.array(bad, np.int64).astype(np.int32)
    got, _ = check_against_ref(disp, segs, conf=conf, radius=2, min_count=3, conf_min=40.0, profile=True)
    assert (got["flags"][10:18] == RR.OUT_OF_RANGE).all() and (got["flags"][:10] & RR.OUT_OF_RANGE == 0).all()
    assert len(set(segs[:, 0].tolist())) >= 3
    one, _ = check_against_ref(disp, segs[40:41], conf=conf, radius=2, min_count=3, conf_min=40.0, profile=True)  # K = 1
    RR.assert_records_equal(one, got[40:41])
    # rows padded to a stride larger than W: the same records
    pad = torch.full((F, H, W + 5), float("nan"), dtype=torch.float32, device=dev())
    pad[:, :, :W] = torch.from_numpy(disp).to(dev())
    view = pad[:, :, :W]
    assert view.stride(1) == W + 5
    r = sdr.Ruler(Q, radius=2, min_count=3, conf_min=40.0, profile=True)
    rec, _ = r.measure_device(view, segs, conf=torch.from_numpy(conf).to(dev()))
    torch.cuda.synchronize()
    RR.assert_records_equal(rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE), got)


def heavy_work(stream, x, n=150):
    """A few tens of milliseconds of work on `stream`, and an event recorded behind it."""
    with torch.cuda.stream(stream):
        for _ in range(n):
            x.mul_(1.0)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def test_host_segments_do_not_wait_for_the_stream():
    """measure_device returns while the stream's earlier work is still running, with host segments
    (what a mouse click produces) as with device ones, and through a copy of a strided input."""
    rng = np.random.default_rng(15)
    F, H, W = 2, 30, 44
    disp = make_map(rng, F, H, W)
    segs = random_segments(rng, 20, F, H, W)
    want = RR.measure(disp, segs, Q, radius=1, min_count=2, profile=True)
    r = sdr.Ruler(Q, radius=1, min_count=2, profile=True)
    dd = torch.from_numpy(disp).to(dev())
    tr = torch.from_numpy(np.ascontiguousarray(disp.transpose(0, 2, 1))).to(dev()).transpose(1, 2)  # stride(2) != 1
    x = torch.zeros(64 << 20, dtype=torch.float32, device=dev())
    side = torch.cuda.Stream(dev())
    r.measure_device(dd, segs, stream=side)  # first use: staging and kernels are set up
    x.mul_(1.0)
    torch.cuda.synchronize()
    for d_in, s_in in ((dd, segs), (dd, [tuple(s) for s in segs.tolist()]), (tr, segs),
                       (dd, torch.from_numpy(segs).to(dev()))):
        busy = heavy_work(side, x)
        rec, _ = r.measure_device(d_in, s_in, stream=side, profile_cap=0)
        returned_early = not busy.query()
        torch.cuda.synchronize()
        assert returned_early, "measure_device waited for the stream's earlier work"
        RR.assert_records_equal(rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE), want)
    # more uploads in flight than the staging ring has slots: still the right records
    busy = heavy_work(side, x, 20)
    recs = [r.measure_device(dd, segs[i:i + 1], stream=side, profile_cap=0)[0] for i in range(20)]
    torch.cuda.synchronize()
    got = np.concatenate([t.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE) for t in recs])
    RR.assert_records_equal(got, want)


def test_no_segments_writes_nothing():
    disp = torch.zeros((2, 4, 4), dtype=torch.float32, device=dev())
    out = torch.full((4, 80), 0x5A, dtype=torch.uint8, device=dev())
    prof = torch.full((4, 3, 4), float(SENTINEL), dtype=torch.float32, device=dev())
    p = _lib.RulerParams(1, 1, -1.0, 0.0, 1, 3)
    check(lib().sdr_measure_disp_device(disp.data_ptr(), 0, 4, 16, 4, 4, 2, None, _Q(Q), ctypes.byref(p), None, 0,
                                        out.data_ptr(), prof.data_ptr(), None))
    xyz = torch.zeros((2, 4, 4, 3), dtype=torch.float32, device=dev())
    check(lib().sdr_measure_xyz_device(xyz.data_ptr(), 12, 48, 4, 4, 2, None, 0, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert (out == 0x5A).all() and (prof == float(SENTINEL)).all()
    r = sdr.Ruler(Q, profile=True)
    rec, pr = r.measure(disp, [])
    assert rec.shape == (0,) and pr.shape[0] == 0
    assert r.measure_xyz(xyz, []).shape == (0,)


# ---- int16 input ----
def test_int16_input():
    """StereoSGBM's CV_16S map with a negative minDisparity: the invalid value is (minD - 1) * 16."""
    rng = np.random.default_rng(8)
    F, H, W, minD = 2, 18, 41, -20
    d16 = rng.integers(minD * 16, (minD + 64) * 16, (F, H, W)).astype(np.int16)
    d16[rng.random((F, H, W)) < 0.25] = (minD - 1) * 16
    segs = random_segments(rng, 60, F, H, W)
    for r, mc in ((0, 1), (3, 5)):
        got, _ = check_against_ref(d16, segs, radius=r, min_count=mc, min_disp=float(minD - 1), profile=True)
    assert (got["d0"][np.isfinite(got["d0"])] > minD - 1).all()
    # the float map of the same values gives the same records
    f32 = d16.astype(np.float32) * np.float32(0.0625)
    same, _ = run_device(f32, segs, radius=3, min_count=5, min_disp=float(minD - 1), profile=True)
    RR.assert_records_equal(same, got)


# ---- identity with reprojectImageTo3D and the XYZ mode ----
def test_identity_with_reproject_and_xyz_mode():
    rng = np.random.default_rng(9)
    F, H, W = 2, 21, 37
    disp = make_map(rng, F, H, W, holes=0.15)
    segs = random_segments(rng, 120, F, H, W)
    segs[5] = (0, W, 0, 0, 0)
    dd = torch.from_numpy(disp).to(dev())
    xyz = sdr.reprojectImageTo3D(dd, Q, False)
    torch.cuda.synchronize()
    xyz_h = xyz.cpu().numpy()
    got, _ = check_against_ref(disp, segs, radius=0, min_count=1)
    r = sdr.Ruler(Q)
    gx = r.measure_xyz(xyz, segs)
    RR.assert_records_equal(gx, RR.measure_xyz(xyz_h, segs))
    RR.assert_records_equal(r.measure_xyz(xyz_h, segs), gx)  # the host ABI
    assert gx["flags"][5] == RR.OUT_OF_RANGE
    checked = 0
    for k, (f, x0, y0, x1, y1) in enumerate(segs.tolist()):
        if k == 5:
            continue
        for e, (x, y) in enumerate(((x0, y0), (x1, y1))):
            if got["flags"][k] & (1 << e):  # a valid point is the pixel of reprojectImageTo3D, bit for bit
                assert np.array_equal(got["p%d" % e][k].view(np.uint32), xyz_h[f, y, x].view(np.uint32))
                assert np.array_equal(gx["p%d" % e][k].view(np.uint32), xyz_h[f, y, x].view(np.uint32))
        if got["flags"][k] & 3 == 3:
            assert got["distance"][k].view(np.uint64) == gx["distance"][k].view(np.uint64)
            checked += 1
        assert bool(gx["flags"][k] & 1) == bool(np.isfinite(xyz_h[f, y0, x0]).all())
    assert checked >= 40
    # without the validity gate the XYZ mode reports what the reference prints: inf or NaN
    assert not np.isfinite(gx["distance"][(gx["flags"] & 3) != 3]).any()


# ---- hypothesis ----
@settings(max_examples=hyp_examples(40), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(1, 40), W=st.integers(1, 90), radius=st.integers(0, 4), min_count=st.integers(1, 9),
       with_conf=st.booleans(), profile=st.booleans(), i16=st.booleans(), seed=st.integers(0, 2 ** 31 - 1))
def test_hypothesis_random_maps(H, W, radius, min_count, with_conf, profile, i16, seed):
    rng = np.random.default_rng(seed)
    F = int(rng.integers(1, 3))
    disp = make_map(rng, F, H, W, holes=float(rng.uniform(0, 0.6)))
    if i16:
        disp = np.nan_to_num(disp * 16, nan=-16.0, posinf=32767.0, neginf=-32768.0).astype(np.int16)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32) if with_conf else None
    segs = random_segments(rng, int(rng.integers(1, 9)), F, H, W)
    if rng.random() < 0.3:
        segs[0, int(rng.integers(0, 5))] = int(rng.choice([-1, 100]))
    check_against_ref(disp, segs, conf=conf, radius=radius, min_count=min_count,
                      conf_min=float(rng.uniform(0, 200)), profile=profile)


# ---- the host ABI ----
def test_host_abi_equals_device_abi():
    rng = np.random.default_rng(11)
    F, H, W = 2, 17, 45
    disp = make_map(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    segs = random_segments(rng, 50, F, H, W)
    segs[3] = (F, 0, 0, 0, 0)
    kw = dict(radius=2, min_count=2, conf_min=30.0, profile=True)
    got, prof = check_against_ref(disp, segs, conf=conf, **kw)
    hrec, hprof = sdr.Ruler(Q, **kw).measure(disp, segs, conf=conf)
    RR.assert_records_equal(hrec, got)
    RR.assert_profile_equal(hprof, prof)
    # a strided host map (rows of W + 3) and int16
    wide = np.full((F, H, W + 3), np.nan, np.float32)
    wide[:, :, :W] = disp
    srec, _ = sdr.Ruler(Q, **kw).measure(wide[:, :, :W], segs, conf=conf)
    RR.assert_records_equal(srec, got)
    d16 = rng.integers(-16, 1200, (H, W)).astype(np.int16)
    s2 = segs[segs[:, 0] == 0]
    a = sdr.Ruler(Q, radius=1).measure(d16, s2)
    b, _ = run_device(d16[None], s2, radius=1)
    RR.assert_records_equal(a, b)
    # the tensor form of measure() downloads the same records
    t, tp = sdr.Ruler(Q, **kw).measure(torch.from_numpy(disp).to(dev()), segs, conf=torch.from_numpy(conf).to(dev()))
    RR.assert_records_equal(t, got)
    RR.assert_profile_equal(tp, prof)


# ---- end to end ----
@pytest.fixture(scope="module")
def sbs():
    return S.sbs_bgr_frame(96, 400, 80, seed=21)  # half size 48 x 200, as test_gpu_census's class path


def test_stereo_disparity_ruler(sbs):
    W = sbs.shape[1] // 2
    sd = sdr.StereoDisparity(Q)
    out = sd.computeDisparity(np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:]))
    ruler = sd.ruler(radius=2, min_count=3, conf_min=128.0, profile=True)
    assert ruler.min_disp == -1.0 and np.array_equal(ruler.Q, Q)
    rng = np.random.default_rng(12)
    segs = random_segments(rng, 24, 1, *out.shape)
    got, prof = ruler.measure(out, segs, conf=sd.conf_map)
    want_prof = np.full_like(prof, np.nan)
    want = RR.measure(out[None], segs, Q, conf=sd.conf_map[None], radius=2, min_count=3, min_disp=-1.0,
                      conf_min=128.0, profile=True, profile_cap=prof.shape[1], profile_buf=want_prof)
    RR.assert_records_equal(got, want)
    RR.assert_profile_equal(prof, want_prof)
    assert ((got["flags"] & 3) == 3).any()  # the scene has measurable points
    # radius 0 on the same map is computeDepth's pixel
    depth = sd.computeDepth(out)
    r0 = sd.ruler().measure(out, segs)
    for k, (_, x0, y0, x1, y1) in enumerate(segs.tolist()):
        if r0["flags"][k] & 1:
            assert np.array_equal(r0["p0"][k].view(np.uint32), depth[y0, x0].view(np.uint32))


def test_live_loop_measure_on_the_frame_stream(sbs):
    """LiveLoop(ruler=...): measure() is enqueued right after the frame on the frame's stream, with
    no synchronise in between; the records equal the restatement on the downloaded disp and conf,
    and the loop's other outputs equal those of a loop without the ruler."""
    from stereo_depth_ruler_amd.pipeline import LiveLoop
    from stereo_depth_ruler_amd.rectify import StereoRectifier

    H, W = sbs.shape[0], sbs.shape[1] // 2
    K = np.array([[700.0, 0, W / 2], [0, 700.0, H / 2], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    cfg = types.SimpleNamespace(imageSize=(W, H), cameraMatrixLeft=K, cameraMatrixRight=K, distCoeffsLeft=None,
                                distCoeffsRight=None, R1=np.eye(3), R2=np.eye(3), P1=P, P2=P)
    rect = StereoRectifier(cfg)
    frame = torch.from_numpy(sbs[None]).to(dev())
    plain = LiveLoop(rect, Q, 1)
    s0 = torch.cuda.current_stream(dev())
    plain.enqueue(frame, s0)
    torch.cuda.synchronize()
    assert plain.ruler is None and plain.conf is None
    with pytest.raises(RuntimeError):
        plain.measure([(0, 0, 1, 1)], s0)
    loop = LiveLoop(rect, Q, 1, ruler=dict(radius=1, min_count=2, conf_min=100.0, profile=True))
    assert loop.ruler.min_disp == -1.0
    rng = np.random.default_rng(13)
    segs = random_segments(rng, 16, 1, loop.h2, loop.w2)
    side = torch.cuda.Stream(dev())
    side.wait_stream(s0)
    loop.enqueue(frame, s0)  # sizes the loop's scratch
    torch.cuda.synchronize()
    x = torch.zeros(64 << 20, dtype=torch.float32, device=dev())
    x.mul_(1.0)
    torch.cuda.synchronize()
    busy = heavy_work(side, x)
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        rec, prof = loop.measure(segs, side)  # host segments; no synchronise since the enqueue
    returned_early = not busy.query()
    torch.cuda.synchronize()
    assert returned_early, "the frame and its measurement waited for the stream's earlier work"
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    assert torch.equal(loop.filtered, plain.filtered)
    assert torch.equal(loop.depth.view(torch.int32), plain.depth.view(torch.int32))
    got = rec.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE)
    want_prof = np.full(tuple(prof.shape), np.nan, np.float32)
    want = RR.measure(disp, segs, Q, conf=conf, radius=1, min_count=2, min_disp=-1.0, conf_min=100.0,
                      profile=True, profile_cap=prof.shape[1], profile_buf=want_prof)
    RR.assert_records_equal(got, want)
    RR.assert_profile_equal(prof.cpu().numpy(), want_prof)
    assert ((got["flags"] & 3) == 3).any()
    check(lib().sdr_rectifier_reset_stream(rect._h))
    plain.close()
    loop.close()


# ---- the C++ facade ----
def test_cpp_facade_ruler(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler and sdr::MeasurementLog give Python's records, profile
    and CSV bytes (tests/cpp/facade_ruler.cpp)."""
    exe = tmp_path / "facade_ruler"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_ruler.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    rng = np.random.default_rng(14)
    H, W, K, radius, mc, cap = 19, 43, 12, 2, 2, 25
    disp = make_map(rng, 1, H, W)
    conf = rng.uniform(0, 255, (1, H, W)).astype(np.float32)
    segs = random_segments(rng, K, 1, H, W)
    disp[0].tofile(tmp_path / "disp.bin")
    conf[0].tofile(tmp_path / "conf.bin")
    segs.tofile(tmp_path / "segs.bin")
    np.asarray(Q, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), str(K), str(radius), str(mc), str(cap), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "single_equal=1" in res.stdout and f"log_size={K}" in res.stdout and "bad_radius_code=-1" in res.stdout
    r = sdr.Ruler(Q, radius=radius, min_count=mc, conf_min=10.0, profile=True)
    want, wprof = run_device(disp, segs, conf=conf, profile_cap=cap, radius=radius, min_count=mc, conf_min=10.0,
                             profile=True)
    got = np.fromfile(tmp_path / "rec.bin", dtype=MEASUREMENT_DTYPE)
    RR.assert_records_equal(got, want)
    RR.assert_profile_equal(np.fromfile(tmp_path / "prof.bin", dtype=np.float32).reshape(K, cap, 4), wprof)
    xyz = sdr.reprojectImageTo3D(disp[0], Q, False)
    RR.assert_records_equal(np.fromfile(tmp_path / "rec_xyz.bin", dtype=MEASUREMENT_DTYPE), r.measure_xyz(xyz, segs))
    log = sdr.MeasurementLog()
    for k in range(K):
        log.add(100 + k, want[k], segs[k])
    assert (tmp_path / "log.csv").read_bytes() == log.to_csv().encode()
    assert log.to_csv() == RR.csv_text(range(100, 100 + K), segs, want)
