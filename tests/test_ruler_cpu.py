"""The ruler without a GPU: the numpy restatement of its definition (tests/ruler_ref.py) against
known answers, the reference's CSV bytes, the C structs' layout and the host-side argument guards."""
import ctypes
import os

import numpy as np
import pytest

import ruler_ref as RR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import MEASUREMENT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CSV = os.path.join(ROOT, "tests", "golden", "measurements.csv")
Q = S.REFERENCE_Q


# ---- the lower median ----
@pytest.mark.parametrize("values, want", [
    ([7.0], 7.0),
    ([9.0, 3.0], 3.0),              # n = 2: the lower of the two, not their mean
    ([5.0, 1.0, 3.0], 3.0),
    ([8.0, 2.0, 6.0, 4.0], 4.0),    # n = 4: element 1 of (2, 4, 6, 8)
    ([2.5, 2.5, 2.5, 2.5, 2.5], 2.5),
])
def test_lower_median_known_answers(values, want):
    got = RR.lower_median(values)
    assert got.dtype == np.float32 and got == np.float32(want)


def test_sample_selects_a_window_value():
    d = np.array([[10.0, 20.0, 30.0], [40.0, -1.0, 60.0], [70.0, 80.0, np.nan]], np.float32)
    xyz, dm, n, ok = RR.sample(d, None, Q, 1, 1, 1, 1, -1.0, 0.0)
    assert n == 7 and ok and dm == np.float32(40.0)  # (10 20 30 40 60 70 80)[3]
    want = RR.reproject(Q, 1, 1, np.float64(40.0))
    assert np.array_equal(xyz.view(np.uint32), want.view(np.uint32))
    # min_count above the valid count: invalid, all NaN
    xyz, dm, n, ok = RR.sample(d, None, Q, 1, 1, 1, 8, -1.0, 0.0)
    assert n == 7 and not ok and np.isnan(dm) and np.isnan(xyz).all()
    # clipped at the corner: rows 0..1 x columns 0..1
    xyz, dm, n, ok = RR.sample(d, None, Q, 0, 0, 1, 1, -1.0, 0.0)
    assert n == 3 and dm == np.float32(20.0)


def test_validity_equalities():
    """d == min_disp is rejected (strict >); conf == conf_min is accepted (>=); NaN conf is not."""
    d = np.array([[5.0, 2.0, 7.0]], np.float32)
    _, dm, n, ok = RR.sample(d, None, Q, 1, 0, 1, 1, 2.0, 0.0)
    assert n == 2 and dm == np.float32(5.0)
    _, _, n, ok = RR.sample(d, None, Q, 1, 0, 0, 1, 2.0, 0.0)
    assert n == 0 and not ok
    conf = np.array([[10.0, 9.999, np.nan]], np.float32)
    _, dm, n, ok = RR.sample(d, conf, Q, 1, 0, 1, 1, -1.0, 10.0)
    assert n == 1 and dm == np.float32(5.0) and ok
    # non-finite disparities never count; -0.0 > -1 does
    d = np.array([[np.inf, -np.inf, np.nan, -0.0]], np.float32)
    _, dm, n, ok = RR.sample(d, None, Q, 2, 0, 2, 1, -1.0, 0.0)
    assert n == 1 and dm == 0 and np.signbit(dm)


def test_conf_min_is_ignored_without_a_confidence_map():
    d = np.array([[5.0, 2.0, 7.0]], np.float32)
    _, dm, n, ok = RR.sample(d, None, Q, 1, 0, 1, 1, -1.0, np.nan)
    assert n == 3 and dm == np.float32(5.0) and ok
    _, _, n, ok = RR.sample(d, np.full((1, 3), 9.0, np.float32), Q, 1, 0, 1, 1, -1.0, np.nan)
    assert n == 0 and not ok


def test_computed_nans_are_canonical():
    """0 * inf in the reprojection makes a NaN whose sign depends on the machine; the record holds
    the canonical quiet NaN."""
    d = np.zeros((1, 2, 2), np.float32)
    Qc = np.array(Q)
    Qc[0, 3] = 0.0  # X = x / 0 at x = 0: 0 * inf
    r = RR.measure(d, [(0, 0, 0, 1, 1)], Qc)[0]
    assert np.isnan(r["p0"][0]) and r["p0"].view(np.uint32)[0] == 0x7FC00000
    assert r["distance"].view(np.uint64) == 0x7FF8000000000000


def test_zero_disparity_is_invalid_with_reference_q():
    """d = 0 makes w = 0 with REFERENCE_Q: the point is not finite, so it is invalid."""
    d = np.zeros((1, 3, 3), np.float32)
    r = RR.measure(d, [(0, 0, 0, 2, 2)], Q)[0]
    assert r["flags"] == 0 and np.isnan(r["distance"]) and r["n0"] == 1 and r["n1"] == 1
    assert not np.isfinite(r["p0"]).all() and r["d0"] == 0


# ---- the walk ----
def test_rdiv_and_walks():
    assert [RR.rdiv(a, 2) for a in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 1, 1, 2]  # ties round up
    assert RR.walk(3, 4, 3, 4) == [(3, 4)]                                         # n = 1
    assert RR.walk(1, 2, 4, 2) == [(1, 2), (2, 2), (3, 2), (4, 2)]                 # horizontal
    assert RR.walk(4, 2, 1, 2) == [(4, 2), (3, 2), (2, 2), (1, 2)]                 # negative delta
    assert RR.walk(5, 1, 5, 3) == [(5, 1), (5, 2), (5, 3)]                         # vertical
    assert RR.walk(0, 0, 2, 2) == [(0, 0), (1, 1), (2, 2)]                         # diagonal
    assert RR.walk(2, 0, 0, 2) == [(2, 0), (1, 1), (0, 2)]                         # anti-diagonal
    assert RR.walk(2, 2, 0, 0) == [(2, 2), (1, 1), (0, 0)]
    # a tie: 2 steps in x, 1 in y -- the middle sample's y is 0.5 and rounds up (towards +y), whichever
    # end the walk starts from, so the walk is not mirror-symmetric: the segment flipped in y takes
    # the other pixel
    assert RR.walk(0, 0, 2, 1) == [(0, 0), (1, 1), (2, 1)]
    assert RR.walk(0, 1, 2, 0) == [(0, 1), (1, 1), (2, 0)]  # -0.5 rounds up to 0: y = 1 + 0, not (1, 0)
    assert RR.walk(0, 0, 4, 1) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1)]
    # swapping the endpoints visits the same pixels in reverse: rdiv(a - m*d, m) = rdiv(a, m) - d
    rng = np.random.default_rng(1)
    for x0, y0, x1, y1 in rng.integers(-20, 20, (200, 4)).tolist() + [[0, 0, 2, 1], [2, 1, 0, 0], [0, 1, 2, 0]]:
        assert RR.walk(x1, y1, x0, y0) == RR.walk(x0, y0, x1, y1)[::-1]
    for (x0, y0, x1, y1) in ((0, 0, 9, 3), (9, 3, 0, 0), (2, 8, 5, 0), (7, 7, 0, 6)):
        w = RR.walk(x0, y0, x1, y1)
        assert w[0] == (x0, y0) and w[-1] == (x1, y1) and len(w) == max(abs(x1 - x0), abs(y1 - y0)) + 1
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(w, w[1:]))


# ---- reprojection against the oracle ----
def test_reprojection_equals_oracle(oracle):
    rng = np.random.default_rng(5)
    d = rng.uniform(-2, 90, (40, 64)).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf, 0.0, -1.0, -0.0):
        ys, xs = rng.integers(0, 40, 12), rng.integers(0, 64, 12)
        d[ys, xs] = v
    want = oracle.reproject(d, Q, False)
    ys, xs = np.mgrid[0:40, 0:64]
    got = RR.reproject(Q, xs, ys, d.astype(np.float64))
    same = got.view(np.uint32) == want.view(np.uint32)  # both on this CPU: NaNs included
    assert same.all(), int((~same).sum())
    # and one pixel through sample(): radius 0, min_count 1 is the pixel of reprojectImageTo3D
    for (x, y) in ((0, 0), (63, 39), (17, 5)):
        if np.isfinite(d[y, x]) and d[y, x] > -1:
            xyz, dm, n, _ = RR.sample(d, None, Q, x, y, 0, 1, -1.0, 0.0)
            assert n == 1 and np.array_equal(xyz.view(np.uint32), want[y, x].view(np.uint32))


# ---- distance ----
def test_distance_is_cv_norm():
    a = np.array([1.5, -2.0, 1000.25], np.float32)
    b = np.array([0.5, 2.0, 1000.0], np.float32)
    assert RR.distance(a, b) == np.sqrt(np.float64(1.0) + 16.0 + 0.0625)
    assert RR.distance(a, b) == RR.distance(b, a)
    # the difference is rounded to float32 before it is squared
    a = np.array([16777216.0, 0, 0], np.float32)
    b = np.array([-1.0, 0, 0], np.float32)
    assert RR.distance(a, b) == 16777216.0
    assert np.isinf(RR.distance(np.array([np.inf, 0, 0], np.float32), b))
    assert np.isnan(RR.distance(np.array([np.inf, 0, 0], np.float32), np.array([np.inf, 0, 0], np.float32)))


# ---- the profile ----
def test_profile_known_answers():
    d = np.full((1, 4, 12), 40.0, np.float32)
    d[0, 1, [0, 1, 5, 6, 7, 11]] = -1.0       # holes at the start (2), the middle (3) and the end (1)
    d[0, 1, 8] = 20.0                         # a depth step
    buf = np.full((2, 6, 4), -7.0, np.float32)
    r = RR.measure(d, [(0, 0, 1, 11, 1), (0, 3, 2, 3, 2)], Q, profile=True, profile_cap=6, profile_buf=buf)
    a = r[0]
    assert (a["path_samples"], a["path_valid"], a["max_gap"]) == (12, 6, 3)
    assert a["flags"] == RR.TRUNCATED and np.isnan(a["distance"])  # both endpoints are holes
    z40, z20 = RR.reproject(Q, 0, 0, 40.0)[2], RR.reproject(Q, 0, 0, 20.0)[2]
    assert a["z_min"] == z40 and a["z_max"] == z20 and a["max_dz"] == np.float32(z20 - z40)
    assert np.isnan(buf[0, :2]).all() and buf[0, 2, 3] == 40.0 and np.isnan(buf[0, 5]).all()
    b = r[1]  # zero length: one sample, no step
    assert (b["path_samples"], b["path_valid"], b["max_gap"]) == (1, 1, 0)
    assert b["flags"] == 3 and b["distance"] == 0.0 and np.isnan(b["max_dz"]) and b["z_min"] == z40
    assert buf[1, 0, 3] == 40.0 and (buf[1, 1:] == -7.0).all()  # rows past the segment stay
    # without the profile the counts are 0 and the floats NaN
    c = RR.measure(d, [(0, 2, 0, 9, 3)], Q)[0]
    assert (c["path_samples"], c["path_valid"], c["max_gap"]) == (0, 0, 0)
    assert np.isnan([c["z_min"], c["z_max"], c["max_dz"]]).all() and c["flags"] == 3
    # out of range: flag bit 2, every float NaN
    for seg in ((1, 0, 0, 1, 1), (-1, 0, 0, 1, 1), (0, 12, 0, 1, 1), (0, 0, 0, 1, 4), (0, 0, -1, 1, 1)):
        o = RR.measure(d, [seg], Q, profile=True)[0]
        assert o["flags"] == RR.OUT_OF_RANGE and np.isnan(o["p0"]).all() and np.isnan(o["distance"])
        assert (o["n0"], o["n1"], o["path_samples"]) == (0, 0, 0)


# ---- why the window: a noisy wall with holes and outliers ----
def wall_scene(seed):
    rng = np.random.default_rng(seed)
    H, W = 60, 160
    d = 40.0 + rng.normal(0.0, 0.25, (H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    u = rng.random((H, W))
    d[u < 0.15] = -1.0
    out = (u >= 0.15) & (u < 0.18)
    d[out] = rng.uniform(1, 79, int(out.sum())).astype(np.float32)
    segs = np.stack([np.zeros(20, np.int64), rng.integers(0, W, 20), rng.integers(0, H, 20),
                     rng.integers(0, W, 20), rng.integers(0, H, 20)], axis=1)
    return d[None], segs


def test_wall_scene_single_pixel_fails_window_does_not():
    not_finite_r0, valid_r2 = 0, 0
    for seed in range(20):
        d, segs = wall_scene(seed)
        r0 = RR.measure(d, segs, Q, radius=0, min_count=1)
        r2 = RR.measure(d, segs, Q, radius=2, min_count=3)
        not_finite_r0 += int((~np.isfinite(r0["distance"])).sum())
        valid_r2 += int(((r2["flags"] & 3) == 3).sum())
        assert np.isfinite(r2["distance"]).all()
    assert not_finite_r0 >= 1, not_finite_r0
    assert valid_r2 == 400, valid_r2


# ---- the CSV log ----
GOLDEN_RECORDS = [(3, (434, 117, 440, 189), 2400.2902), (3, (385, 162, 397, 241), 1929.7459)]


def test_csv_reference_bytes():
    want = open(GOLDEN_CSV, "rb").read()
    recs = np.zeros(2, MEASUREMENT_DTYPE)
    recs["distance"] = [g[2] for g in GOLDEN_RECORDS]
    segs = [(0,) + g[1] for g in GOLDEN_RECORDS]
    assert RR.csv_text([3, 3], segs, recs).encode() == want


def test_csv_engine_bytes(tmp_path):
    """sdr_measurements_csv and MeasurementLog reproduce the reference's file byte for byte."""
    want = open(GOLDEN_CSV, "rb").read()
    log = sdr.MeasurementLog()
    for idx, seg, dist in GOLDEN_RECORDS:
        r = np.zeros((), MEASUREMENT_DTYPE)
        r["distance"] = dist
        log.add(idx, r, seg)
    assert len(log) == 2
    assert log.to_csv().encode() == want
    assert log.to_csv(header=False).encode() == want[want.index(b"\n") + 1:]
    path = tmp_path / "measurements.csv"
    log.save_csv(path)
    log.save_csv(path)  # appends, header included, as the reference's std::ios::app does
    assert path.read_bytes() == want + want
    # the length query, a buffer that is too small, an empty log
    L = _lib.lib()
    idx = (ctypes.c_int * 2)(3, 3)
    segs = (_lib.Segment * 2)(*[_lib.Segment(0, *g[1]) for g in GOLDEN_RECORDS])
    recs = (_lib.Measurement * 2)()
    for i, g in enumerate(GOLDEN_RECORDS):
        recs[i].distance = g[2]
    n = L.sdr_measurements_csv(idx, segs, recs, 2, 1, None, 0)
    assert n == len(want)
    buf = ctypes.create_string_buffer(n + 1)
    assert L.sdr_measurements_csv(idx, segs, recs, 2, 1, buf, n + 1) == n and buf.raw[:n] == want
    assert L.sdr_measurements_csv(idx, segs, recs, 2, 1, buf, n) == -1
    assert L.sdr_measurements_csv(None, None, None, 0, 1, None, 0) == want.index(b"\n") + 1
    assert L.sdr_measurements_csv(None, None, None, 0, 0, None, 0) == 0
    assert L.sdr_measurements_csv(None, segs, recs, 2, 1, None, 0) == -1
    assert sdr.MeasurementLog().to_csv(header=False) == ""


def test_csv_non_finite_distance():
    recs = np.zeros(2, MEASUREMENT_DTYPE)
    recs["distance"] = [np.inf, 12.5]
    log = sdr.MeasurementLog()
    log.add(1, recs[0], (0, 1, 2, 3, 4))
    log.add(2, recs[1], (5, 6, 7, 8))
    assert log.to_csv(header=False) == "1, [1, 2],    [3, 4], inf cm   \n2, [5, 6],    [7, 8], 1.25000 cm   \n"


# ---- struct layout ----
OFFSETS = dict(p0=0, p1=12, d0=24, d1=28, distance=32, n0=40, n1=44, path_samples=48, path_valid=52,
               max_gap=56, z_min=60, z_max=64, max_dz=68, flags=72, reserved=76)


def test_struct_layout():
    assert ctypes.sizeof(_lib.Measurement) == 80 and MEASUREMENT_DTYPE.itemsize == 80
    assert RR.DTYPE == MEASUREMENT_DTYPE
    for name, off in OFFSETS.items():
        assert getattr(_lib.Measurement, name).offset == off, name
        assert MEASUREMENT_DTYPE.fields[name][1] == off, name
    assert [n for n, _ in _lib.Measurement._fields_] == list(MEASUREMENT_DTYPE.names)
    assert ctypes.sizeof(_lib.RulerParams) == 24
    assert [(n, getattr(_lib.RulerParams, n).offset) for n, _ in _lib.RulerParams._fields_] == [
        ("radius", 0), ("min_count", 4), ("min_disp", 8), ("conf_min", 12), ("profile", 16), ("profile_cap", 20)]
    assert ctypes.sizeof(_lib.Segment) == 20
    p = _lib.RulerParams(9, 9, 9.0, 9.0, 9, 9)
    _lib.lib().sdr_ruler_params_default(ctypes.byref(p))
    assert (p.radius, p.min_count, p.min_disp, p.conf_min, p.profile, p.profile_cap) == (0, 1, -1.0, 0.0, 0, 0)
    assert _lib.lib().sdr_abi_version() == 4


# ---- host-side guards: every refusal comes before any device call ----
def test_host_guards_without_a_device():
    L = _lib.lib()
    Qc = (ctypes.c_double * 16)(*np.asarray(Q).reshape(16))
    p = _lib.RulerParams(0, 1, -1.0, 0.0, 0, 0)
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F, K = 8, 6, 2, 3

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=p, segs=ptr, k=K, out=ptr,
            prof=None):
        return L.sdr_measure_disp_device(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                         segs, k, out, prof, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, q=Qc, par=p, segs=ptr, k=K, out=ptr,
             prof=None):
        return L.sdr_measure_disp(disp, typ, stride, fs, w, h, f, None, q, ctypes.byref(par) if par else None,
                                  segs, k, out, prof)

    for fn in (dev, host):
        assert fn(disp=None) == -1 and fn(q=None) == -1 and fn(par=None) == -1
        assert fn(segs=None) == -1 and fn(out=None) == -1
        assert fn(k=-1) == -1
        assert fn(w=0) == -1 and fn(h=0) == -1 and fn(f=0) == -1 and fn(w=-3) == -1
        assert fn(stride=W - 1) == -1 and fn(fs=W * H - 1) == -1
        for bad in (_lib.RulerParams(5, 1, -1.0, 0.0, 0, 0), _lib.RulerParams(-1, 1, -1.0, 0.0, 0, 0),
                    _lib.RulerParams(0, 0, -1.0, 0.0, 0, 0), _lib.RulerParams(0, -2, -1.0, 0.0, 0, 0)):
            assert fn(par=bad) == -1
        assert fn(typ=2) == -5 and fn(typ=-1) == -5
        assert L.sdr_last_error()
        # K == 0: SDR_OK, nothing launched, segments and records may be null
        assert fn(k=0, segs=None, out=None) == 0

    def xdev(xyz=ptr, stride=3 * W, fs=3 * W * H, w=W, h=H, f=F, segs=ptr, k=K, out=ptr):
        return L.sdr_measure_xyz_device(xyz, stride, fs, w, h, f, segs, k, out, None)

    def xhost(xyz=ptr, stride=3 * W, fs=3 * W * H, w=W, h=H, f=F, segs=ptr, k=K, out=ptr):
        return L.sdr_measure_xyz(xyz, stride, fs, w, h, f, segs, k, out)

    for fn in (xdev, xhost):
        assert fn(xyz=None) == -1 and fn(segs=None) == -1 and fn(out=None) == -1
        assert fn(k=-1) == -1 and fn(w=0) == -1 and fn(h=-1) == -1 and fn(f=0) == -1
        assert fn(stride=3 * W - 1) == -1
        assert fn(k=0, segs=None, out=None) == 0


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    with pytest.raises(sdr.SDRError):
        r.measure(np.zeros((4, 4), np.float64), [(0, 0, 1, 1)])
    with pytest.raises(sdr.SDRError):
        r.measure(np.zeros((4, 4), np.float32), [(0, 0, 1)])
    with pytest.raises(sdr.SDRError):
        sdr.Ruler(Q, radius=5).measure(np.zeros((4, 4), np.float32), [(0, 0, 1, 1)])
    with pytest.raises(sdr.SDRError):
        r.measure_xyz(np.zeros((4, 4, 2), np.float32), [(0, 0, 1, 1)])
    # no segments: empty records without a device
    assert r.measure(np.zeros((4, 4), np.float32), []).shape == (0,)
    assert r.measure_xyz(np.zeros((4, 4, 3), np.float32), np.zeros((0, 5), np.int32)).shape == (0,)
