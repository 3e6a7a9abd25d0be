"""CPU-only checks of the ruler over time (include/sdr/sdr.h, "the ruler over time"): the numpy
restatement (tests/fuse_ref.py) against plain loops and known answers, the structs, the host guards
of both entries, and what the fusion buys on the noisy wall of tests/test_ruler_cpu.py."""
import ctypes

import numpy as np
import pytest

import fuse_ref as FR
import ruler_ref as RR
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd.ruler import FUSION_DTYPE

Q = S.REFERENCE_Q
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def column(values, dtype=np.float32):
    """A stack (F, 1, 1) of one pixel's values."""
    return np.asarray(values, dtype).reshape(-1, 1, 1)


# ---- the restatement against plain loops ----
def special_stack(rng, F, H, W, tol):
    """Small values on a 1/4 px grid (ties, and differences of exactly `tol`) with NaN, +-inf, +-0.0
    and invalid values planted."""
    v = (rng.integers(-4, 12, (F, H, W)) * 0.25).astype(np.float32)
    v += np.float32(tol) * rng.integers(0, 2, (F, H, W)).astype(np.float32)
    u = rng.random((F, H, W))
    v[u < 0.05] = NAN
    v[(u >= 0.05) & (u < 0.08)] = INF
    v[(u >= 0.08) & (u < 0.11)] = -INF
    v[(u >= 0.11) & (u < 0.16)] = np.float32(-0.0)
    v[(u >= 0.16) & (u < 0.21)] = np.float32(0.0)
    conf = rng.integers(0, 4, (F, H, W)).astype(np.float32)
    conf[rng.random((F, H, W)) < 0.1] = NAN
    return v, conf


@pytest.mark.parametrize("F", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("mode", [FR.MEAN, FR.MEDIAN])
def test_restatement_equals_plain_loops(F, mode):
    rng = np.random.default_rng(100 * F + mode)
    for tol, min_count, min_disp, with_conf in ((0.5, 1, -1.0, True), (0.25, 2, -0.5, False), (0.0, 3, -1e30, True),
                                                (1.0, F, -1.0, False), (1.0, F + 1, -1.0, True)):
        v, conf = special_stack(rng, F, 5, 7, tol)
        kw = dict(conf=conf if with_conf else None, min_disp=min_disp, conf_min=1.0, tol=tol,
                  min_count=min(min_count, 32), mode=mode, fill=NAN)
        FR.assert_fusion_equal(FR.fuse(v, **kw), FR.fuse_loops(v, **kw))
    # int16 input, the ruler's default fill
    s16 = rng.integers(-40, 200, (F, 4, 9)).astype(np.int16)
    FR.assert_fusion_equal(FR.fuse(s16, tol=0.5, mode=mode), FR.fuse_loops(s16, tol=0.5, mode=mode))


# ---- known answers ----
def test_two_surfaces_known_answer():
    v = column([40, 40, 60, 60])
    out, rec, sup, spr, cls = FR.fuse(v, tol=1.0, min_count=3, classes=True)
    assert cls[0, 0] == FR.UNSTABLE and out[0, 0] == -1.0 and sup[0, 0] == 0 and np.isnan(spr[0, 0])
    assert (rec["n_unstable"], rec["n_fused"], rec["n_sparse"], rec["n_empty"]) == (1, 0, 0, 0)
    out, rec, sup, spr, cls = FR.fuse(v, tol=1.0, min_count=2, classes=True)
    assert cls[0, 0] == FR.FUSED and out[0, 0] == 40.0 and sup[0, 0] == 2 and spr[0, 0] == 0.0
    # the last frame is valid and does not agree: an outlier replaced; two values disagree
    assert (rec["n_fused"], rec["n_replaced"], rec["n_filled"], rec["sum_support"], rec["n_disagree"]) == (1, 1, 0, 2, 2)
    # too few valid values is SPARSE, none is EMPTY
    assert FR.fuse(column([40, -1, -1, -1]), min_count=2, classes=True)[4][0, 0] == FR.SPARSE
    assert FR.fuse(column([-1, NAN, -INF, INF]), min_count=1, classes=True)[4][0, 0] == FR.EMPTY


def test_zero_tie_goes_to_the_earlier_frames_bits():
    neg, pos = np.float32(-0.0), np.float32(0.0)
    for first, second in ((neg, pos), (pos, neg)):
        out = FR.fuse(column([first, second]), min_disp=-1.0, tol=0.0, min_count=1, mode=FR.MEDIAN)[0]
        assert out.view(np.uint32)[0, 0] == np.array([first]).view(np.uint32)[0]
    # three values: the median is element 1 of (-0.0, +0.0, 5) in frame order among the equal ones
    out = FR.fuse(column([pos, 5.0, neg]), tol=0.0, min_count=1, mode=FR.MEDIAN)[0]
    assert out.view(np.uint32)[0, 0] == 0x80000000
    # the spread's extremes by < keep the earliest of equal values: (+0) - (+0), not (-0) - (+0)
    spr = FR.fuse(column([pos, neg]), tol=0.0, min_count=1)[3]
    assert spr.view(np.uint32)[0, 0] == 0


def test_int16_mean_is_the_exact_mean_rounded_once():
    rng = np.random.default_rng(5)
    s16 = (640 + rng.integers(-7, 8, (7, 6, 10))).astype(np.int16)  # 40 px +- 7/16: all agree at tol 1
    out, rec, sup, _ = FR.fuse(s16, tol=1.0, min_count=2)
    assert (sup == 7).all()
    total = s16.astype(np.int64).sum(axis=0)
    for y in range(6):
        for x in range(10):
            # the exact rational total / (16 * 7), rounded to float once (a float64 holds the sum exactly)
            assert out[y, x] == np.float32(float(total[y, x]) / 16.0 / 7.0)
    # sum / 16 is exact in double, so one double division rounds the true mean once; float then once
    # more: equal to the single rounding unless the double lands on a float tie, which /7 of these
    # integers does not


def test_one_frame_is_the_validity_gate():
    rng = np.random.default_rng(6)
    v, conf = special_stack(rng, 1, 6, 11, 0.5)
    for mode in (FR.MEAN, FR.MEDIAN):
        out, rec, sup, spr = FR.fuse(v, conf=conf, conf_min=1.0, min_count=1, mode=mode, fill=NAN)
        ok = FR.valid_mask(v, conf, -1.0, 1.0)[0]
        assert np.array_equal(out[ok], v[0][ok])
        if mode == FR.MEDIAN:  # the value itself; the mean of -0.0 alone is +0.0 + -0.0 = +0.0
            assert np.array_equal(out.view(np.uint32)[ok], v[0].view(np.uint32)[ok])
        assert (v[0][ok].view(np.uint32) == 0x80000000).any()
        assert np.isnan(out[~ok]).all()
        assert np.array_equal(sup, ok.astype(np.uint8)) and (spr[ok] == 0).all()
        assert rec["n_fused"] == ok.sum() and rec["n_empty"] == (~ok).sum() and rec["n_filled"] == 0
    # min_count 2 on one frame: every valid pixel is SPARSE
    rec = FR.fuse(v, min_count=2)[1]
    assert rec["n_fused"] == 0 and rec["n_sparse"] + rec["n_empty"] == v[0].size


# ---- the structs ----
def test_struct_layout_and_defaults():
    assert ctypes.sizeof(_lib.FuseParams) == 32 and ctypes.sizeof(_lib.Fusion) == 64
    assert [(n, getattr(_lib.FuseParams, n).offset) for n, _ in _lib.FuseParams._fields_] == [
        ("min_disp", 0), ("conf_min", 4), ("tol", 8), ("fill", 12), ("min_count", 16), ("mode", 20), ("reserved", 24)]
    assert FUSION_DTYPE == FR.DTYPE and FUSION_DTYPE.itemsize == 64
    assert [n for n, _ in _lib.Fusion._fields_] == list(FUSION_DTYPE.names)
    for name in FUSION_DTYPE.names:
        assert getattr(_lib.Fusion, name).offset == FUSION_DTYPE.fields[name][1], name
    assert FUSION_DTYPE.fields["n_fused"][1] == 16 and FUSION_DTYPE.fields["sum_support"][1] == 40
    p = _lib.FuseParams(9.0, 9.0, 9.0, 9.0, 9, 9, (ctypes.c_int32 * 2)(9, 9))
    _lib.lib().sdr_fuse_params_default(ctypes.byref(p))
    assert (p.min_disp, p.conf_min, p.tol, p.fill, p.min_count, p.mode, tuple(p.reserved)) == (
        -1.0, 0.0, 1.0, -1.0, 2, _lib.FUSE_MEAN, (0, 0))
    _lib.lib().sdr_fuse_params_default(None)
    assert (sdr.FUSE_MEAN, sdr.FUSE_MEDIAN, _lib.FUSE_MAX_FRAMES) == (0, 1, 32) == (FR.MEAN, FR.MEDIAN, FR.MAX_FRAMES)
    assert sdr.FuseParams is _lib.FuseParams and sdr.FUSION_DTYPE is FUSION_DTYPE


# ---- host-side guards: every refusal comes before any device call ----
def test_host_guards_without_a_device():
    L = _lib.lib()
    ptr = ctypes.c_void_p(4096)  # never dereferenced: the guards return first
    W, H, F = 8, 6, 3

    def params(**kw):
        p = _lib.FuseParams()
        L.sdr_fuse_params_default(ctypes.byref(p))
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    good = params()

    def dev(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, par=good, out=ptr):
        return L.sdr_fuse_disp_device(disp, typ, stride, fs, w, h, f, None, ctypes.byref(par) if par else None, out,
                                      None, None, None, None)

    def host(disp=ptr, typ=0, stride=W, fs=W * H, w=W, h=H, f=F, par=good, out=ptr):
        return L.sdr_fuse_disp(disp, typ, stride, fs, w, h, f, None, ctypes.byref(par) if par else None, out, None,
                               None, None)

    ARG, LIMIT = -1, -8
    for fn in (dev, host):
        assert fn(disp=None) == ARG and fn(out=None) == ARG and fn(par=None) == ARG
        assert fn(w=0) == ARG and fn(h=0) == ARG and fn(f=0) == ARG and fn(w=-3) == ARG and fn(f=-1) == ARG
        assert fn(stride=W - 1) == ARG
        # whole frames: frame_stride >= stride * height, with a padded row too; one frame has none
        assert fn(fs=W * H - 1) == ARG and fn(stride=W + 2, fs=(W + 2) * H - 1) == ARG
        assert fn(typ=2) == ARG and fn(typ=-1) == ARG
        assert fn(par=params(mode=2)) == ARG and fn(par=params(mode=-1)) == ARG
        for tol in (-0.5, float("nan"), float("inf")):
            assert fn(par=params(tol=tol)) == ARG
        assert fn(par=params(min_count=0)) == ARG and fn(par=params(min_count=33)) == ARG
        bad = params()
        bad.reserved[1] = 1
        assert fn(par=bad) == ARG
        # a fill that the ruler would take for a measurement
        assert fn(par=params(fill=0.0)) == ARG and fn(par=params(fill=40.0)) == ARG
        assert fn(par=params(min_disp=-5.0, fill=-1.0)) == ARG
        assert L.sdr_last_error()
        assert fn(f=33) == LIMIT and fn(f=1000) == LIMIT
        assert fn(w=65536, h=32768, stride=65536, fs=65536 * 32768) == LIMIT
        assert b"INT32_MAX" in L.sdr_last_error()
        # an argument error wins over a limit
        assert fn(f=33, par=params(tol=-1.0)) == ARG


def test_python_surface_checks_arguments():
    r = sdr.Ruler(Q)
    with pytest.raises(sdr.SDRError):
        r.fuse(np.zeros((2, 4, 4), np.float64))
    with pytest.raises(sdr.SDRError):
        r.fuse(np.zeros((2, 4, 4), np.float32), conf=np.zeros((2, 4, 5), np.float32))
    with pytest.raises(sdr.SDRError):
        r.fuse_device(np.zeros((2, 4, 4), np.float32))
    for kw in (dict(tol=-1.0), dict(min_count=0), dict(mode=7), dict(fill=3.0)):
        with pytest.raises(sdr.SDRError) as e:
            r.fuse(np.zeros((2, 4, 4), np.float32), **kw)
        assert e.value.code == -1
    with pytest.raises(sdr.SDRError) as e:
        r.fuse(np.zeros((33, 4, 4), np.float32))
    assert e.value.code == -8


# ---- what the fusion buys: the noisy wall of test_ruler_cpu.py, eight frames of it ----
def wall_frames(seed, F=8):
    """F frames drawn one after another as test_ruler_cpu.wall_scene draws its one, then the 20
    segments."""
    rng = np.random.default_rng(1000 + seed)
    H, W = 60, 160
    frames = []
    for _ in range(F):
        d = 40.0 + rng.normal(0.0, 0.25, (H, W))
        d = (np.round(d * 16) / 16).astype(np.float32)
        u = rng.random((H, W))
        d[u < 0.15] = -1.0
        out = (u >= 0.15) & (u < 0.18)
        d[out] = rng.uniform(1, 79, int(out.sum())).astype(np.float32)
        frames.append(d)
    segs = np.stack([np.zeros(20, np.int64), rng.integers(0, W, 20), rng.integers(0, H, 20),
                     rng.integers(0, W, 20), rng.integers(0, H, 20)], axis=1)
    return np.stack(frames), segs


def wall_truth(segs):
    """The segments' lengths on the noiseless wall at 40 px."""
    flat = np.full((1, 60, 160), 40.0, np.float32)
    return RR.measure(flat, segs, Q, radius=0, min_count=1)["distance"]


def test_wall_scene_over_time():
    """Eight frames of the wall (40 px, sigma 0.25 px quantised to 1/16 px, 15 % holes, 3 %
    outliers), 20 seeds x 20 segments measured at radius 0 / min_count 1, fused with tol 1.0 and
    min_count 2.  Measured: the last frame alone leaves 109 of 400 distances non-finite with a
    median error of 7.85 mm over the finite ones; the fused maps leave 0, with a median error of
    3.16 mm (MEAN) and 4.14 mm (MEDIAN).  Conditions and orderings are asserted, not these values."""
    bad = {"single": 0, "mean": 0, "median": 0}
    err = {"single": [], "mean": [], "median": []}
    for seed in range(20):
        frames, segs = wall_frames(seed)
        truth = wall_truth(segs)
        maps = {"single": frames[-1:], "mean": FR.fuse(frames, tol=1.0, min_count=2, mode=FR.MEAN)[0][None],
                "median": FR.fuse(frames, tol=1.0, min_count=2, mode=FR.MEDIAN)[0][None]}
        for name, d in maps.items():
            dist = RR.measure(d, segs, Q, radius=0, min_count=1)["distance"]
            fin = np.isfinite(dist)
            bad[name] += int((~fin).sum())
            err[name] += list(np.abs(dist[fin] - truth[fin]))
    med = {k: float(np.median(e)) for k, e in err.items()}
    print(f"non-finite of 400: {bad}; median error (mm): {med}")
    assert bad["mean"] == 0 and bad["median"] == 0, bad
    assert bad["single"] >= 1, bad
    assert med["mean"] < med["median"] < med["single"], med


# ---- moving content ----
def moving_stack():
    """F = 8 frames of a still surface at 30 px with fixed holes; in the last three a rectangle
    stands 8 px of disparity nearer."""
    rng = np.random.default_rng(9)
    F, H, W = 8, 40, 64
    box = np.zeros((H, W), bool)
    box[10:25, 20:50] = True
    still = (30.0 + np.round(rng.normal(0.0, 0.2, (F, H, W)) * 16) / 16).astype(np.float32)
    hole = rng.random((H, W)) < 0.1
    still[:, hole] = -1.0
    moved = still.copy()
    moved[5:, box & ~hole] += np.float32(8.0)
    return still, moved, box, hole


def test_moving_content_is_unstable_not_averaged():
    """Five still frames and three moved ones: with min_count 6 no six values of a pixel agree, so
    every pixel of the rectangle is `fill`, UNSTABLE where it has values at all, and nothing outside
    the rectangle changes.  (With min_count 5 the five still frames do agree, n_in == min_count, and
    the rule fuses them: the next test.)"""
    still, moved, box, hole = moving_stack()
    kw = dict(tol=1.0, min_count=6, classes=True)
    out, rec, sup, spr, cls = FR.fuse(moved, **kw)
    out0, rec0, _, _, cls0 = FR.fuse(still, **kw)
    assert (out[box] == -1.0).all() and (sup[box] == 0).all() and np.isnan(spr[box]).all()
    valid_area = int((box & ~hole).sum())
    assert valid_area > 300 and (cls[box & ~hole] == FR.UNSTABLE).all() and (cls[box & hole] == FR.EMPTY).all()
    assert rec["n_unstable"] == valid_area and rec0["n_unstable"] == 0
    assert np.array_equal(cls[~box], cls0[~box])
    assert np.array_equal(out.view(np.uint32)[~box], out0.view(np.uint32)[~box])
    assert rec["n_fused"] == rec0["n_fused"] - valid_area and rec["n_empty"] == rec0["n_empty"] == hole.sum()


def test_moving_content_at_min_count_five_keeps_the_still_surface():
    """The same stack at min_count 5: the lower median of five still and three moved values is a
    still one, the five still values agree with it, and n_in == min_count fuses (as [40, 40, 60, 60]
    does at min_count 2).  The result is the still surface, not an average of the two, and the record
    says that the last frame was replaced in every pixel of the rectangle."""
    still, moved, box, hole = moving_stack()
    out, rec, sup, spr, cls = FR.fuse(moved, tol=1.0, min_count=5, classes=True)
    want = FR.fuse(still[:5], tol=1.0, min_count=5)[0]
    valid_area = int((box & ~hole).sum())
    assert (cls[box & ~hole] == FR.FUSED).all() and (sup[box & ~hole] == 5).all()
    assert np.array_equal(out.view(np.uint32)[box], want.view(np.uint32)[box])
    assert (np.abs(out[box & ~hole] - 30.0) < 1.0).all()
    assert rec["n_replaced"] == valid_area and rec["n_unstable"] == 0 and rec["n_disagree"] == 3 * valid_area
