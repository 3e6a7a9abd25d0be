"""The stand-alone post entries (sdr_post.hip behind the ABI of sdr_engine.hip) at their borders and
strides, BIT FOR BIT: reprojectImageTo3D from float and from int16 disparities (device and host
entries) with a matrix Q that has no zero entry, so that every one of the 16 products and the order
of the sums count; handleMissingValues with a different minimum in every frame of a batch; widths
around the wave (64) and the workgroup (256); padded rows with sentinel-filled padding;
convertTo(1/16) across its grid-stride loop; BGR2GRAY and INTER_AREA 0.5x on padded batches, against
the oracle and a plain integer formula.

Floats are compared as uint32.  Where the reference is NaN the kernel's value must be a NaN: the
sign of 0 * inf differs between machines (test_gpu_ruler.py).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ingest_cases as C  # noqa: E402
import numpy_ref as NR  # noqa: E402
from stereo_depth_ruler_amd._lib import lib  # noqa: E402
from stereo_depth_ruler_amd.sgbm import _cstream  # noqa: E402

ERR_ARG, ERR_SIZE = -1, -4
FSENT = np.float32(-777.25)
SENT = 0xA5
TAIL = 64
WIDTHS = [1, 5, 63, 64, 65, 255, 256, 257, 300]
SHAPES = [(w, 3 + i % 7) for i, w in enumerate(WIDTHS)]  # (W, H), H in 3..9


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dense_q():
    Q = np.random.default_rng(2024).normal(0, 1, (4, 4))
    Q[3] *= 1e-2
    Q[3, 3] += 0.5
    assert (Q != 0).all()
    return Q


Q_DENSE = dense_q()
# w = 0.25 d - 1: exactly zero at d == 4 (X, Y, Z are +-inf there, NaN where the numerator is zero)
Q_ZERO_W = np.array([[1, 0, 0, -2], [0, 1, 0, -1], [0, 0, 0, 700], [0, 0, 0.25, -1]], np.float64)


def qptr(Q):
    return (ctypes.c_double * 16)(*np.asarray(Q, np.float64).ravel())


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def same(got, ref):
    """Equal as uint32, except that a NaN of the reference asks only for a NaN."""
    g, r = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    nan = np.isnan(r)
    return bool(((g.view(np.uint32) == r.view(np.uint32)) | (nan & np.isnan(g))).all())


def frames_with_minima(rng, W, H, grid16=False):
    """Three (H, W) float frames whose minima differ: frame 0 holds its minimum in the last pixel
    only, frame 1 at two places, frame 2 wherever the random values put it (and above the other
    two, so a minimum shared between frames marks the wrong pixels or none)."""
    n = W * H
    if grid16:
        d = (rng.integers(16, 90 * 16, (3, n)) / 16.0).astype(np.float32)
    else:
        d = rng.uniform(1.0, 90.0, (3, n)).astype(np.float32)
    d[0, n - 1] = -3.0
    d[1, 0] = d[1, n // 2] = -7.5
    return d.reshape(3, H, W), (1, 2 if n // 2 != 0 else 1, None)


def check_missing_counts(xyz, ref, counts):
    for f, want in enumerate(counts):
        n = int((xyz[f][..., 2] == 10000.0).sum())
        assert n == int((ref[f][..., 2] == 10000.0).sum()), f
        if want is not None:
            assert n == want, (f, n)


def run_reproject_f32(disp, Q, hm, pad_d=0, pad_x=0):
    """sdr_reproject_device on (F, H, W) frames with rows padded by pad_d / pad_x elements; the
    disparity's padding holds values below every minimum, the output's a sentinel."""
    F, H, W = disp.shape
    ds, xs = W + pad_d, 3 * W + pad_x
    d = np.full((F, H, ds), -1000.0, np.float32)
    d[:, :, :W] = disp
    x = torch.full((F * H * xs + TAIL,), float(FSENT), dtype=torch.float32, device="cuda")
    d_disp = dev(d)
    rc = lib().sdr_reproject_device(d_disp.data_ptr(), W, H, ds, qptr(Q), int(hm), x.data_ptr(), xs, F, _cstream(0))
    torch.cuda.synchronize()
    assert rc == 0, lib().sdr_last_error()
    x = x.cpu().numpy()
    assert (x[F * H * xs:] == FSENT).all()
    x = x[:F * H * xs].reshape(F, H, xs)
    assert (x[:, :, 3 * W:] == FSENT).all()
    return np.ascontiguousarray(x[:, :, :3 * W]).reshape(F, H, W, 3)


def run_reproject_s16(d16, Q, hm, pad_d=0, pad_x=0, expect=0):
    F, H, W = d16.shape
    ds, xs = W + pad_d, 3 * W + pad_x
    d = np.full((F, H, ds), -32768, np.int16)
    d[:, :, :W] = d16
    x = torch.full((F * H * xs + TAIL,), float(FSENT), dtype=torch.float32, device="cuda")
    d_disp = dev(d)
    rc = lib().sdr_disp16_reproject_device(d_disp.data_ptr(), W, H, ds, qptr(Q), int(hm), x.data_ptr(), xs, F,
                                           _cstream(0))
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib().sdr_last_error())
    x = x.cpu().numpy()
    if rc:
        assert (x == FSENT).all()
        return None
    assert (x[F * H * xs:] == FSENT).all()
    x = x[:F * H * xs].reshape(F, H, xs)
    assert (x[:, :, 3 * W:] == FSENT).all()
    return np.ascontiguousarray(x[:, :, :3 * W]).reshape(F, H, W, 3)


def run_reproject_host(disp, Q, hm, pad_d=3, pad_x=4):
    """sdr_reproject (host pointers, one frame) on padded rows."""
    H, W = disp.shape
    d = np.full((H, W + pad_d), -1000.0, np.float32)
    d[:, :W] = disp
    x = np.full((H, 3 * W + pad_x), FSENT, np.float32)
    rc = lib().sdr_reproject(d.ctypes.data, W, H, W + pad_d, qptr(Q), int(hm), x.ctypes.data, 3 * W + pad_x)
    assert rc == 0, lib().sdr_last_error()
    assert (x[:, 3 * W:] == FSENT).all()
    return np.ascontiguousarray(x[:, :3 * W]).reshape(H, W, 3)


_REF = {}


def reference(oracle, key, disp, Q, hm):
    """oracle.reproject of every frame, computed once per key."""
    k = (key, bool(hm))
    if k not in _REF:
        _REF[k] = np.stack([oracle.reproject(f, Q, hm) for f in disp])
    return _REF[k]


# ---- reprojectImageTo3D ---------------------------------------------------------------------------

@pytest.mark.parametrize("hm", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_reproject_float_entries_dense_q(oracle, shape, hm):
    """sdr_reproject_device (dense and padded rows, three frames) and sdr_reproject (padded host
    rows) with the dense Q, against the oracle and the numpy restatement."""
    W, H = shape
    disp, counts = frames_with_minima(np.random.default_rng(W * 31 + H), W, H)
    ref = reference(oracle, ("f32", W, H), disp, Q_DENSE, hm)
    for f in range(3):
        assert same(NR.reproject(disp[f], Q_DENSE, hm), ref[f])  # two references, one answer
    for pad_d, pad_x in ((0, 0), (3, 4), (1, 0), (0, 2)):
        got = run_reproject_f32(disp, Q_DENSE, hm, pad_d, pad_x)
        assert same(got, ref), (pad_d, pad_x)
        if hm:
            check_missing_counts(got, ref, counts)
    host = np.stack([run_reproject_host(disp[f], Q_DENSE, hm) for f in range(3)])
    assert same(host, ref)
    if hm:
        check_missing_counts(host, ref, counts)


@pytest.mark.parametrize("hm", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_reproject_int16_entry_dense_q(oracle, shape, hm):
    """sdr_disp16_reproject_device, three frames with the int16 extremes among the values; padded
    rows without handle_missing, and the refusal of handle_missing on a strided map."""
    W, H = shape
    rng = np.random.default_rng(W * 37 + H)
    n = W * H
    d16 = rng.integers(16, 90 * 16, (3, n)).astype(np.int16)
    # frame 0: the minimum -32768 in the last pixel only; frame 1: -120 at two places; frame 2: its own
    d16[0, n - 1] = -32768
    d16[1, 0] = d16[1, n // 2] = -120
    d16[2, n // 3] = 32767
    if n > 4:
        d16[0, 1] = 32767
    d16 = d16.reshape(3, H, W)
    df = np.stack([oracle.disp_to_float(f) for f in d16])
    assert np.array_equal(df, d16.astype(np.float32) * np.float32(0.0625))
    ref = reference(oracle, ("s16", W, H), df, Q_DENSE, hm)
    got = run_reproject_s16(d16, Q_DENSE, hm)
    assert same(got, ref)
    if hm:
        check_missing_counts(got, ref, (1, 2 if n // 2 != 0 else 1, None))
        run_reproject_s16(d16, Q_DENSE, True, pad_d=3, expect=ERR_ARG)
        assert same(run_reproject_s16(d16, Q_DENSE, True, pad_x=5), ref)  # only the map must be dense
    else:
        for pad_d, pad_x in ((3, 4), (1, 0)):
            assert same(run_reproject_s16(d16, Q_DENSE, False, pad_d, pad_x), ref), (pad_d, pad_x)


@pytest.mark.parametrize("hm", [False, True], ids=["plain", "missing"])
def test_reproject_special_values(oracle, hm):
    """NaN, +inf, +-0 (and -inf without handle_missing) in float input, and w == 0 exactly (d == 4
    with Q_ZERO_W): against the oracle, whose minimum skips NaN as k_min_f32 does."""
    for (W, H) in ((5, 3), (63, 7), (257, 5), (300, 9)):
        rng = np.random.default_rng(W + 1000 * H)
        disp, counts = frames_with_minima(rng, W, H, grid16=True)
        flat = disp.reshape(3, -1)
        n = W * H
        spec = [np.nan, np.inf, 0.0, -0.0, 4.0, 4.0] + ([] if hm else [-np.inf])
        for f in range(3):
            at = rng.choice(np.arange(1, n - 1), size=min(len(spec), n - 2), replace=False)
            at = at[(at != n // 2)]
            flat[f, at] = np.array(spec, np.float32)[:at.size]
        for name, Q in (("dense", Q_DENSE), ("zero_w", Q_ZERO_W)):
            ref = np.stack([oracle.reproject(f, Q, hm) for f in disp])
            if name == "zero_w":
                assert np.isinf(ref[disp == 4.0]).any()
            got = run_reproject_f32(disp, Q, hm, 3, 4)
            assert same(got, ref), (W, H, name)
            host = np.stack([run_reproject_host(disp[f], Q, hm) for f in range(3)])
            assert same(host, ref), (W, H, name)
            if hm:
                check_missing_counts(got, ref, counts)
        # d == 4 on the int16 entry: 64 / 16
        d16 = np.clip(np.nan_to_num(disp, nan=1.0, posinf=2.0, neginf=3.0) * 16, -32768, 32767).astype(np.int16)
        ref = np.stack([oracle.reproject(oracle.disp_to_float(f), Q_ZERO_W, hm) for f in d16])
        assert same(run_reproject_s16(d16, Q_ZERO_W, hm), ref)


def test_reproject_refusals():
    b = torch.full((4096,), float(FSENT), dtype=torch.float32, device="cuda")
    p, Q = b.data_ptr(), qptr(Q_DENSE)
    L = lib()
    for fn in (L.sdr_reproject_device, L.sdr_disp16_reproject_device):
        assert fn(p, 8, 4, 7, Q, 0, p, 24, 1, None) == ERR_ARG   # disp_stride < width
        assert fn(p, 8, 4, 8, Q, 0, p, 23, 1, None) == ERR_ARG   # xyz_stride < 3 * width
        assert fn(p, 8, 4, 8, Q, 0, p, 24, 0, None) == ERR_ARG   # no frames
        assert fn(p, 0, 4, 8, Q, 0, p, 24, 1, None) == ERR_ARG
        assert fn(None, 8, 4, 8, Q, 0, p, 24, 1, None) == ERR_ARG
        assert fn(p, 8, 4, 8, None, 0, p, 24, 1, None) == ERR_ARG
    torch.cuda.synchronize()
    assert (b.cpu().numpy() == FSENT).all()


# ---- convertTo(CV_32F, 1/16) ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 256 * 4096 + 3])
def test_disp16_to_float(n):
    """n across the grid-stride loop (4096 workgroups of 256): every value once, nothing past n."""
    rng = np.random.default_rng(n + 1)
    d = rng.integers(-32768, 32768, n + 5).astype(np.int16)
    d[:min(n, 2)] = [-32768, 32767][:min(n, 2)]
    if n > 2:
        d[n - 1] = -32768
    out = torch.full((n + TAIL,), float(FSENT), dtype=torch.float32, device="cuda")
    d_in = dev(d)
    rc = lib().sdr_disp16_to_float_device(d_in.data_ptr(), out.data_ptr(), n, _cstream(0))
    torch.cuda.synchronize()
    assert rc == 0, lib().sdr_last_error()
    out = out.cpu().numpy()
    assert (out[n:] == FSENT).all()
    want = d[:n].astype(np.float32) * np.float32(0.0625)
    assert np.array_equal(out[:n].view(np.uint32), want.view(np.uint32))
    assert lib().sdr_disp16_to_float_device(None, 1, 1, None) == ERR_ARG


# ---- BGR2GRAY, INTER_AREA 0.5x --------------------------------------------------------------------

PRE_SIZES = [(2, 2), (254, 4), (258, 6), (90, 64)]


def run_rows_u8(fn, src, W, H, sstride, dshape, dstride, expect=0):
    """fn(d_src, W, H, sstride, d_dst, dstride, F, stream) on (F, rows, sstride) bytes -> the
    (F, dh, dw) result, after checking the sentinel in the destination's padding and tail."""
    F = src.shape[0]
    dh, dw = dshape
    dst = torch.full((F * dh * dstride + TAIL,), SENT, dtype=torch.uint8, device="cuda")
    d_src = dev(src)
    rc = fn(d_src.data_ptr(), W, H, sstride, dst.data_ptr(), dstride, F, _cstream(0))
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib().sdr_last_error())
    dst = dst.cpu().numpy()
    if rc:
        assert (dst == SENT).all()
        return None
    assert (dst[F * dh * dstride:] == SENT).all()
    dst = dst[:F * dh * dstride].reshape(F, dh, dstride)
    assert (dst[:, :, dw:] == SENT).all()
    return np.ascontiguousarray(dst[:, :, :dw])


@pytest.mark.parametrize("pads", [(0, 0), (7, 5)], ids=["dense", "padded"])
@pytest.mark.parametrize("size", PRE_SIZES, ids=[f"{w}x{h}" for w, h in PRE_SIZES])
def test_bgr2gray_and_area_half(oracle, size, pads):
    """Three frames, dense and padded rows: the oracle and the plain integer formulas."""
    W, H = size
    ps, pd = pads
    F = 3
    rng = np.random.default_rng(W * 3 + H + ps)
    bgr = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    bgr[0, 0, 0] = 255  # (the largest sum: 1868 + 9617 + 4899 = 2^14 exactly)
    bgr[0, -1, -1] = 0
    src = rng.integers(0, 256, (F, H, 3 * W + ps), dtype=np.uint8)
    src[:, :, :3 * W] = bgr.reshape(F, H, 3 * W)
    gray = run_rows_u8(lib().sdr_bgr2gray_device, src, W, H, 3 * W + ps, (H, W), W + pd)
    for f in range(F):
        ref = oracle.bgr2gray(bgr[f])
        assert np.array_equal(ref, C.bgr2gray_int(bgr[f]))
        assert np.array_equal(gray[f], ref), f
    gsrc = rng.integers(0, 256, (F, H, W + ps), dtype=np.uint8)
    gsrc[:, :, :W] = gray
    small = run_rows_u8(lib().sdr_resize_area_half_device, gsrc, W, H, W + ps, (H // 2, W // 2), W // 2 + pd)
    for f in range(F):
        ref = oracle.resize_area_half(gray[f])
        assert np.array_equal(ref, C.area_half_int(gray[f]))
        assert np.array_equal(small[f], ref), f


def test_pre_step_refusals():
    src = np.zeros((1, 6, 24), np.uint8)
    R, G = lib().sdr_resize_area_half_device, lib().sdr_bgr2gray_device
    run_rows_u8(R, src, 7, 6, 24, (3, 3), 8, expect=ERR_SIZE)   # odd width
    run_rows_u8(R, src, 8, 5, 24, (2, 4), 8, expect=ERR_SIZE)   # odd height
    run_rows_u8(R, src, 8, 6, 7, (3, 4), 8, expect=ERR_ARG)     # stride < width
    run_rows_u8(R, src, 8, 6, 24, (3, 4), 3, expect=ERR_ARG)    # dst_stride < width / 2
    run_rows_u8(G, src, 8, 6, 23, (6, 8), 8, expect=ERR_ARG)    # bgr_stride < 3 * width
    run_rows_u8(G, src, 8, 6, 24, (6, 8), 7, expect=ERR_ARG)    # gray_stride < width
    b = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert R(b.data_ptr(), 8, 6, 8, b.data_ptr(), 4, 0, None) == ERR_ARG
    assert G(None, 8, 6, 24, b.data_ptr(), 8, 1, None) == ERR_ARG
