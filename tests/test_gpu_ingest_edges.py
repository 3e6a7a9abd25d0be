"""The ingest entry points (sdr_rectify.hip) at their borders and strides, BIT FOR BIT against
oracle/rectify_oracle.c, on the calibrations of ingest_cases.py: maps whose taps leave the source
on every side (sx == -1, sx == W - 1, sy == -1, sy == H - 1, fully outside), odd sizes, W == 2,
every output selection of sdr_rectify_sbs_device, padded rows and frame strides with sentinel-filled
padding, the refusals, and ndist 0 / 4 / 5 / 8 / 12 / 14 with P as 3 x 3 and 3 x 4.  The shift
calibrations are also checked against their closed form (plain numpy, no oracle).
test_ingest_cases_cpu.py proves, without a GPU, that the cases hold the classes they claim.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ingest_cases as C  # noqa: E402
from stereo_depth_ruler_amd._lib import SDRError, lib  # noqa: E402
from stereo_depth_ruler_amd.rectify import StereoRectifier, initUndistortRectifyMap  # noqa: E402
from stereo_depth_ruler_amd.sgbm import _cstream  # noqa: E402

ERR_ARG, ERR_SIZE, ERR_TYPE = -1, -4, -5
SENT = 0xA5
TAIL = 64
OUTS = ("left", "right", "small_left", "small_right")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def ids(sizes):
    return [f"{w}x{h}" for w, h in sizes]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def sentinel(n):
    return torch.full((n,), SENT, dtype=torch.uint8, device="cuda")


def rectifier(case):
    r = StereoRectifier(C.config(case))
    assert lib().sdr_rectifier_set_stream(r._h, _cstream(0)) == 0
    return r


def eye_of(frames, case, f, eye):
    return np.ascontiguousarray(frames[f, :, eye * case.W:(eye + 1) * case.W])


_REF = {}


def sbs_reference(oracle, case):
    """Per frame and eye: the oracle's rectified BGR and, for even sizes, the half-size gray
    (remap -> BGR2GRAY -> INTER_AREA 0.5x); computed once per case."""
    if case.id not in _REF:
        frames = C.sbs_frames(case.W, case.H)
        even = case.W % 2 == 0 and case.H % 2 == 0
        ref = {k: [] for k in OUTS}
        for f in range(frames.shape[0]):
            for eye, key in ((0, "left"), (1, "right")):
                m1, m2 = C.oracle_maps(oracle, case, eye)
                rect = oracle.remap_bilinear(eye_of(frames, case, f, eye), m1, m2)
                ref[key].append(rect)
                if even:
                    ref["small_" + key].append(oracle.resize_area_half(oracle.bgr2gray(rect)))
        _REF[case.id] = {k: np.stack(v) for k, v in ref.items() if v}
    return _REF[case.id]


def run_sbs(r, case, want, stride=None, fstride=None, nframes=None, expect=0):
    """sdr_rectify_sbs_device through the raw ABI on ingest_cases' frames: `want` names the outputs
    requested.  Every requested output is a sentinel-filled buffer with TAIL bytes past its end;
    returns {name: array} after asserting the status and the tails."""
    W, H = case.W, case.H
    frames = C.sbs_frames(W, H)
    F = frames.shape[0] if nframes is None else nframes
    stride = 6 * W if stride is None else stride
    fstride = stride * H if fstride is None else fstride
    rows = max(stride, 6 * W)
    host = np.random.default_rng(7).integers(0, 256, (frames.shape[0], max(fstride, rows * H)), dtype=np.uint8)
    for f in range(frames.shape[0]):
        for y in range(H):
            host[f, y * rows:y * rows + 6 * W] = frames[f, y].reshape(-1)
    src = dev(host)
    shapes = {"left": (F, H, W, 3), "right": (F, H, W, 3), "small_left": (F, H // 2, W // 2),
              "small_right": (F, H // 2, W // 2)}
    bufs = {k: sentinel(max(int(np.prod(shapes[k])), 0) + TAIL) for k in want}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None  # noqa: E731
    rc = lib().sdr_rectify_sbs_device(r._h, src.data_ptr(), stride, fstride, F, ptr("left"), ptr("right"),
                                      ptr("small_left"), ptr("small_right"))
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib().sdr_last_error())
    out = {}
    for k, b in bufs.items():
        b = b.cpu().numpy()
        n = int(np.prod(shapes[k])) if F > 0 else 0
        assert (b[n:] == SENT).all(), f"{k}: wrote past its end"
        if rc:
            assert (b == SENT).all(), f"{k}: written by a refused call"
        else:
            out[k] = b[:n].reshape(shapes[k])
    return out


# ---- maps -------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", C.SIZES, ids=ids(C.SIZES))
def test_maps_bit_exact_every_case(oracle, size):
    """ndist 0, 4, 5, 8, 12 and 14 on either eye, P as 3 x 3 (shift) and 3 x 4 (zoom), through the
    stand-alone entry and through the rectifier."""
    for case in C.cases_of(*size):
        r = StereoRectifier(C.config(case))
        for eye in (0, 1):
            ref1, ref2 = C.oracle_maps(oracle, case, eye)
            K, D, R, P = case.eyes[eye]
            for dist in ((D, None) if D.size == 0 else (D,)):
                g1, g2 = initUndistortRectifyMap(K, dist, R, P, (case.W, case.H))
                assert np.array_equal(g1, ref1) and np.array_equal(g2, ref2), (case.id, eye)
            h1, h2 = r.maps(eye)
            assert np.array_equal(h1, ref1) and np.array_equal(h2, ref2), (case.id, eye)
        r.close()


def test_map_refusals():
    W, H = 38, 24
    K, D, R, P = C.zoom_eye(W, H, 14, C.ANGLE)
    for bad_d, bad_p in ((np.r_[D[:12], 0.01, 0.0], P), (np.r_[D[:12], 0.0, -0.02], P), (D[:3], P),
                         (D, P[:, :2]), (D[:1], P), (D[:13], P)):
        with pytest.raises(SDRError) as e:
            initUndistortRectifyMap(K, bad_d, R, bad_p, (W, H))
        assert e.value.code == ERR_ARG
    # the same through the rectifier, on either eye
    good = C.cases_of(W, H)[2]
    for eye in (0, 1):
        for bad in (np.r_[D[:12], 0.01, 0.0], D[:3]):
            cfg = C.config(good)
            setattr(cfg, "distCoeffsLeft" if eye == 0 else "distCoeffsRight", bad)
            with pytest.raises(SDRError) as e:
                StereoRectifier(cfg)
            assert e.value.code == ERR_ARG
    cfg = C.config(good)
    cfg.P1, cfg.P2 = cfg.P1[:, :2], cfg.P2[:, :2]
    with pytest.raises(SDRError) as e:
        StereoRectifier(cfg)
    assert e.value.code == ERR_ARG
    # 14 coefficients with a zero tilt are the 12-coefficient model
    m = initUndistortRectifyMap(K, D, R, P, (W, H))
    n = initUndistortRectifyMap(K, D[:12], R, P, (W, H))
    assert np.array_equal(m[0], n[0]) and np.array_equal(m[1], n[1])


# ---- sdr_rectify_sbs_device ---------------------------------------------------------------------

ODD_TREATMENT = C.SIZES_ODD + [(2, 2)]


@pytest.mark.parametrize("size", ODD_TREATMENT, ids=ids(ODD_TREATMENT))
def test_sbs_bgr_only(oracle, size):
    """Odd sizes (2 x 2 blocks hanging over the right and bottom edges), and W == 2: the BGR
    outputs alone, both eyes; a small output of an odd size is refused."""
    for case in C.cases_of(*size):
        r = rectifier(case)
        ref = sbs_reference(oracle, case)
        got = run_sbs(r, case, ("left", "right"))
        for k in ("left", "right"):
            assert np.array_equal(got[k], ref[k]), (case.id, k)
        if case.name.startswith("shift"):
            sign = 1 if case.name == "shift+" else -1
            frames = C.sbs_frames(case.W, case.H)
            for f in range(frames.shape[0]):
                for eye, k in ((0, "left"), (1, "right")):
                    assert np.array_equal(got[k][f], C.shift_closed_form(eye_of(frames, case, f, eye), sign))
        if case.W % 2 or case.H % 2:
            for want in (OUTS, ("small_left",), ("small_right",), ("left", "small_right")):
                run_sbs(r, case, want, expect=ERR_SIZE)
        r.close()


SELECTIONS = (OUTS, ("small_left", "small_right"), ("right",), ("small_left",))


@pytest.mark.parametrize("size", C.SIZES_EVEN, ids=ids(C.SIZES_EVEN))
def test_sbs_output_selections(oracle, size):
    """Even sizes: all four outputs, the small pair, the right eye's BGR alone and the left eye's
    small alone -- what is requested is bit-exact (remap, then BGR2GRAY, then INTER_AREA 0.5x, per
    frame and eye), and nothing else is written."""
    for case in C.cases_of(*size):
        r = rectifier(case)
        ref = sbs_reference(oracle, case)
        for want in SELECTIONS:
            got = run_sbs(r, case, want)
            assert set(got) == set(want)
            for k in want:
                assert np.array_equal(got[k], ref[k]), (case.id, want, k)
        if case.name.startswith("shift"):
            sign = 1 if case.name == "shift+" else -1
            frames = C.sbs_frames(case.W, case.H)
            got = run_sbs(r, case, OUTS)
            for f in range(frames.shape[0]):
                for eye, k in ((0, "left"), (1, "right")):
                    rect = C.shift_closed_form(eye_of(frames, case, f, eye), sign)
                    assert np.array_equal(got[k][f], rect)
                    assert np.array_equal(got["small_" + k][f], C.area_half_int(C.bgr2gray_int(rect)))
        r.close()


@pytest.mark.parametrize("size", C.SIZES, ids=ids(C.SIZES))
def test_sbs_padded_rows_and_frames(oracle, size):
    """sbs_stride = 6 W + 5 (rows that start at odd addresses) and a frame stride past stride * H:
    the dense call's results, and no byte past any output's end."""
    W, H = size
    even = W % 2 == 0 and H % 2 == 0
    want = OUTS if even else ("left", "right")
    for case in C.cases_of(W, H)[1:4]:  # shift-, and two zoom pairs
        r = rectifier(case)
        ref = sbs_reference(oracle, case)
        stride = 6 * W + 5
        got = run_sbs(r, case, want, stride=stride, fstride=stride * H + 11)
        for k in want:
            assert np.array_equal(got[k], ref[k]), (case.id, k)
        # one frame: the frame stride is not read
        got = run_sbs(r, case, want, stride=stride, fstride=0, nframes=1)
        for k in want:
            assert np.array_equal(got[k][0], ref[k][0]), (case.id, k)
        r.close()


def test_sbs_refusals():
    case = C.cases_of(38, 24)[2]
    r = rectifier(case)
    W, H = case.W, case.H
    run_sbs(r, case, OUTS, nframes=0, expect=ERR_ARG)
    run_sbs(r, case, OUTS, nframes=-1, expect=ERR_ARG)
    run_sbs(r, case, OUTS, stride=6 * W - 1, fstride=6 * W * H, expect=ERR_ARG)
    run_sbs(r, case, OUTS, stride=6 * W + 5, fstride=(6 * W + 5) * H - 1, expect=ERR_ARG)
    buf = sentinel(64)
    assert lib().sdr_rectify_sbs_device(r._h, None, 6 * W, 6 * W * H, 1, buf.data_ptr(), None, None, None) == ERR_ARG
    assert lib().sdr_rectify_sbs_device(None, buf.data_ptr(), 6 * W, 6 * W * H, 1, buf.data_ptr(), None, None,
                                        None) == ERR_ARG
    r.close()
    # an eye one pixel wide: the 6-byte span needs two
    K, D, R, P = C.shift_eye(1, 4, 1)
    thin = C._case("thin", 1, 4, (K, D, R, P), (K, D, R, P))
    r = rectifier(thin)
    run_sbs(r, thin, ("left", "right"), expect=ERR_SIZE)
    r.close()


def test_rectify_sbs_torch_equals_raw_abi(oracle):
    """One frame of 2 * 66 x 10 through StereoRectifier.rectify_sbs (torch input, the live loop's
    call) against the raw ABI result and the oracle."""
    for case in C.cases_of(66, 10)[1:4]:
        r = rectifier(case)
        raw = run_sbs(r, case, OUTS, nframes=1)
        frame = torch.from_numpy(np.array(C.sbs_frames(case.W, case.H)[0])).cuda()
        out = r.rectify_sbs(frame)
        torch.cuda.synchronize()
        ref = sbs_reference(oracle, case)
        for k in OUTS:
            assert np.array_equal(out[k].cpu().numpy(), raw[k][0]), (case.id, k)
            assert np.array_equal(raw[k][0], ref[k][0]), (case.id, k)
        only_small = r.rectify_sbs(frame, bgr=False)
        assert set(only_small) == {"small_left", "small_right"}
        assert np.array_equal(only_small["small_right"].cpu().numpy(), ref["small_right"][0])
        r.close()


# ---- sdr_remap_bilinear_device -------------------------------------------------------------------

def padded(a, row_bytes, frame_bytes, rng):
    """(F, H, rowlen) uint8 frames laid out with padded rows and frames: (flat buffer, mask of the
    bytes that belong to the frames)."""
    F, H, n = a.shape
    buf = rng.integers(0, 256, F * frame_bytes, dtype=np.uint8)
    mask = np.zeros(F * frame_bytes, bool)
    for f in range(F):
        for y in range(H):
            o = f * frame_bytes + y * row_bytes
            buf[o:o + n] = a[f, y]
            mask[o:o + n] = True
    return buf, mask


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("size", [(37, 23), (64, 8), (130, 70)], ids=ids([(37, 23), (64, 8), (130, 70)]))
def test_remap_strided_batched(oracle, size, cn):
    """Three frames, a source of another size than the map, padded source and destination rows and
    frame strides past the frame: bit-exact, and the destination's padding keeps its sentinel."""
    dw, dh = size
    sw, sh = dw - 3, dh + 2
    F = 3
    rng = np.random.default_rng(dw * 7 + cn)
    for case in C.cases_of(dw, dh)[2:5]:
        for eye in (0, 1):
            m1, m2 = C.oracle_maps(oracle, case, eye)
            src = rng.integers(0, 256, (F, sh, sw * cn), dtype=np.uint8)
            sstride, sfstride = sw * cn + 7, (sw * cn + 7) * sh + 13
            dstride, dfstride = dw * cn + 9, (dw * cn + 9) * dh + 21
            sbuf, _ = padded(src, sstride, sfstride, rng)
            dmask = padded(np.zeros((F, dh, dw * cn), np.uint8), dstride, dfstride, rng)[1]
            dbuf = sentinel(F * dfstride + TAIL)
            d_src, d_m1, d_m2 = dev(sbuf), dev(m1), dev(m2.view(np.int16))
            rc = lib().sdr_remap_bilinear_device(d_src.data_ptr(), sw, sh, sstride, sfstride, cn,
                                                 d_m1.data_ptr(), d_m2.data_ptr(), dw, dh,
                                                 dbuf.data_ptr(), dstride, dfstride, F, _cstream(0))
            torch.cuda.synchronize()
            assert rc == 0, lib().sdr_last_error()
            got = dbuf.cpu().numpy()
            assert (got[F * dfstride:] == SENT).all() and (got[:F * dfstride][~dmask] == SENT).all()
            got = got[:F * dfstride][dmask].reshape((F, dh, dw) + ((3,) if cn == 3 else ()))
            for f in range(F):
                s = src[f].reshape((sh, sw) + ((3,) if cn == 3 else ()))
                assert np.array_equal(got[f], oracle.remap_bilinear(s, m1, m2)), (case.id, eye, f)


def test_remap_refusals():
    b = sentinel(4096)
    p = b.data_ptr()
    L = lib().sdr_remap_bilinear_device
    assert L(p, 8, 8, 8, 64, 2, p, p, 8, 8, p, 16, 128, 1, None) == ERR_TYPE
    assert L(p, 8, 8, 23, 64, 3, p, p, 8, 8, p, 24, 192, 1, None) == ERR_ARG
    assert L(p, 8, 8, 24, 64, 3, p, p, 8, 8, p, 23, 192, 1, None) == ERR_ARG
    assert L(p, 8, 8, 8, 64, 1, p, p, 8, 8, p, 8, 64, 0, None) == ERR_ARG
    assert L(p, 8, 8, 8, 64, 1, None, p, 8, 8, p, 8, 64, 1, None) == ERR_ARG
    torch.cuda.synchronize()
    assert (b.cpu().numpy() == SENT).all()


# ---- sdr_rectify_device --------------------------------------------------------------------------

@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("size", [(37, 23), (66, 10)], ids=ids([(37, 23), (66, 10)]))
def test_rectify_device_channels_and_one_eye(oracle, size, cn):
    """channels == 1 and 3, two frames; both eyes, then each eye alone (the other eye's pointers
    null): only the requested eye is written."""
    W, H = size
    F = 2
    rng = np.random.default_rng(W + cn)
    shape = (F, H, W) + ((3,) if cn == 3 else ())
    n = int(np.prod(shape))
    for case in C.cases_of(W, H)[2:4]:
        r = rectifier(case)
        imgs = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in (0, 1)]
        ref = [np.stack([oracle.remap_bilinear(imgs[e][f], *C.oracle_maps(oracle, case, e)) for f in range(F)])
               for e in (0, 1)]
        din = [dev(a) for a in imgs]
        for eyes in ((0, 1), (0,), (1,)):
            outs = [sentinel(n + TAIL), sentinel(n + TAIL)]
            a = [din[e].data_ptr() if e in eyes else None for e in (0, 1)]
            o = [outs[e].data_ptr() if e in eyes else None for e in (0, 1)]
            rc = lib().sdr_rectify_device(r._h, a[0], a[1], W * cn, W * H * cn, cn, F, o[0], o[1], W * cn,
                                          W * H * cn)
            torch.cuda.synchronize()
            assert rc == 0, lib().sdr_last_error()
            for e in (0, 1):
                got = outs[e].cpu().numpy()
                assert (got[n:] == SENT).all()
                if e in eyes:
                    assert np.array_equal(got[:n].reshape(shape), ref[e]), (case.id, eyes, e)
                else:
                    assert (got == SENT).all()
        # an input without an output (and the reverse) is an error, not a skipped eye
        out = sentinel(n + TAIL)
        assert lib().sdr_rectify_device(r._h, din[0].data_ptr(), din[1].data_ptr(), W * cn, W * H * cn, cn, F,
                                        out.data_ptr(), None, W * cn, W * H * cn) == ERR_ARG
        assert lib().sdr_rectify_device(r._h, din[0].data_ptr(), None, W * cn, W * H * cn, 2, F, out.data_ptr(),
                                        None, W * cn, W * H * cn) == ERR_TYPE
        r.close()
