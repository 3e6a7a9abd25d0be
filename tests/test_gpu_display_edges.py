"""The display entry points (sdr_display.hip) at their rounding, comparison and stride edges, BIT FOR
BIT against oracle/display_oracle.c on the frames of emit_cases.py: the first float of each of the
255 levels of the gamma map (numDisparities 16, 80, 128, 256) and of the depth map with its three
neighbours on either side, all 65 536 operand pairs of the overlay's addWeighted and of both EMAs,
the values on which the depth statistics compare (10000, 12000, the zeros, a denormal, NaN, the
infinities) in lane 0, lane 63, columns 255 and 256 and the last pixel, alone or as the only
candidate for the minimum or the maximum, 70 and 130 frames in one call (the statistics are read
back 64 frames at a time), range states that clamp, col0 on either side of the width, frames wider
than a block; padded strides on every entry that takes one, with NaN or a sentinel byte in the
padding; what restarts the EMA and what does not; and the refusals.  The C ABI is called directly
where the Python wrappers fix an argument.  test_emit_cases_cpu.py proves, without a GPU, that the
frames hold what they claim."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import emit_cases as E  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd._lib import lib  # noqa: E402

ERR_ARG, ERR_TYPE = -1, -5
SENT = E.SENT
TAIL = 64
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def sentinel(n):
    return torch.full((n,), SENT, dtype=torch.uint8, device="cuda")


def last_error():
    return lib().sdr_last_error().decode(errors="replace")


def display():
    d = sdr.Display()
    d._stream()  # the current torch stream: ordered with the copies around the calls
    return d


def lut_ptr(lut):
    return None if lut is None else lut.ctypes.data


def disp_raw(d, buf, W, H, stride, fstride, F, nd, expect=0):
    """sdr_show_disparity_map_device on a flat float buffer -> (F, H, W) u8."""
    src = dev(buf)
    out = sentinel(F * H * W + TAIL)
    rc = lib().sdr_show_disparity_map_device(d._h, src.data_ptr(), W, H, stride, fstride, F, nd, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, last_error())
    got = out.cpu().numpy()
    assert (got[F * H * W:] == SENT).all()
    return got[:F * H * W].reshape(F, H, W)


def depth_raw(d, x, zr=None, lut=None, coverage=False):
    """sdr_show_depth_map_device on x (F, H, W[, 3]) -> (bgr (F, H, W, 3), coverage list or None);
    zr: a CUDA float64 pair, updated in place."""
    ch = 3 if x.ndim == 4 else 1
    F, H, W = x.shape[:3]
    src = dev(x)
    out = sentinel(F * H * W * 3 + TAIL)
    pct = (ctypes.c_double * F)(*([-1.0] * F)) if coverage else None
    rc = lib().sdr_show_depth_map_device(d._h, src.data_ptr(), W, H, ch, F, None if zr is None else zr.data_ptr(),
                                         lut_ptr(lut), out.data_ptr(), pct)
    torch.cuda.synchronize()
    assert rc == 0, (rc, last_error())
    got = out.cpu().numpy()
    assert (got[F * H * W * 3:] == SENT).all()
    return got[:F * H * W * 3].reshape(F, H, W, 3), (list(pct) if coverage else None)


def zstate(v=E.ZR0):
    return torch.tensor(list(v), dtype=torch.float64, device="cuda")


_DEPTH_REF = {}


def depth_ref(oracle, key, x, lut, zr0=E.ZR0):
    """The oracle's show_depthMap sequence over the frames of x from the state zr0: images (EMA
    carried), the range state after every frame, depth_coverage of every 3-channel frame."""
    if key not in _DEPTH_REF:
        zr, prev, outs, states, cov = np.array(zr0), None, [], [], []
        for f in range(len(x)):
            prev = oracle.show_depth_map(x[f], zr, lut, prev)
            outs.append(prev)
            states.append(zr.tolist())
            if x.ndim == 4:
                cov.append(oracle.depth_coverage(x[f], 80))
        _DEPTH_REF[key] = (np.stack(outs), states, cov)
    return _DEPTH_REF[key]


# ---- thresholds -------------------------------------------------------------------------------------

@pytest.mark.parametrize("nd", E.NUM_DISP)
def test_gamma_level_thresholds(oracle, nd):
    """Every level's first float and its neighbours, then 0, -0, a denormal, numDisp, 2 numDisp, the
    infinities, NaN and -1, 300 pixels a row: device entry, host entry, and a second frame (the EMA
    of the frame with itself moved by one pixel)."""
    frame = E.gamma_frame(oracle, nd)
    H, W = frame.shape
    ref = oracle.show_disparity_map(frame, nd)
    two = np.stack([frame, np.roll(frame, 1, 1)])
    ref2 = oracle.show_disparity_map(two[1], nd, ref)
    got = disp_raw(display(), two.reshape(-1), W, H, W, W * H, 2, nd)
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref2)
    assert np.array_equal(display().show_disparity_map(np.array(frame), nd), ref)  # host-pointer ABI


def test_depth_level_thresholds(oracle):
    """The same for show_depthMap with a table that shows the level, one and three channels; the
    range state goes from {1000, 2000} to exactly {950, 2700}."""
    frame = E.depth_frame(oracle)
    zr = np.array(E.ZR0)
    ref = oracle.show_depth_map(frame, zr, E.IDENT)
    for x in (frame[None], np.stack([frame * 0 + 7, frame * 0 - 3, frame], -1)[None]):
        z = zstate()
        got, _ = depth_raw(display(), x, z, E.IDENT)
        assert np.array_equal(got[0], ref)
        assert z.cpu().numpy().tolist() == zr.tolist() == [950.0, 2700.0]
    # the handle's own state and the built-in TURBO table, host entry
    turbo = oracle.colormap_lut(oracle.COLORMAP_TURBO)
    assert np.array_equal(display().show_depth_map(np.array(frame)), oracle.show_depth_map(frame, np.array(E.ZR0), turbo))


# ---- every operand pair of addWeighted ----------------------------------------------------------------

def overlay_raw(d, vis, left_buf, lstride, lfstride, W, H, F, lut, want=("heat", "overlay"), left_null=False,
                expect=0):
    """sdr_disparity_overlay_device -> {name: (F, H, W, 3)}; outputs not wanted are passed NULL."""
    d_vis, d_left = dev(vis), dev(left_buf)
    n = F * H * W * 3
    bufs = {k: sentinel(max(n, 0) + TAIL) for k in want}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None  # noqa: E731
    rc = lib().sdr_disparity_overlay_device(d._h, d_vis.data_ptr(), None if left_null else d_left.data_ptr(),
                                            lstride, lfstride, W, H, F, lut_ptr(lut), ptr("heat"), ptr("overlay"))
    torch.cuda.synchronize()
    assert rc == expect, (rc, last_error())
    out = {}
    for k, b in bufs.items():
        b = b.cpu().numpy()
        if rc:
            assert (b == SENT).all(), f"{k}: written by a refused call"
        else:
            assert (b[n:] == SENT).all(), f"{k}: wrote past its end"
            out[k] = b[:n].reshape(F, H, W, 3)
    return out


def test_overlay_every_operand_pair(oracle):
    vis, left = E.overlay_pairs()
    heat = oracle.apply_colormap(vis, E.IDENT)
    ref = oracle.add_weighted(oracle.resize_area_half_bgr(left), 0.7, heat, 0.3)
    got = overlay_raw(display(), vis, left.reshape(-1), 512 * 3, 0, 256, 256, 1, E.IDENT)
    assert np.array_equal(got["heat"][0], heat) and np.array_equal(got["overlay"][0], ref)


def test_disparity_ema_every_operand_pair(oracle):
    x = E.ema_disp_frames(oracle)
    first = oracle.show_disparity_map(x[0], 80)
    second = oracle.show_disparity_map(x[1], 80, first)
    got = disp_raw(display(), x.reshape(-1), 256, 256, 256, 256 * 256, 2, 80)
    assert np.array_equal(got[0], first) and np.array_equal(got[1], second)
    d = display()  # one call a frame: the history is read back from the handle
    assert np.array_equal(disp_raw(d, x[0].reshape(-1), 256, 256, 256, 0, 1, 80)[0], first)
    assert np.array_equal(disp_raw(d, x[1].reshape(-1), 256, 256, 256, 0, 1, 80)[0], second)


def test_depth_ema_every_operand_pair(oracle):
    x = E.ema_depth_frames(oracle)
    ref, states, _ = depth_ref(oracle, "ema", x, E.IDENT)
    z = zstate()
    got, _ = depth_raw(display(), x, z, E.IDENT)
    assert np.array_equal(got, ref) and z.cpu().numpy().tolist() == states[-1]
    d, z = display(), zstate()
    for f in range(2):
        got, _ = depth_raw(d, x[f:f + 1], z, E.IDENT)
        assert np.array_equal(got[0], ref[f]) and z.cpu().numpy().tolist() == states[f]


# ---- the comparisons of the depth statistics -----------------------------------------------------------

def coverage_raw(d, x, col0):
    F, H, W = x.shape[:3]
    src = dev(x)
    pct = (ctypes.c_double * F)(*([-1.0] * F))
    rc = lib().sdr_depth_coverage_device(d._h, src.data_ptr(), W, H, F, col0, pct)
    assert rc == 0, (rc, last_error())
    return list(pct)


def test_compare_values_at_wave_and_block_ends(oracle):
    """130 frames of 2 x 300 in one call: each compare value at lane 0, lane 63, column 255, column
    256 and the last pixel, as the only candidate for the minimum or the maximum and as the only
    valid Z (hi == lo: 1000 / 2000).  Images, the final range state and all 130 coverages; then
    frame by frame on one handle, the state after every frame."""
    x = E.zcmp_frames()
    turbo = oracle.colormap_lut(oracle.COLORMAP_TURBO)
    ref, states, cov = depth_ref(oracle, "zcmp", x, turbo)
    z = zstate()
    got, pct = depth_raw(display(), x, z, None, coverage=True)
    assert pct == cov
    assert z.cpu().numpy().tolist() == states[-1]
    assert np.array_equal(got, ref)
    assert coverage_raw(display(), x, 0) == [oracle.depth_coverage(x[f], 0) for f in range(len(x))]
    d, z = display(), zstate()
    for f in range(len(x)):
        got, pct = depth_raw(d, x[f:f + 1], z, None, coverage=True)
        assert z.cpu().numpy().tolist() == states[f], (f, E.ZVALS[f // 10])
        assert pct == [cov[f]] and np.array_equal(got[0], ref[f]), (f, E.ZVALS[f // 10])
    # Z alone (channels == 1) takes the same decisions
    zonly = np.ascontiguousarray(x[..., 2])
    z1 = zstate()
    got, _ = depth_raw(display(), zonly, z1, None)
    assert np.array_equal(got, ref) and z1.cpu().numpy().tolist() == states[-1]


def test_seventy_frames_in_one_call(oracle):
    """70 frames of 3 x 90 (two without a valid Z, one with exactly one): the statistics of frames
    64..69 come back in a second chunk."""
    x = E.many_frames()
    ref, states, cov = depth_ref(oracle, "many", x, E.IDENT)
    assert cov[64:] != cov[:6] and len(set(cov[64:])) > 1  # the second chunk is not the first again
    z = zstate()
    got, pct = depth_raw(display(), x, z, E.IDENT, coverage=True)
    assert pct == cov
    assert z.cpu().numpy().tolist() == states[-1] and np.array_equal(got, ref)
    for col0 in (0, 85):
        assert coverage_raw(display(), x, col0) == [oracle.depth_coverage(x[f], col0) for f in range(70)]
    d, z = display(), zstate()
    for f in range(70):
        got, pct = depth_raw(d, x[f:f + 1], z, E.IDENT, coverage=True)
        assert z.cpu().numpy().tolist() == states[f], f
        assert pct == [cov[f]] and np.array_equal(got[0], ref[f]), f


@pytest.mark.parametrize("case", E.CLAMP_STATES, ids=["near-10000", "near-0"])
def test_range_states_that_clamp(oracle, case):
    state, (lo, hi) = case
    frame = E.clamp_frame(lo, hi)
    zr = np.array(state)
    ref = oracle.show_depth_map(frame, zr, E.IDENT)
    z = zstate(state)
    got, _ = depth_raw(display(), frame[None], z, E.IDENT)
    assert z.cpu().numpy().tolist() == zr.tolist()
    assert np.array_equal(got[0], ref)
    zh = np.array(state)  # the host entry carries the state in and out
    assert np.array_equal(display().show_depth_map(np.array(frame), zrange=zh),
                          oracle.show_depth_map(frame, np.array(state), oracle.colormap_lut(oracle.COLORMAP_TURBO)))
    assert zh.tolist() == zr.tolist()


@pytest.mark.parametrize("W", E.COL0_W)
def test_coverage_col0_against_width(oracle, W):
    d = display()
    for H in (1, 2, 3):
        x = E.coverage_frame(W, H)
        for col0 in E.col0_list(W):
            ref = oracle.depth_coverage(x, col0)
            assert coverage_raw(d, x[None], col0) == [ref], (W, H, col0)
            pct = ctypes.c_double(-1.0)
            assert lib().sdr_depth_coverage(d._h, x.ctypes.data, W, H, col0, ctypes.byref(pct)) == 0
            assert pct.value == ref, (W, H, col0)


# ---- strides ----------------------------------------------------------------------------------------

SW, SH, SF = 257, 4, 3


def stride_disp():
    rng = np.random.default_rng(257)
    x = rng.uniform(-5, 90, (SF, SH, SW)).astype(F32)
    x[:, 0, :6] = [np.nan, np.inf, -np.inf, 0.0, 80.0, 1e-3]
    return x


def disp_sequence(oracle, x, nd=80):
    out, prev = [], None
    for f in range(len(x)):
        prev = oracle.show_disparity_map(x[f], nd, prev)
        out.append(prev)
    return np.stack(out)


def test_disparity_map_padded_rows_and_frames(oracle):
    """stride = W + 5 and frame_stride = stride * H + 11 elements, NaN in the padding."""
    x = stride_disp()
    ref = disp_sequence(oracle, x)
    stride = SW + 5
    fstride = stride * SH + 11
    buf = np.r_[E.padded_f32(x, stride, fstride), np.full(TAIL, np.nan, F32)]
    assert np.array_equal(disp_raw(display(), buf, SW, SH, stride, fstride, SF, 80), ref)
    # one frame: the frame stride is not read
    assert np.array_equal(disp_raw(display(), buf, SW, SH, stride, 0, 1, 80)[0], ref[0])


def test_disparity_map_host_padded_in_and_out(oracle):
    x = stride_disp()
    ref = disp_sequence(oracle, x)
    stride, ostride = SW + 5, SW + 9
    d = display()
    for f in range(SF):
        buf = E.padded_f32(x[f:f + 1], stride, stride * SH)
        out = np.full(SH * ostride, SENT, np.uint8)
        assert lib().sdr_show_disparity_map(d._h, buf.ctypes.data, SW, SH, stride, 80, out.ctypes.data, ostride) == 0
        out = out.reshape(SH, ostride)
        assert np.array_equal(out[:, :SW], ref[f]) and (out[:, SW:] == SENT).all()


def left_views(seed=6):
    rng = np.random.default_rng(seed)
    vis = rng.integers(0, 256, (SF, SH, SW), dtype=np.uint8)
    left = rng.integers(0, 256, (SF, 2 * SH, 2 * SW, 3), dtype=np.uint8)
    return vis, left


def overlay_ref(oracle, vis, left, lut):
    heat = np.stack([oracle.apply_colormap(v, lut) for v in vis])
    ov = np.stack([oracle.add_weighted(oracle.resize_area_half_bgr(left[f]), 0.7, heat[f], 0.3)
                   for f in range(len(vis))])
    return heat, ov


def test_overlay_padded_left_rows_and_frames(oracle):
    """left_stride = 6 W + 7 bytes with frames 13 bytes further apart than their rows, and with
    left_frame_stride = 0 (frames dense at the padded row length); a sentinel byte in the padding."""
    vis, left = left_views()
    jet = oracle.colormap_lut(oracle.COLORMAP_JET)
    heat, ov = overlay_ref(oracle, vis, left, jet)
    rows = left.reshape(SF, 2 * SH, 6 * SW)
    ls = 6 * SW + 7
    for lfs, passed in ((ls * 2 * SH + 13, ls * 2 * SH + 13), (ls * 2 * SH, 0)):
        buf = np.r_[E.padded_u8(rows, ls, lfs), np.full(TAIL, SENT, np.uint8)]
        got = overlay_raw(display(), vis, buf, ls, passed, SW, SH, SF, None)
        assert np.array_equal(got["heat"], heat) and np.array_equal(got["overlay"], ov), passed
    # the host entry, one frame, padded left rows
    d = display()
    buf = E.padded_u8(rows[1:2], ls, ls * 2 * SH)
    h, o = np.full((SH, SW, 3), SENT, np.uint8), np.full((SH, SW, 3), SENT, np.uint8)
    assert lib().sdr_disparity_overlay(d._h, vis[1].ctypes.data, buf.ctypes.data, ls, SW, SH, h.ctypes.data,
                                       o.ctypes.data) == 0
    assert np.array_equal(h, heat[1]) and np.array_equal(o, ov[1])


def test_heat_alone_overlay_alone_and_both(oracle):
    vis, left = left_views(8)
    lut = np.random.default_rng(8).integers(0, 256, (256, 3), dtype=np.uint8)
    heat, ov = overlay_ref(oracle, vis, left, lut)
    flat, d = left.reshape(-1), display()
    args = (6 * SW, 0, SW, SH, SF, lut)
    got = overlay_raw(d, vis, flat, *args, want=("heat",))
    assert set(got) == {"heat"} and np.array_equal(got["heat"], heat)
    got = overlay_raw(d, vis, flat, *args, want=("heat",), left_null=True)  # no left view: none is read
    assert np.array_equal(got["heat"], heat)
    got = overlay_raw(d, vis, flat, *args, want=("overlay",))
    assert set(got) == {"overlay"} and np.array_equal(got["overlay"], ov)
    got = overlay_raw(d, vis, flat, *args)
    assert np.array_equal(got["heat"], heat) and np.array_equal(got["overlay"], ov)
    # host entry: either output alone
    h, o = np.full((SH, SW, 3), SENT, np.uint8), np.full((SH, SW, 3), SENT, np.uint8)
    jh, jo = overlay_ref(oracle, vis[:1], left[:1], oracle.colormap_lut(oracle.COLORMAP_JET))
    L = lib().sdr_disparity_overlay
    assert L(d._h, vis[0].ctypes.data, left[0].ctypes.data, 6 * SW, SW, SH, h.ctypes.data, None) == 0
    assert L(d._h, vis[0].ctypes.data, left[0].ctypes.data, 6 * SW, SW, SH, None, o.ctypes.data) == 0
    assert np.array_equal(h, jh[0]) and np.array_equal(o, jo[0])


# ---- state --------------------------------------------------------------------------------------------

def test_what_restarts_the_ema(oracle):
    x = stride_disp()
    small = np.ascontiguousarray(x[:, :3, :200])
    plain = [oracle.show_disparity_map(x[f], 80) for f in range(SF)]
    d, other = display(), display()

    def show(h, a):
        return disp_raw(h, a.reshape(-1), a.shape[1], a.shape[0], a.shape[1], 0, 1, 80)[0]

    assert np.array_equal(show(d, x[0]), plain[0])
    assert np.array_equal(show(other, small[0]), oracle.show_disparity_map(small[0], 80))  # another handle, another size
    blended = oracle.show_disparity_map(x[1], 80, plain[0])
    assert np.array_equal(show(d, x[1]), blended) and not np.array_equal(blended, plain[1])
    assert np.array_equal(show(d, small[2]), oracle.show_disparity_map(small[2], 80))  # a size change restarts
    assert np.array_equal(show(d, x[2]), plain[2])                                     # and so does the way back
    assert np.array_equal(show(d, x[0]), oracle.show_disparity_map(x[0], 80, plain[2]))
    d.reset()
    assert np.array_equal(show(d, x[1]), plain[1])
    # the same for the depth map's history, whose range state a size change leaves alone
    z = E.many_frames()
    ref, states, _ = depth_ref(oracle, "many", z, E.IDENT)
    d, zr = display(), zstate()
    for f in range(2):
        assert np.array_equal(depth_raw(d, z[f:f + 1], zr, E.IDENT)[0][0], ref[f])
    cut = np.ascontiguousarray(z[2:3, :2, :50])
    zo = np.array(states[1])
    assert np.array_equal(depth_raw(d, cut, zr, E.IDENT)[0][0], oracle.show_depth_map(cut[0], zo, E.IDENT))
    assert zr.cpu().numpy().tolist() == zo.tolist()


def test_host_coverage_between_depth_maps_changes_nothing(oracle):
    z = E.many_frames()
    turbo = oracle.colormap_lut(oracle.COLORMAP_TURBO)
    ref, states, cov = depth_ref(oracle, "many-turbo", z, turbo)
    d = display()  # the handle's own range state, host entries
    out0, c0 = d.show_depth_map(np.array(z[0]), coverage=True)
    pct = ctypes.c_double(-1.0)
    other = E.coverage_frame(300, 3)
    assert lib().sdr_depth_coverage(d._h, other.ctypes.data, 300, 3, 80, ctypes.byref(pct)) == 0
    assert pct.value == oracle.depth_coverage(other, 80)
    assert lib().sdr_depth_coverage(d._h, z[7].ctypes.data, 90, 3, 0, ctypes.byref(pct)) == 0
    assert pct.value == oracle.depth_coverage(z[7], 0)
    out1, c1 = d.show_depth_map(np.array(z[1]), coverage=True)
    assert np.array_equal(out0, ref[0]) and np.array_equal(out1, ref[1]) and [c0, c1] == cov[:2]
    out2 = d.show_depth_map(np.array(z[2]))
    assert np.array_equal(out2, ref[2])


# ---- refusals -----------------------------------------------------------------------------------------

def test_refusals(oracle):
    W, H, F = 40, 6, 2
    d = display()
    fl = torch.full((F * H * W * 3 + 64,), 5.0, dtype=torch.float32, device="cuda")
    u8 = sentinel(F * 4 * H * W * 3 + 64)
    out = sentinel(F * H * W * 3 + 64)
    p, q, o = fl.data_ptr(), u8.data_ptr(), out.data_ptr()
    pct = (ctypes.c_double * F)(-1.0, -1.0)
    L = lib()

    def refused(rc, code=ERR_ARG):
        assert rc == code, (rc, last_error())
        assert last_error()

    S = L.sdr_show_disparity_map_device
    for args in ((None, p, W, H, W, W * H, F, 80, o), (d._h, None, W, H, W, W * H, F, 80, o),
                 (d._h, p, W, H, W, W * H, F, 80, None), (d._h, p, 0, H, W, W * H, F, 80, o),
                 (d._h, p, W, -1, W, W * H, F, 80, o), (d._h, p, W, H, W, W * H, 0, 80, o),
                 (d._h, p, W, H, W - 1, W * H, F, 80, o)):
        refused(S(*args))
    D = L.sdr_show_depth_map_device
    refused(D(d._h, p, W, H, 2, F, None, None, o, pct), ERR_TYPE)
    assert "channels" in last_error()
    refused(D(d._h, p, W, H, 0, F, None, None, o, pct), ERR_TYPE)
    for args in ((None, p, W, H, 3, F, None, None, o, pct), (d._h, None, W, H, 3, F, None, None, o, pct),
                 (d._h, p, W, H, 3, F, None, None, None, pct), (d._h, p, 0, H, 3, F, None, None, o, pct),
                 (d._h, p, W, 0, 3, F, None, None, o, pct), (d._h, p, W, H, 3, -1, None, None, o, pct)):
        refused(D(*args))
    C = L.sdr_depth_coverage_device
    for args in ((None, p, W, H, F, 80, pct), (d._h, None, W, H, F, 80, pct), (d._h, p, W, H, F, 80, None),
                 (d._h, p, 0, H, F, 80, pct), (d._h, p, W, 0, F, 80, pct), (d._h, p, W, H, 0, 80, pct)):
        refused(C(*args))
    O = L.sdr_disparity_overlay_device
    for args in ((None, q, q, 6 * W, 0, W, H, F, None, o, o), (d._h, None, q, 6 * W, 0, W, H, F, None, o, o),
                 (d._h, q, q, 6 * W, 0, W, H, F, None, None, None),  # neither output
                 (d._h, q, None, 6 * W, 0, W, H, F, None, None, o),  # an overlay without a left view
                 (d._h, q, None, 6 * W, 0, W, H, F, None, o, o),
                 (d._h, q, q, 6 * W - 1, 0, W, H, F, None, o, o), (d._h, q, q, 6 * W, 0, 0, H, F, None, o, o),
                 (d._h, q, q, 6 * W, 0, W, 0, F, None, o, o), (d._h, q, q, 6 * W, 0, W, H, 0, None, o, o)):
        refused(O(*args))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and list(pct) == [-1.0, -1.0]
    # host entries
    hin = np.full(H * W * 3, 5.0, F32)
    hl = np.full(4 * H * W * 3, 7, np.uint8)
    ho = np.full(H * W * 3, SENT, np.uint8)
    hp, hq, hoo = hin.ctypes.data, hl.ctypes.data, ho.ctypes.data
    one = ctypes.c_double(-1.0)
    refused(L.sdr_show_disparity_map(d._h, hp, W, H, W - 1, 80, hoo, W))
    refused(L.sdr_show_disparity_map(d._h, hp, W, H, W, 80, hoo, W - 1))
    refused(L.sdr_show_disparity_map(d._h, None, W, H, W, 80, hoo, W))
    refused(L.sdr_show_disparity_map(d._h, hp, 0, H, W, 80, hoo, W))
    refused(L.sdr_show_depth_map(d._h, hp, W, H, 2, None, hoo, ctypes.byref(one)), ERR_TYPE)
    refused(L.sdr_show_depth_map(d._h, hp, W, H, 3, None, None, ctypes.byref(one)))
    refused(L.sdr_show_depth_map(d._h, hp, W, 0, 3, None, hoo, ctypes.byref(one)))
    refused(L.sdr_depth_coverage(d._h, hp, W, H, 80, None))
    refused(L.sdr_depth_coverage(d._h, hp, -1, H, 80, ctypes.byref(one)))
    refused(L.sdr_disparity_overlay(d._h, hq, hq, 6 * W - 1, W, H, hoo, hoo))
    refused(L.sdr_disparity_overlay(d._h, hq, None, 6 * W, W, H, hoo, hoo))
    refused(L.sdr_disparity_overlay(d._h, hq, hq, 6 * W, W, H, None, None))
    refused(L.sdr_disparity_overlay(d._h, hq, hq, 6 * W, 0, H, hoo, hoo))
    assert (ho == SENT).all() and one.value == -1.0
    # a refused call leaves the history alone: the next frame is still the first
    x = E.gamma_frame(oracle, 80)
    assert np.array_equal(d.show_disparity_map(np.array(x), 80), oracle.show_disparity_map(x, 80))
