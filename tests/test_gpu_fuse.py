"""GPU: the ruler over time (sdr_fuse_disp*, csrc/sdr_fuse.hip) through every layer: every map and
record compared bit for bit with the numpy restatement (tests/fuse_ref.py), no pixel left out."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fuse_ref as FR  # noqa: E402
import plane_ref as PR  # noqa: E402
import ruler_ref as RR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import FuseParams, check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import FUSION_DTYPE, MEASUREMENT_DTYPE, PLANE_DTYPE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q
NAN, INF = np.float32(np.nan), np.float32(np.inf)
FRAMES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32]  # both sides of every frame capacity (4, 8, 16, 32)
LAYOUTS = ["dense", "row+1", "row+4", "offset"]
PX = 4  # csrc/sdr_fuse.hip, kFusePx: the most pixels a thread owns (two float, four or two int16), one vector access where aligned


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def stack_of(rng, F, H, W, dtype, tol=0.5):
    """Values on a grid that divides `tol` (ties, and values exactly tol apart), some invalid; float
    stacks also carry NaN, +-inf and +-0.0.  conf: 0..3 with NaNs."""
    if dtype == np.int16:
        v = rng.integers(-24, 64, (F, H, W)).astype(np.int16)  # 1/16 px: -1.5 .. 4 px around min_disp -1
        v[rng.random((F, H, W)) < 0.3] = 32
    else:
        v = (rng.integers(-8, 16, (F, H, W)) * np.float32(tol / 2)).astype(np.float32)
        u = rng.random((F, H, W))
        v[u < 0.04] = NAN
        v[(u >= 0.04) & (u < 0.06)] = INF
        v[(u >= 0.06) & (u < 0.08)] = -INF
        v[(u >= 0.08) & (u < 0.12)] = np.float32(-0.0)
        v[(u >= 0.12) & (u < 0.16)] = np.float32(0.0)
    conf = rng.integers(0, 4, (F, H, W)).astype(np.float32)
    conf[rng.random((F, H, W)) < 0.08] = NAN
    return v, conf


def on_device(stack, layout):
    """The stack as a CUDA tensor view (F, H, W) of the layout: dense; rows W + 1 apart (no vector
    alignment unless W + 1 is a multiple of a thread's pixels); rows W + 4 apart in frames of H + 1 rows (the
    alignment a dense stack of the width has, plus whole vectors of padding); dense from one element
    into an allocation."""
    F, H, W = stack.shape
    t = torch.from_numpy(np.ascontiguousarray(stack)).to(dev())
    if layout == "dense":
        return t
    if layout == "offset":
        buf = torch.zeros(F * H * W + 1, dtype=t.dtype, device=dev())
        buf[1:] = t.reshape(-1)
        view = buf[1:].view(F, H, W)
        assert view.data_ptr() % (PX * t.element_size()) == t.element_size()
        return view
    pad_w, pad_h = (1, 0) if layout == "row+1" else (4, 1)
    buf = torch.full((F, H + pad_h, W + pad_w), 7, dtype=t.dtype, device=dev())
    buf[:, :H, :W] = t
    view = buf[:, :H, :W]
    assert view.stride(1) == W + pad_w and (F == 1 or view.stride(0) == (H + pad_h) * (W + pad_w))
    return view


def host_outs(outs):
    torch.cuda.synchronize()
    fused, rec = outs[0].cpu().numpy()[0], outs[1].cpu().numpy().view(FUSION_DTYPE)[0]
    return fused, rec, outs[2].cpu().numpy(), outs[3].cpu().numpy()


def check_fuse(stack, conf=None, layout="dense", min_disp=-1.0, conf_min=0.0, **kw):
    """fuse_device on the layout == the restatement, every output on every bit."""
    r = sdr.Ruler(Q, min_disp=min_disp, conf_min=conf_min)
    d = on_device(stack, layout)
    c = torch.from_numpy(conf).to(dev()) if conf is not None else None
    got = host_outs(r.fuse_device(d, c, support=True, spread=True, **kw))
    want = FR.fuse(stack, conf, min_disp=min_disp, conf_min=conf_min, **kw)
    FR.assert_fusion_equal(got, want)
    return want


# ---- every frame count, element type, mode, with and without confidence ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("F", FRAMES)
def test_every_frame_count(F, dtype):
    rng = np.random.default_rng(17 * F + (dtype == np.int16))
    fused = 0
    for W, layout in ((68, "dense"), (67, "row+1"), (67, "dense"), (65, "row+4")):
        # 68 dense: every access a vector; 67 in rows of 68: vector loads, a tail, scalar stores;
        # 67 dense: all scalar; 65 in rows of 69: scalar loads
        v, conf = stack_of(rng, F, 5, W, dtype)
        for mode in (FR.MEAN, FR.MEDIAN):
            for c in (None, conf):
                want = check_fuse(v, c, layout, conf_min=1.0, tol=0.5, min_count=min(2, F), mode=mode)
                fused += int(want[1]["n_fused"])
    assert fused > 0


# ---- sizes around the vector, the wave and the workgroup's 1024 pixels; every layout ----
@pytest.mark.parametrize("H", [1, 2, 5])
@pytest.mark.parametrize("W", [1, 3, 4, 5, 63, 64, 65, 259])
def test_sizes_and_layouts(W, H):
    rng = np.random.default_rng(1000 * H + W)
    for i, layout in enumerate(LAYOUTS):
        for dtype in (np.float32, np.int16):
            F = (5, 3, 9, 2)[i]
            v, conf = stack_of(rng, F, H, W, dtype)
            check_fuse(v, conf, layout, conf_min=1.0, tol=0.5, min_count=2, mode=(FR.MEAN, FR.MEDIAN)[i % 2],
                       fill=NAN)


def test_several_workgroups_and_a_tail_row():
    """1024 pixels a workgroup: 259 x 17 is five of them, the last one part full."""
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.int16):
        v, conf = stack_of(rng, 6, 17, 259, dtype)
        check_fuse(v, conf, "row+1", conf_min=1.0, tol=0.5, min_count=3)  # rows of 260: the vector path
        check_fuse(v, None, "dense", tol=0.5, min_count=3, mode=FR.MEDIAN)


# ---- content ----
@pytest.mark.parametrize("F", [1, 4, 7, 32])
def test_content_edges(F):
    rng = np.random.default_rng(40 + F)
    H, W = 3, 24
    # all invalid: NaN, -inf, below min_disp, and a confidence map that refuses everything
    v = np.full((F, H, W), -2.0, np.float32)
    v[:, 0] = NAN
    v[:, 1, ::2] = -INF
    want = check_fuse(v, None, tol=1.0, min_count=1)
    assert want[1]["n_empty"] == H * W and (want[0] == -1.0).all()
    ok, conf = stack_of(rng, F, H, W, np.float32)
    want = check_fuse(ok, np.full_like(conf, NAN), tol=1.0, min_count=1, fill=NAN)
    assert want[1]["n_empty"] == H * W and np.isnan(want[0]).all()
    # every value equal (ties all the way: frame order decides every rank), +-0.0 among them
    for value in (np.float32(2.5), np.float32(-0.0), np.float32(0.0)):
        want = check_fuse(np.full((F, H, W), value, np.float32), None, tol=0.0, min_count=F)
        assert want[1]["n_fused"] == H * W and want[1]["sum_support"] == F * H * W
    zeros = np.where(rng.random((F, H, W)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    for mode in (FR.MEAN, FR.MEDIAN):
        check_fuse(zeros, None, tol=0.0, min_count=1, mode=mode)
    # values exactly tol apart (they agree), and one float above
    v = np.full((F, H, W), 8.0, np.float32)
    v[::2] = np.float32(8.75)
    v[:, 2] = np.nextafter(np.float32(8.75), INF)
    v[1::2, 2] = np.float32(8.0)
    for mode in (FR.MEAN, FR.MEDIAN):
        want = check_fuse(v, None, tol=0.75, min_count=F, mode=mode)
        if F > 1:
            assert (want[2][:2] == F).all() and (want[2][2] == 0).all()
    # min_count = F, and min_count > F (nothing can be fused: SPARSE or EMPTY everywhere)
    v, conf = stack_of(rng, F, H, W, np.float32)
    check_fuse(v, conf, conf_min=1.0, tol=0.5, min_count=F)
    if F < 32:
        want = check_fuse(v, conf, conf_min=1.0, tol=0.5, min_count=F + 1)
        assert want[1]["n_fused"] == 0 and want[1]["n_unstable"] == 0
    # fill as NaN (its bits: the canonical quiet NaN goes through unchanged), as min_disp, as -inf
    for fill in (NAN, None, -INF, np.float32(-7.5)):
        check_fuse(v, conf, conf_min=2.0, tol=0.25, min_count=min(3, F), fill=fill)
    # large magnitudes: a difference that overflows agrees with nothing, sums stay in double
    big = np.float32(3.0e38)
    v = np.where(rng.random((F, H, W)) < 0.5, big, -big).astype(np.float32)
    for mode in (FR.MEAN, FR.MEDIAN):
        check_fuse(v, None, min_disp=-INF, tol=1.0, min_count=1, mode=mode)


# ---- every combination of the optional outputs; the raw entry ----
def raw_call(d, conf, p, out, sup, spr, rec, stream=None):
    F, H, W = d.shape
    return lib().sdr_fuse_disp_device(d.data_ptr(), 0 if d.dtype == torch.float32 else 1, d.stride(1),
                                      d.stride(0) if F > 1 else d.stride(1) * H, W, H, F,
                                      conf.data_ptr() if conf is not None else None, ctypes.byref(p), out.data_ptr(),
                                      sup.data_ptr() if sup is not None else None,
                                      spr.data_ptr() if spr is not None else None,
                                      rec.data_ptr() if rec is not None else None, stream)


def test_every_combination_of_outputs():
    rng = np.random.default_rng(8)
    F, H, W = 6, 4, 36
    v, conf = stack_of(rng, F, H, W, np.float32)
    want = FR.fuse(v, conf, conf_min=1.0, tol=0.5, min_count=2)
    d, c = torch.from_numpy(v).to(dev()), torch.from_numpy(conf).to(dev())
    p = FuseParams(-1.0, 1.0, 0.5, -1.0, 2, FR.MEAN)
    for bits in range(8):
        out = torch.full((H, W), 99.0, dtype=torch.float32, device=dev())
        sup = torch.full((H, W), 99, dtype=torch.uint8, device=dev()) if bits & 1 else None
        spr = torch.full((H, W), 99.0, dtype=torch.float32, device=dev()) if bits & 2 else None
        rec = torch.full((64,), 99, dtype=torch.uint8, device=dev()) if bits & 4 else None
        check(raw_call(d, c, p, out, sup, spr, rec))
        torch.cuda.synchronize()
        FR.assert_fusion_equal((out.cpu().numpy(), rec.cpu().numpy() if rec is not None else None,
                                sup.cpu().numpy() if sup is not None else None,
                                spr.cpu().numpy() if spr is not None else None), want)


def test_too_many_frames_refused_without_a_launch():
    F, H, W = 33, 2, 8
    d = torch.ones((F, H, W), dtype=torch.float32, device=dev())
    out = torch.full((H, W), 99.0, dtype=torch.float32, device=dev())
    rec = torch.full((64,), 99, dtype=torch.uint8, device=dev())
    p = FuseParams(-1.0, 0.0, 1.0, -1.0, 2, FR.MEAN)
    assert raw_call(d, None, p, out, None, None, rec) == -8  # SDR_ERR_LIMIT
    assert b"SDR_FUSE_MAX_FRAMES" in lib().sdr_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 99.0).all() and (rec.cpu().numpy() == 99).all()  # nothing ran: not even the clear
    with pytest.raises(sdr.SDRError) as e:
        sdr.Ruler(Q).fuse(d)
    assert e.value.code == -8
    with pytest.raises(sdr.SDRError) as e:
        sdr.Ruler(Q).fuse(np.ones((F, H, W), np.float32))
    assert e.value.code == -8


# ---- the host-pointer entry and the Python forms ----
def test_host_abi_forms():
    """sdr_fuse_disp (host pointers, strided rows and frames) == fuse_device == the restatement;
    Ruler.fuse takes arrays and tensors, and hands out only the maps asked for."""
    rng = np.random.default_rng(12)
    r = sdr.Ruler(Q, conf_min=1.0)
    for dtype in (np.float32, np.int16):
        for F, H, W in ((1, 3, 5), (5, 4, 37), (12, 5, 64)):
            base, conf = stack_of(rng, F, H + 1, W + 3, dtype)
            v = base[:, :H, :W]  # rows W + 3 apart, frames of H + 1 rows
            conf = np.ascontiguousarray(conf[:, :H, :W])
            kw = dict(tol=0.5, min_count=min(2, F), mode=FR.MEDIAN if F == 5 else FR.MEAN)
            want = FR.fuse(v, conf, conf_min=1.0, **kw)
            fused, rec, sup, spr = r.fuse(v, conf, support=True, spread=True, **kw)
            assert fused.shape == (1, H, W) and fused.dtype == np.float32 and rec.dtype == FUSION_DTYPE
            FR.assert_fusion_equal((fused[0], rec, sup, spr), want)
            got = r.fuse(torch.from_numpy(np.ascontiguousarray(v)).to(dev()), torch.from_numpy(conf).to(dev()),
                         support=True, spread=True, **kw)
            FR.assert_fusion_equal((got[0][0], got[1], got[2], got[3]), want)
    v, conf = stack_of(rng, 3, 4, 9, np.float32)
    assert len(r.fuse(v)) == 2 and len(r.fuse(v, support=True)) == 3 and len(r.fuse(v, spread=True)) == 3
    only_spread = r.fuse(v, spread=True, tol=0.5)
    FR.assert_fusion_equal((only_spread[0][0], only_spread[1], None, only_spread[2]), FR.fuse(v, tol=0.5))
    # a single (H, W) map is a stack of one
    one = r.fuse(v[0], min_count=1)
    FR.assert_fusion_equal((one[0][0], one[1], None, None), FR.fuse(v[:1], min_count=1))
    # out=: the map is written into the caller's tensor
    mine = torch.empty((4, 9), dtype=torch.float32, device=dev())
    outs = r.fuse_device(torch.from_numpy(v).to(dev()), out=mine, tol=0.5)
    assert outs[0].data_ptr() == mine.data_ptr() and tuple(outs[0].shape) == (1, 4, 9)
    torch.cuda.synchronize()
    FR.assert_fusion_equal((mine.cpu().numpy(), outs[1].cpu().numpy(), None, None), FR.fuse(v, tol=0.5))


def wall(seed=3, F=8, H=60, W=160):
    """F frames of test_ruler_cpu.py's noisy wall, as int16 (1/16 px) and float."""
    rng = np.random.default_rng(seed)
    d = np.round((40.0 + rng.normal(0.0, 0.25, (F, H, W))) * 16)
    u = rng.random((F, H, W))
    d[u < 0.15] = -16
    out = (u >= 0.15) & (u < 0.18)
    d[out] = np.round(rng.uniform(1, 79, int(out.sum())) * 16)
    s16 = d.astype(np.int16)
    return s16, s16.astype(np.float32) * np.float32(0.0625)


def test_chain_on_a_side_stream():
    """fuse_device -> measure_device and fit_plane_device on the fused tensor, on a stream that is
    not the default one, no synchronise in between: the restatements applied in sequence."""
    s16, f32 = wall()
    F, H, W = s16.shape
    r = sdr.Ruler(Q, radius=1, min_count=2)
    segs = [(0, 3, 4, 150, 50), (0, 159, 0, 0, 59), (0, 80, 30, 80, 30)]
    regions = [(0, 0, 0, W - 1, H - 1), (0, 10, 10, 60, 40)]
    side = torch.cuda.Stream(dev())
    for stack in (s16, f32):
        dt = torch.from_numpy(stack).to(dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            fused, rec, sup = r.fuse_device(dt, tol=1.0, min_count=2, support=True, stream=side)
            meas, _ = r.measure_device(fused, segs, stream=side)
            planes = r.fit_plane_device(fused, regions, stream=side)
        side.synchronize()
        want = FR.fuse(stack, tol=1.0, min_count=2)
        FR.assert_fusion_equal((fused.cpu().numpy()[0], rec.cpu().numpy(), sup.cpu().numpy(), None), want)
        m_want = RR.measure(want[0][None], segs, Q, radius=1, min_count=2)
        RR.assert_records_equal(meas.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE), m_want)
        PR.assert_planes_equal(planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE), PR.fit_planes(want[0][None], regions, Q))
        assert want[1]["n_fused"] == H * W and want[1]["n_filled"] > 0 and want[1]["n_replaced"] > 0


def test_live_loop_fuse_on_the_frame_stream():
    from stereo_depth_ruler_amd.pipeline import LiveLoop
    from stereo_depth_ruler_amd.rectify import StereoRectifier

    batch = 4
    sbs = S.sbs_bgr_frame(96, 400, 80, seed=21)
    H, W = sbs.shape[0], sbs.shape[1] // 2
    rng = np.random.default_rng(4)
    frames = np.clip(sbs[None].astype(np.int16) + rng.integers(-3, 4, (batch,) + sbs.shape), 0, 255).astype(np.uint8)
    K = np.array([[700.0, 0, W / 2], [0, 700.0, H / 2], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    cfg = types.SimpleNamespace(imageSize=(W, H), cameraMatrixLeft=K, cameraMatrixRight=K, distCoeffsLeft=None,
                                distCoeffsRight=None, R1=np.eye(3), R2=np.eye(3), P1=P, P2=P)
    rect = StereoRectifier(cfg)
    loop = LiveLoop(rect, Q, batch, ruler=dict(radius=1, min_count=2, conf_min=100.0))
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    w2, h2 = loop.w2, loop.h2
    segs = [(0, 5, 5, w2 - 6, h2 - 6), (0, w2 // 2, 2, w2 // 2, h2 - 3)]
    ft = torch.from_numpy(frames).to(dev())
    with torch.cuda.stream(side):
        loop.enqueue(ft, side)
        fused, rec, sup, spr = loop.fuse(side, tol=1.0, min_count=2, support=True, spread=True)
        meas, _ = loop.ruler.measure_device(fused, segs, conf=None, stream=side)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    want = FR.fuse(disp, conf, min_disp=loop.ruler.min_disp, conf_min=100.0, tol=1.0, min_count=2)
    FR.assert_fusion_equal((fused.cpu().numpy()[0], rec.cpu().numpy(), sup.cpu().numpy(), spr.cpu().numpy()), want)
    assert tuple(fused.shape) == (1, h2, w2) and want[1]["frames"] == batch and want[1]["n_fused"] > 0
    m_want = RR.measure(want[0][None], segs, Q, radius=1, min_count=2, min_disp=loop.ruler.min_disp)
    RR.assert_records_equal(meas.cpu().numpy().reshape(-1).view(MEASUREMENT_DTYPE), m_want)
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()
    bare = LiveLoop(rect, Q, 1)
    with pytest.raises(RuntimeError, match="without ruler="):
        bare.fuse(side)
    bare.close()


def test_cpp_facade_fuse(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::fuse gives Python's maps and records as bytes
    (tests/cpp/facade_fuse.cpp)."""
    exe = tmp_path / "facade_fuse"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_fuse.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    _, f32 = wall(seed=5, F=5, H=20, W=37)
    F, H, W = f32.shape
    conf = np.random.default_rng(6).integers(0, 256, (F, H, W)).astype(np.float32)
    f32.tofile(tmp_path / "stack.bin")
    conf.tofile(tmp_path / "conf.bin")
    np.asarray(Q, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), str(F), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    r = sdr.Ruler(Q, conf_min=100.0)
    mean = r.fuse(f32, conf, tol=1.0, min_count=2, support=True, spread=True)
    median = r.fuse(f32, conf, tol=0.5, min_count=3, mode=sdr.FUSE_MEDIAN, fill=NAN)
    FR.assert_fusion_equal((mean[0][0],) + mean[1:], FR.fuse(f32, conf, conf_min=100.0, tol=1.0, min_count=2))
    FR.assert_fusion_equal((median[0][0], median[1], None, None),
                           FR.fuse(f32, conf, conf_min=100.0, tol=0.5, min_count=3, mode=FR.MEDIAN, fill=NAN))
    assert (tmp_path / "mean.bin").read_bytes() == mean[0].tobytes()
    assert (tmp_path / "median.bin").read_bytes() == median[0].tobytes()
    assert (tmp_path / "support.bin").read_bytes() == mean[2].tobytes()
    assert (tmp_path / "spread.bin").read_bytes() == mean[3].tobytes()
    assert (tmp_path / "records.bin").read_bytes() == mean[1].tobytes() + median[1].tobytes()
    meas = r.measure(mean[0], [(0, 1, 1, W - 2, H - 2)])
    assert (tmp_path / "measure.bin").read_bytes() == meas.tobytes()
    assert f"fused={mean[1]['n_fused']} median_has_maps=0" in res.stdout and mean[1]["n_fused"] > 0
    # frames of two sizes and a measured fill: argument errors; 33 frames: the limit
    assert "odd_code=-1" in res.stdout and "fill_code=-1" in res.stdout and "many_code=-8" in res.stdout
