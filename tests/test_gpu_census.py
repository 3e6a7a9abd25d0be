"""GPU: the census matching cost (COST_CENSUS, sdr.h SDR_COST_CENSUS_9X7) through every layer,
bit-exact against its numpy pin (tests/census_ref.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import census_ref as CR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import lib  # noqa: E402
from stereo_depth_ruler_amd.sgbm import reproject_disp16  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = sdr.COST_CENSUS


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def census_args(D, mode, bs, minD=0, uniq=12, speckle=(0, 0), d12=1):
    """StereoSGBM.create arguments with penalties scaled for a census block cost (<= 62*bs^2)."""
    return (minD, D, bs, 2 * bs * bs, 12 * bs * bs, d12, 0, uniq, speckle[0], speckle[1], mode)


def ref_of(L, R, args, stages=3, **kw):
    minD, D, bs, P1, P2, d12, _, uniq, ws, sr, mode = args
    return CR.sgm_census(L, R, minD, D, bs, P1, P2, d12, uniq, ws, sr, mode, stages=stages, **kw)


CASES = [
    # (H, W, D, mode, bs, extras, swap (R, L))
    (32, 64, 16, 0, 5, {}, False),                                        # base
    (33, 97, 16, 1, 5, {}, False),                                        # odd width: the transform's byte path
    (31, 70, 16, 2, 5, {}, False),                                        # stripe-start bands
    (33, 100, 16, 3, 3, {}, False),                                       # 4 paths
    (5, 60, 16, 0, 5, {}, False),                                         # H shorter than the window and the box
    (9, 60, 16, 2, 5, {}, False),                                         # tiny stripes
    (11, 60, 16, 1, 5, {}, False),                                        # HH bottom rows keep P2
    (24, 40, 16, 0, 7, {}, False),                                        # W1 = 24: less than a column block
    (24, 50, 16, 0, 7, {}, False),                                        # a full column block + a 2-column edge block
    (48, 200, 128, 0, 5, {}, False),                                      # K = 1, all 64 lanes
    (37, 121, 96, 1, 3, dict(minD=3, uniq=0, speckle=(10, 1)), False),    # 48 live lanes: the aliasing lanes
    (70, 260, 144, 0, 5, dict(speckle=(40, 2)), False),                   # K = 2, partial second half
    (36, 300, 256, 0, 9, {}, False),                                      # K = 2 full
    (29, 140, 112, 2, 1, dict(d12=1000000), False),                       # bs = 1 (no box); LR check skipped
    (50, 160, 48, 0, 5, dict(minD=-20), False),                           # negative minD
    (64, 200, 80, 2, 5, dict(minD=-79, uniq=0, d12=1000000), True),       # the right matcher
    (40, 200, 64, 0, 11, dict(speckle=(30, 2)), False),                   # largest block
]


@pytest.mark.parametrize("idx", range(len(CASES)),
                         ids=[f"{c[0]}x{c[1]}_d{c[2]}_m{c[3]}_bs{c[4]}" for c in CASES])
def test_census_bit_exact(idx):
    H, W, D, mode, bs, extra, swap = CASES[idx]
    L, R, _ = S.make_pair(H, W, max(D, 16), seed=100 + idx)
    if swap:
        L, R = R, L
    args = census_args(D, mode, bs, **extra)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    assert m.getCostType() == CENSUS
    got = m.compute(L, R)
    ref = ref_of(L, R, args)
    assert np.array_equal(got, ref), f"{(got != ref).sum()} px differ"
    assert np.array_equal(m.debug_stage(2, (H, W), np.int16), ref_of(L, R, args, stages=0))
    if mode in (0, 1):
        minD = args[0]
        W1 = W + min(minD, 0) - max(minD + D, 0)
        C = m.debug_cost_volume(H, W1, D)
        assert np.array_equal(C, CR.census_cost_volume(L, R, minD, D, bs, args[4], mode))
    if idx < 3:
        T = m.debug_stage(7, (2, H, W), np.uint64)
        assert np.array_equal(T[0], CR.census_9x7(L)) and np.array_equal(T[1], CR.census_9x7(R))
    m.close()


def test_strided_device_input():
    """Rows padded to a stride that is no multiple of 4 (the transform's byte path on an aligned
    width): the result equals the dense one."""
    H, W, D = 30, 96, 16
    L, R, _ = S.make_pair(H, W, D, seed=201)
    args = census_args(D, 0, 5)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    dev = torch.device("cuda", 0)
    dense = m.compute(torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)).cpu().numpy()
    stride = W + 7
    buf = torch.zeros((2, H, stride), dtype=torch.uint8, device=dev)
    buf[0, :, :W] = torch.from_numpy(L).to(dev)
    buf[1, :, :W] = torch.from_numpy(R).to(dev)
    out = torch.empty((H, W), dtype=torch.int16, device=dev)
    from stereo_depth_ruler_amd.sgbm import set_handle_stream
    from stereo_depth_ruler_amd._lib import check
    set_handle_stream(m._h, 0)
    check(lib().sdr_sgbm_compute_device(m._h, buf[0].data_ptr(), buf[1].data_ptr(), W, H, stride, H * stride, 1,
                                        out.data_ptr(), W, W * H))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), dense)
    assert np.array_equal(dense, ref_of(L, R, args))


def test_batch_equals_per_frame():
    Ls, Rs = S.make_batch(3, 40, 120, 32, seed0=210)
    args = census_args(32, 0, 5)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    dev = torch.device("cuda", 0)
    got = m.compute(torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], m.compute(Ls[i], Rs[i])), i
    assert np.array_equal(got[1], ref_of(Ls[1], Rs[1], args))


def test_batched_hh_sweeps():
    """8 frames of MODE_HH take the row sweeps; every frame equals the numpy pin."""
    Ls, Rs = S.make_batch(8, 40, 120, 32, seed0=220)
    args = census_args(32, 1, 5)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    dev = torch.device("cuda", 0)
    m.enable_timing(2)
    got = m.compute(torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)).cpu().numpy()
    m.check_status()
    assert m.kernel_time(sdr.sgbm.KERNEL_SWEEP)[1] == 1  # the sweeps ran, not the chains
    for i in range(8):
        assert np.array_equal(got[i], ref_of(Ls[i], Rs[i], args)), i


@pytest.fixture(scope="module")
def class_pair():
    L, R, _ = S.make_pair(96, 400, 160, seed=230)
    return np.repeat(L[:, :, None], 3, 2), np.repeat(R[:, :, None], 3, 2)


def test_class_path(class_pair):
    """StereoDisparity(Q, cost=COST_CENSUS): the paired matchers' raw maps equal the numpy pin, and
    the output equals the same pipeline assembled from separate calls."""
    bl, br = class_pair
    sd = sdr.StereoDisparity(S.REFERENCE_Q, cost=CENSUS)
    assert sd.matcher.getCostType() == CENSUS and sd.right_matcher.getCostType() == CENSUS
    out = sd.computeDisparity(bl, br)
    dev = torch.device("cuda", 0)
    sl = sdr.resize_area_half(sdr.cvt_bgr2gray(torch.from_numpy(bl).to(dev))).cpu().numpy()
    sr = sdr.resize_area_half(sdr.cvt_bgr2gray(torch.from_numpy(br).to(dev))).cpu().numpy()
    # the matchers as the WLS filter's constructor leaves them
    la = (0, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2)
    ra = (-79, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2)
    assert np.array_equal(sd.last_disp_left, ref_of(sl, sr, la))
    assert np.array_equal(sd.last_disp_right, ref_of(sr, sl, ra))
    # the same pipeline from separate calls
    ml = sdr.StereoSGBM.create(0, 80, 5, 600, 2400, 1, 63, 12, 200, 2, sdr.MODE_SGBM_3WAY, cost=CENSUS)
    mr = sdr.createRightMatcher(ml)
    wls = sdr.createDisparityWLSFilter(ml)
    assert ml.getCostType() == CENSUS and mr.getCostType() == CENSUS
    wls.setLambda(8000.0)
    wls.setSigmaColor(1.1)
    dl, dr = ml.compute(sl, sr), mr.compute(sr, sl)
    assert np.array_equal(dl, sd.last_disp_left) and np.array_equal(dr, sd.last_disp_right)
    filt = wls.filter(dl, sl, disparity_map_right=dr)
    assert np.array_equal(np.asarray(filt), sd.last_filtered)
    assert np.array_equal(out, sd.last_filtered.astype(np.float32) * np.float32(0.0625))
    # a BT right matcher beside a census left one runs unpaired, each with its own cost
    sd.right_matcher.setCostType(sdr.COST_BT)
    sd.computeDisparity(bl, br)
    assert np.array_equal(sd.last_disp_left, dl) and not np.array_equal(sd.last_disp_right, dr)


def test_compute_reproject_fused():
    H, W, D = 48, 160, 48
    L, R, _ = S.make_pair(H, W, D, seed=240)
    args = census_args(D, 0, 5, speckle=(30, 2))
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    dev = torch.device("cuda", 0)
    Ld, Rd = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    disp, xyz = m.compute_reproject(Ld, Rd, S.REFERENCE_Q, True)
    ref = m.compute(Ld, Rd)
    torch.cuda.synchronize()
    assert torch.equal(disp[0], ref)
    assert np.array_equal(disp[0].cpu().numpy(), ref_of(L, R, args))
    want = reproject_disp16(disp, S.REFERENCE_Q, True)
    assert np.array_equal(xyz.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))


def test_invariance_under_increasing_intensity_change(oracle):
    """The reason for the feature: a strictly increasing intensity change of one image leaves the
    census disparity bit-identical; the BT matcher's output changes."""
    H, W, D = 48, 200, 80
    L, R, _ = S.make_pair(H, W, D, seed=250)
    L = (L.astype(np.int32) * 200 // 255).astype(np.uint8)
    R = (R.astype(np.int32) * 200 // 255).astype(np.uint8)
    lut = np.arange(256)
    lut = (lut + lut // 4).astype(np.int32)
    assert lut[200] <= 255 and (np.diff(lut[:201]) > 0).all()
    R2 = lut[R].astype(np.uint8)
    args = census_args(D, 2, 5)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    a, b = m.compute(L, R), m.compute(L, R2)
    assert np.array_equal(a, b)
    assert np.array_equal(a, ref_of(L, R, args))
    bt_args = (0, D, 5, 600, 2400, 1, 63, 12, 0, 0, 2)
    bt = sdr.StereoSGBM.create(*bt_args)
    c, d = bt.compute(L, R), bt.compute(L, R2)
    assert not np.array_equal(c, d)
    assert np.array_equal(d, oracle.sgbm_compute(L, R2, oracle.make_params(*bt_args)))


def test_switching_cost_type_leaves_no_state(oracle):
    H, W, D = 40, 150, 48
    L, R, _ = S.make_pair(H, W, D, seed=260)
    args = (0, D, 5, 50, 300, 1, 63, 12, 30, 2, 0)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    cen = m.compute(L, R)
    assert np.array_equal(cen, ref_of(L, R, args))
    m.setCostType(sdr.COST_BT)
    assert m.getCostType() == sdr.COST_BT
    assert np.array_equal(m.compute(L, R), oracle.sgbm_compute(L, R, oracle.make_params(*args)))
    with pytest.raises(sdr.SDRError):
        m.debug_stage(7, (2, H, W), np.uint64)  # the last compute was BT
    m.setCostType(CENSUS)
    assert np.array_equal(m.compute(L, R), cen)
    with pytest.raises(sdr.SDRError):
        m.setCostType(7)
    assert m.getCostType() == CENSUS


def test_refusals_on_a_live_handle():
    L, R, _ = S.make_pair(40, 400, 64, seed=270)
    m = sdr.StereoSGBM.create(*census_args(64, 0, 5), cost=CENSUS)
    with pytest.raises(sdr.SDRError) as ei:
        m.compute(np.repeat(L[:, :, None], 3, 2), np.repeat(R[:, :, None], 3, 2))
    assert ei.value.code == -5
    m.setBlockSize(13)
    with pytest.raises(sdr.SDRError) as ei:
        m.compute(L, R)
    assert ei.value.code == -8
    m.setBlockSize(5)
    m.setNumDisparities(272)
    with pytest.raises(sdr.SDRError) as ei:
        m.compute(L, R)
    assert ei.value.code == -8
    m.setNumDisparities(64)
    assert np.array_equal(m.compute(L, R), ref_of(L, R, census_args(64, 0, 5)))


def test_graph_capture_replay():
    """One MODE_SGBM census call captured after a sizing call and replayed twice (as
    test_gpu_parity.test_graph_capture_replay; the captured graph is linear)."""
    dev = torch.device("cuda", 0)
    F, H, W, D = 2, 48, 200, 64
    args = census_args(D, 0, 5, speckle=(50, 2))
    Ls, Rs = S.make_batch(F, H, W, D, seed0=500)
    Ld, Rd = torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    m.compute(Ld, Rd)  # sizes the scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.compute(Ld, Rd)
    for seed in (600, 700):
        L2, R2 = S.make_batch(F, H, W, D, seed0=seed)
        Ld.copy_(torch.from_numpy(L2))
        Rd.copy_(torch.from_numpy(R2))
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i in range(F):
            assert np.array_equal(got[i], ref_of(L2[i], R2[i], args)), (seed, i)
    again = m.compute(Ld, Rd)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy(), got)
    m.close()


def test_cpp_facade_census(tmp_path):
    """include/sdr/stereo.hpp: setCostType + compute equals the Python result (tests/cpp/facade_census.cpp)."""
    exe = tmp_path / "facade_census"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_census.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    H, W, D = 48, 200, 80
    L, R, _ = S.make_pair(H, W, D, seed=280)
    args = census_args(D, 2, 5)
    m = sdr.StereoSGBM.create(*args, cost=CENSUS)
    want = m.compute(L, R)
    mr = sdr.createRightMatcher(m)
    want_r = mr.compute(R, L)
    L.tofile(tmp_path / "l.bin")
    R.tofile(tmp_path / "r.bin")
    want.tofile(tmp_path / "want.bin")
    want_r.tofile(tmp_path / "want_r.bin")
    res = subprocess.run([str(exe), str(W), str(H), str(D), str(args[3]), str(args[4]), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "census_equal=1" in res.stdout and "right_equal=1" in res.stdout
    assert "cost_roundtrip=1" in res.stdout and "bad_cost_code=-1" in res.stdout
