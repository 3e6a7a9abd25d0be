"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle, bit-exact.

Disparity is int16 and compared bit for bit; XYZ float32 is compared bit for bit too (the oracle
and the kernel both evaluate reprojectImageTo3D in f64 with contraction off), which is stricter
than the north star's 1e-3 m (= 1.0 in the reference's mm units) tolerance, asserted as well.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.sgbm import reproject_disp16, selftest_wave_ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XYZ_TOL_MM = 1.0  # north star: 1e-3 m; reference Q is in millimetres


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run_both(oracle, L, R, args, **kw):
    m = sdr.StereoSGBM.create(*args, **kw)
    got = m.compute(L, R)
    p = oracle.make_params(*args, **kw)
    return got, oracle.sgbm_compute(L, R, p), m


def test_selftest_wave_ops():
    assert selftest_wave_ops() == [0, 0, 0, 0]


CASES = [
    # (H, W, D, mode, bs, minD, uniq, speckle ws/range, d12, P1, P2, cap, seed)
    (32, 64, 16, 0, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 0),
    (33, 97, 16, 1, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 1),
    (31, 70, 16, 2, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 2),
    (40, 96, 32, 0, 3, 0, 10, (0, 0), 1, 8, 32, 63, 3),
    (48, 160, 64, 0, 5, 0, 12, (50, 2), 1, 600, 2400, 63, 4),
    (48, 200, 128, 0, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 5),
    (48, 200, 80, 2, 5, 0, 12, (200, 2), 1, 600, 2400, 63, 6),
    (60, 320, 256, 1, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 7),
    (50, 160, 48, 0, 5, -20, 12, (0, 0), 1, 600, 2400, 63, 8),
    (45, 150, 32, 2, 7, 0, 5, (0, 0), 2, 200, 800, 31, 9),
    (37, 121, 96, 1, 3, 3, 0, (10, 1), 1, 100, 900, 15, 10),
    (29, 140, 112, 2, 1, 0, 15, (0, 0), 1000000, 10, 50, 63, 11),
    (64, 200, 80, 2, 5, -79, 0, (0, 0), 1000000, 600, 2400, 63, 12),   # right matcher
    (25, 90, 16, 0, 9, 0, 20, (5, 4), 1, 30, 120, 63, 13),
    (70, 260, 144, 0, 5, 0, 8, (40, 2), 1, 600, 2400, 63, 14),
    (70, 300, 240, 2, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 15),
    (11, 60, 16, 1, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 16),            # short image, HH bottom rule
    (9, 60, 16, 2, 5, 0, 12, (0, 0), 1, 600, 2400, 63, 17),             # 3WAY tiny stripes
    (40, 200, 64, 0, 11, 0, 12, (30, 2), 1, 600, 2400, 63, 18),         # largest block (11x11)
    (44, 210, 48, 2, 11, 0, 10, (0, 0), 1, 600, 2400, 63, 19),          # 3WAY, 11x11
    (36, 300, 256, 0, 9, 0, 12, (0, 0), 1, 600, 2400, 63, 20),          # D = 256, 5-path
    (33, 100, 16, 3, 5, 0, 12, (20, 2), 1, 600, 2400, 63, 21),          # MODE_HH4 (4 paths)
    (48, 200, 128, 3, 3, -6, 10, (0, 0), 1, 300, 1800, 31, 22),         # MODE_HH4, minD < 0
    (40, 320, 208, 3, 7, 0, 5, (50, 2), 2, 100, 900, 15, 23),           # MODE_HH4, D > 128
    (48, 200, 64, 0, 5, 0, 10, (50, 2), 1, 300, 1800, 200, 24),         # preFilterCap > 127 (uchar wrap)
    (40, 180, 48, 2, 3, -4, 12, (0, 0), 1, 600, 2400, 255, 25),         # 3WAY, cap 255
    (36, 160, 32, 1, 5, 0, 10, (20, 2), 1, 200, 900, 1000, 26),         # MODE_HH, ftzero 1001 (tab[0] wraps)
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}_d{c[2]}_m{c[3]}_bs{c[4]}_min{c[5]}" for c in CASES])
def test_sgbm_bit_exact(oracle, case):
    H, W, D, mode, bs, minD, uniq, (ws, sr), d12, P1, P2, cap, seed = case
    L, R, _ = S.make_pair(H, W, max(D, 16), seed=seed)
    args = (minD, D, bs, P1, P2, d12, cap, uniq, ws, sr, mode)
    got, ref, m = run_both(oracle, L, R, args)
    assert np.array_equal(got, ref), f"{(got != ref).sum()} px differ"
    # intermediate (after LR check, before median/speckle) as well
    raw_ref = oracle.sgbm_compute(L, R, oracle.make_params(*args), stages=0)
    assert np.array_equal(m.debug_stage(2, (H, W), np.int16), raw_ref)


@pytest.mark.parametrize("nstripes", [1, 3, 8])
def test_3way_nstripes(oracle, nstripes):
    L, R, _ = S.make_pair(90, 200, 48, seed=21)
    args = (0, 48, 5, 600, 2400, 1, 63, 12, 0, 0, 2)
    got, ref, _ = run_both(oracle, L, R, args, nstripes=nstripes)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("rule", [1, 2])
@pytest.mark.parametrize("mode", [0, 2])
def test_uniqueness_rule_switch(oracle, rule, mode):
    L, R, _ = S.make_pair(50, 160, 32, seed=22)
    args = (0, 32, 5, 600, 2400, 1, 63, 15, 0, 0, mode)
    got, ref, _ = run_both(oracle, L, R, args, uniq_rule=rule)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("rule", [1, 2])
def test_uniqueness_rule_switch_rec12(oracle, rule):
    """Both rules through k_south_wta's 12-bit-record consumer (mode 0, D = 128, one frame)."""
    L, R, _ = S.make_pair(48, 200, 128, seed=27)
    args = (0, 128, 5, 600, 2400, 1, 63, 15, 0, 0, 0)
    got, ref, _ = run_both(oracle, L, R, args, uniq_rule=rule)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("rule", [1, 2])
def test_uniqueness_rule_switch_two_columns(oracle, rule):
    """Both rules through k_south_wta's two-column form: test_two_chain_paths' batched 3WAY shape
    (4 frames x 4 stripes x 372 column chains, more than 8 a CU; D = 48, 3 paths)."""
    mode, D, H, W, batch = 2, 48, 300, 420, 4
    args = (0, D, 5, 600, 2400, 1, 63, 15, 0, 0, mode)
    Ls = np.empty((batch, H, W), np.uint8)
    Rs = np.empty((batch, H, W), np.uint8)
    for i in range(batch):
        Ls[i], Rs[i], _ = S.make_pair(H, W, D, seed=34 + i)
    dev = torch.device("cuda", 0)
    m = sdr.StereoSGBM.create(*args, uniq_rule=rule)
    out = m.compute(torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)).cpu().numpy()
    p = oracle.make_params(*args, uniq_rule=rule)
    for i in range(batch):
        ref = oracle.sgbm_compute(Ls[i], Rs[i], p)
        assert np.array_equal(out[i], ref), f"frame {i}: {(out[i] != ref).sum()} px differ"
    m.close()


def test_cost_volume_bit_exact(oracle):
    L, R, _ = S.make_pair(40, 150, 48, seed=23)
    for mode in (0, 1, 3):
        args = (0, 48, 5, 600, 2400, 1, 63, 12, 0, 0, mode)
        m = sdr.StereoSGBM.create(*args)
        m.compute(L, R)
        C = m.debug_cost_volume(40, 150 - 48, 48)
        assert np.array_equal(C, oracle.cost_volume(L, R, oracle.make_params(*args)))


GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_fixtures(path):
    g = np.load(path)
    args = tuple(int(v) for v in g["params"])
    m = sdr.StereoSGBM.create(*args)
    assert np.array_equal(m.compute(g["left"], g["right"]), g["disp"])
    # device path + fused reprojection (pcd_write.cpp:111-116)
    Ld = torch.from_numpy(g["left"]).cuda()
    Rd = torch.from_numpy(g["right"]).cuda()
    disp, xyz = m.compute_reproject(Ld, Rd, S.REFERENCE_Q, True)
    assert np.array_equal(disp[0].cpu().numpy(), g["disp"])
    assert np.array_equal(xyz[0].cpu().numpy().view(np.uint32), g["xyz"].view(np.uint32))


def test_batch_equals_single_frames(oracle):
    Ls, Rs = S.make_batch(5, 48, 144, 32, seed0=40)
    args = (0, 32, 5, 600, 2400, 1, 63, 12, 30, 2, 0)
    m = sdr.StereoSGBM.create(*args)
    out = m.compute(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda())
    torch.cuda.synchronize()
    p = oracle.make_params(*args)
    for i in range(5):
        assert np.array_equal(out[i].cpu().numpy(), oracle.sgbm_compute(Ls[i], Rs[i], p)), i


def test_full_size_c2_sgbm5_d128(oracle):
    """BASELINE configs[1]: 1280x720, d=128, 5-path + reproject(handleMissing) -- bit-exact."""
    L, R, gt = S.make_pair(720, 1280, 128, seed=100)
    args = (0, 128, 5, 600, 2400, 1, 63, 12, 200, 2, 0)
    m = sdr.StereoSGBM.create(*args)
    disp, xyz = m.compute_reproject(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), S.REFERENCE_Q, True)
    got = disp[0].cpu().numpy()
    ref = oracle.sgbm_compute(L, R, oracle.make_params(*args))
    assert np.array_equal(got, ref)
    ref_xyz = oracle.reproject(oracle.disp_to_float(ref), S.REFERENCE_Q, True)
    g = xyz[0].cpu().numpy()
    assert np.array_equal(g.view(np.uint32), ref_xyz.view(np.uint32))
    fin = np.isfinite(ref_xyz)
    assert np.max(np.abs(g[fin] - ref_xyz[fin])) <= XYZ_TOL_MM
    # the host-pointer forms (pinned staging, chunked copies) give the same bytes
    hd, hx = m.compute_reproject(L, R, S.REFERENCE_Q, True)
    assert np.array_equal(hd, got) and np.array_equal(hx.view(np.uint32), ref_xyz.view(np.uint32))
    _, hx2 = m.compute_reproject(L, R, S.REFERENCE_Q, True, disp=False)
    assert np.array_equal(hx2.view(np.uint32), ref_xyz.view(np.uint32))
    assert np.array_equal(m.compute(L, R), got)
    # ground-truth sanity on the synthetic scene
    v = got > -16
    assert v.mean() > 0.8
    assert (np.abs(got[v] / 16.0 - gt[v]) > 1).mean() < 0.08


def test_full_size_hh8_d256(oracle):
    """configs[2] frame shape: 1280x720, d=256, MODE_HH -- bit-exact."""
    L, R, _ = S.make_pair(720, 1280, 256, seed=101)
    args = (0, 256, 5, 600, 2400, 1, 63, 12, 200, 2, 1)
    got, ref, _ = run_both(oracle, L, R, args)
    assert np.array_equal(got, ref)


def test_reference_exact_class_matchers(oracle):
    """C0: 640x360, the reference's left matcher (3WAY d=80, WLS-mutated) and its right matcher."""
    L, R, _ = S.make_pair(360, 640, 80, seed=102)
    left = (0, 80, 5, 600, 2400, 1000000, 63, 12, 0, 2, 2)
    got, ref, m = run_both(oracle, L, R, left)
    assert np.array_equal(got, ref)
    rm = sdr.createRightMatcher(m)
    rp = rm.params()
    assert (rp.minDisparity, rp.uniquenessRatio, rp.disp12MaxDiff, rp.speckleWindowSize) == (-79, 0, 1000000, 0)
    got_r = rm.compute(R, L)
    ref_r = oracle.sgbm_compute(R, L, oracle.make_params(-79, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    assert np.array_equal(got_r, ref_r)


def class_path_ref(oracle, bgr_l, bgr_r):
    """Oracle composition of StereoDisparity::computeDisparity (stereo_disparity.cpp:17-39):
    gray -> INTER_AREA 0.5 -> left matcher (3WAY d=80, mutated by createDisparityWLSFilter:
    disp12MaxDiff 1e6, speckle 0, uniqueness 0) + right matcher -> WLS (8000, 1.1) -> /16."""
    gl = oracle.resize_area_half(oracle.bgr2gray(bgr_l))
    gr = oracle.resize_area_half(oracle.bgr2gray(bgr_r))
    ref_l = oracle.sgbm_compute(gl, gr, oracle.make_params(0, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    ref_r = oracle.sgbm_compute(gr, gl, oracle.make_params(-79, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    h, w = gl.shape
    q = oracle.wls_params_for_sgbm(0, 80, 5, w, h, 8000.0, 1.1)
    filt, conf = oracle.wls_filter(ref_l, ref_r, gl, q, return_conf=True)
    return ref_l, ref_r, filt, conf, oracle.disp_to_float(filt)


def test_class_path_stereo_disparity(oracle):
    """StereoDisparity.computeDisparity: gray + INTER_AREA + both matchers + WLS + /16 on device."""
    from stereo_depth_ruler_amd.stereo_disparity import StereoDisparity

    rng = np.random.default_rng(7)
    Lg, Rg, _ = S.make_pair(720, 1280, 160, seed=103)
    bgr_l = np.stack([Lg, np.roll(Lg, 1, 1), rng.integers(0, 256, Lg.shape).astype(np.uint8)], -1)
    bgr_r = np.stack([Rg, np.roll(Rg, 1, 1), rng.integers(0, 256, Rg.shape).astype(np.uint8)], -1)
    sd = StereoDisparity(S.REFERENCE_Q)
    out = sd.computeDisparity(bgr_l, bgr_r)
    ref_l, ref_r, filt, conf, ref_out = class_path_ref(oracle, bgr_l, bgr_r)
    assert np.array_equal(sd.last_disp_left, ref_l)
    assert np.array_equal(sd.last_disp_right, ref_r)
    assert np.array_equal(sd.conf_map.view(np.uint32), conf.view(np.uint32))
    assert np.array_equal(sd.last_filtered, filt)
    assert np.array_equal(out, ref_out)
    depth = sd.computeDepth(out)
    ref_depth = oracle.reproject(out, S.REFERENCE_Q, False)
    assert np.array_equal(depth.view(np.uint32), ref_depth.view(np.uint32))
    assert sd.get_matcher().getNumDisparities() == 80
    assert sd.get_matcher().getUniquenessRatio() == 0


def test_reproject_apis(oracle):
    rng = np.random.default_rng(8)
    d16 = rng.integers(-16, 128 * 16, size=(200, 333)).astype(np.int16)
    df = oracle.disp_to_float(d16)
    for hm in (False, True):
        ref = oracle.reproject(df, S.REFERENCE_Q, hm)
        host = sdr.reprojectImageTo3D(df, S.REFERENCE_Q, hm)
        assert np.array_equal(host.view(np.uint32), ref.view(np.uint32))
        dev = sdr.reprojectImageTo3D(torch.from_numpy(df).cuda(), S.REFERENCE_Q, hm).cpu().numpy()
        assert np.array_equal(dev.view(np.uint32), ref.view(np.uint32))
        fused = reproject_disp16(torch.from_numpy(d16).cuda(), S.REFERENCE_Q, hm).cpu().numpy()
        assert np.array_equal(fused.view(np.uint32), ref.view(np.uint32))
        # OpenCV semantics: int16 input is used as-is
        raw = sdr.reprojectImageTo3D(d16, S.REFERENCE_Q, hm)
        ref_raw = oracle.reproject(d16.astype(np.float32), S.REFERENCE_Q, hm)
        assert np.array_equal(raw.view(np.uint32), ref_raw.view(np.uint32))


def test_reproject_appendix_b_on_gpu():
    from test_oracle_kat import APPENDIX_B

    disp = np.zeros((720, 1280), np.float32)
    pts = [(int(x), int(y), d, X, Y, Z) for x, y, d, X, Y, Z in APPENDIX_B if x == int(x)]
    for x, y, d, *_ in pts:
        disp[y, x] = d
    out = sdr.reprojectImageTo3D(torch.from_numpy(disp).cuda(), S.REFERENCE_Q).cpu().numpy()
    for x, y, d, X, Y, Z in pts:
        assert tuple(out[y, x]) == (np.float32(X), np.float32(Y), np.float32(Z))


def test_gray_and_area_kernels(oracle):
    rng = np.random.default_rng(9)
    bgr = rng.integers(0, 256, size=(2, 64, 90, 3)).astype(np.uint8)
    g = sdr.cvt_bgr2gray(torch.from_numpy(bgr).cuda())
    small = sdr.resize_area_half(g).cpu().numpy()
    g = g.cpu().numpy()
    for i in range(2):
        assert np.array_equal(g[i], oracle.bgr2gray(bgr[i]))
        assert np.array_equal(small[i], oracle.resize_area_half(g[i]))


def test_errors_mirror_opencv_asserts():
    L = np.zeros((20, 64), np.uint8)
    with pytest.raises(sdr.SDRError) as e:
        sdr.StereoSGBM.create(0, 100, 5).compute(L, L)
    assert e.value.code == -2
    with pytest.raises(sdr.SDRError) as e:
        sdr.StereoSGBM.create(0, 16, 5, mode=7).compute(L, L)
    assert e.value.code == -3
    with pytest.raises(sdr.SDRError):
        sdr.StereoSGBM.create(0, 16, 5).compute(L, np.zeros((20, 65), np.uint8))
    with pytest.raises(sdr.SDRError):
        sdr.StereoSGBM.create(0, 16, 5).compute(L.astype(np.int16), L.astype(np.int16))
    # disparity range wider than the image: everything is invalid (OpenCV's early return)
    out = sdr.StereoSGBM.create(0, 80, 5).compute(L[:, :60], L[:, :60])
    assert np.all(out == -16)


def test_determinism_and_streams(oracle):
    L, R, _ = S.make_pair(120, 400, 64, seed=24)
    args = (0, 64, 5, 600, 2400, 1, 63, 12, 100, 2, 0)
    m = sdr.StereoSGBM.create(*args)
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    a = m.compute(Ld, Rd).clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = m.compute(Ld, Rd)
    s.synchronize()
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), oracle.sgbm_compute(L, R, oracle.make_params(*args)))


def test_kernel_timing_api():
    L, R, _ = S.make_pair(64, 200, 32, seed=25)
    m = sdr.StereoSGBM.create(0, 32, 5, 600, 2400, 1, 63, 12, 50, 2, 0)
    m.enable_timing(2)
    m.compute(L, R)
    t, n = m.kernel_time(-1, reset=True)
    assert n >= 5 and t > 0  # prefilter, cost, paths, wta, lr + median + speckle (one KTimer each)
    st = m.last_timing()
    assert st["paths_ms"] > 0


def test_cpp_facade(oracle, tmp_path):
    """include/sdr/stereo.hpp used like the reference's C++ callers (tests/cpp/facade_test.cpp)."""
    exe = tmp_path / "facade_test"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_test.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    H, W = 240, 400
    L, R, _ = S.make_pair(H, W, 80, seed=26)
    bl = np.repeat(L[:, :, None], 3, 2)
    br = np.repeat(R[:, :, None], 3, 2)
    for name, a in (("l", L), ("r", R), ("bl", bl), ("br", br)):
        a.tofile(tmp_path / f"{name}.bin")
    res = subprocess.run([str(exe), str(W), str(H)] + [str(tmp_path / f"{n}.bin") for n in ("l", "r", "bl", "br")]
                         + [str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "numDisparities=80" in res.stdout and "exception code=-2" in res.stdout
    assert "fused_equal=1" in res.stdout
    disp = np.fromfile(tmp_path / "disp.bin", np.int16).reshape(H, W)
    ref = oracle.sgbm_compute(L, R, oracle.make_params(0, 80, 5, 600, 2400, 1, 63, 12, 200, 2, 2))
    assert np.array_equal(disp, ref)
    xyz = np.fromfile(tmp_path / "xyz.bin", np.float32).reshape(H, W, 3)
    ref_xyz = oracle.reproject(oracle.disp_to_float(ref), S.REFERENCE_Q, True)
    assert np.array_equal(xyz.view(np.uint32), ref_xyz.view(np.uint32))
    cls = np.fromfile(tmp_path / "class_disp.bin", np.float32).reshape(H // 2, W // 2)
    _, _, _, conf, ref_cls = class_path_ref(oracle, bl, br)
    assert np.array_equal(cls, ref_cls)
    cconf = np.fromfile(tmp_path / "class_conf.bin", np.float32).reshape(H // 2, W // 2)
    assert np.array_equal(cconf.view(np.uint32), conf.view(np.uint32))
    # display outputs through the facade, two frames (the second through the EMA)
    h2, w2 = H // 2, W // 2
    depth = oracle.reproject(ref_cls, S.REFERENCE_Q, False)
    zr = np.array([1000.0, 2000.0])
    turbo, jet = oracle.colormap_lut(oracle.COLORMAP_TURBO), oracle.colormap_lut(oracle.COLORMAP_JET)
    pv = pd = None
    for k in range(2):
        vis = oracle.show_disparity_map(ref_cls, 80, pv)
        dv = oracle.show_depth_map(depth, zr, turbo, pd)
        assert np.array_equal(np.fromfile(tmp_path / f"vis{k}.bin", np.uint8).reshape(h2, w2), vis)
        assert np.array_equal(np.fromfile(tmp_path / f"depthvis{k}.bin", np.uint8).reshape(h2, w2, 3), dv)
        pv, pd = vis, dv
    small = oracle.resize_area_half_bgr(bl)
    ov = oracle.add_weighted(small, 0.7, oracle.apply_colormap(pv, jet), 0.3)
    assert np.array_equal(np.fromfile(tmp_path / "overlay.bin", np.uint8).reshape(h2, w2, 3), ov)
    cov = float(res.stdout.split("\ncoverage=")[1].split()[0])
    assert cov == oracle.depth_coverage(depth, 80)
    # one Display through show_depthMap -> depth_coverage -> show_depthMap: the second
    # map blends against the first, as with no coverage call in between
    zr = np.array([1000.0, 2000.0])
    pd = None
    for k in range(2):
        dv = oracle.show_depth_map(depth, zr, turbo, pd)
        assert np.array_equal(np.fromfile(tmp_path / f"dd_depthvis{k}.bin", np.uint8).reshape(h2, w2, 3), dv), k
        assert float(res.stdout.split(f"dd_coverage{k}=")[1].split()[0]) == oracle.depth_coverage(depth, 80)
        pd = dv


def test_host_pointer_strides_and_sizes(oracle):
    """sdr_sgbm_compute / sdr_sgbm_compute_reproject / sdr_reproject on padded host rows (stride >
    width, output strides > width), and frame sizes that shrink and grow between calls (the
    handle's pinned staging and device buffers only grow)."""
    import ctypes

    from stereo_depth_ruler_amd._lib import lib
    args = (0, 48, 5, 600, 2400, 1, 63, 12, 50, 2, 0)
    m = sdr.StereoSGBM.create(*args)
    p = oracle.make_params(*args)
    Q = (ctypes.c_double * 16)(*np.asarray(S.REFERENCE_Q, np.float64).ravel())
    for (H, W, seed) in ((64, 200, 1), (40, 120, 2), (90, 333, 3)):
        L, R, _ = S.make_pair(H, W, 48, seed=seed)
        ref = oracle.sgbm_compute(L, R, p)
        ref_xyz = oracle.reproject(oracle.disp_to_float(ref), S.REFERENCE_Q, True)
        pad = 37
        Lp = np.zeros((H, W + pad), np.uint8)
        Rp = np.zeros((H, W + pad), np.uint8)
        Lp[:, :W], Rp[:, :W] = L, R
        dp = np.full((H, W + 5), 7, np.int16)
        assert lib().sdr_sgbm_compute(m._h, Lp.ctypes.data, Rp.ctypes.data, W, H, 1, W + pad, dp.ctypes.data, W + 5) == 0
        assert np.array_equal(dp[:, :W], ref) and (dp[:, W:] == 7).all()
        xp = np.full((H, 3 * W + 4), 9, np.float32)
        dp[:] = 7
        assert lib().sdr_sgbm_compute_reproject(m._h, Lp.ctypes.data, Rp.ctypes.data, W, H, W + pad, dp.ctypes.data,
                                                W + 5, Q, 1, xp.ctypes.data, 3 * W + 4) == 0
        assert np.array_equal(dp[:, :W], ref) and (dp[:, W:] == 7).all()
        assert np.array_equal(xp[:, :3 * W].reshape(H, W, 3).view(np.uint32), ref_xyz.view(np.uint32))
        assert (xp[:, 3 * W:] == 9).all()
        df = np.zeros((H, W + 3), np.float32)
        df[:, :W] = oracle.disp_to_float(ref)
        xp[:] = 9
        assert lib().sdr_reproject(df.ctypes.data, W, H, W + 3, Q, 1, xp.ctypes.data, 3 * W + 4) == 0
        assert np.array_equal(xp[:, :3 * W].reshape(H, W, 3).view(np.uint32), ref_xyz.view(np.uint32))
    m.close()


def test_host_pointer_page_locked_buffers(oracle):
    """Page-locked caller buffers (sdr.host_empty) take the direct-DMA branch: same bytes."""
    args = (0, 64, 5, 600, 2400, 1, 63, 12, 50, 2, 0)
    H, W = 70, 250
    L, R, _ = S.make_pair(H, W, 64, seed=5)
    ref = oracle.sgbm_compute(L, R, oracle.make_params(*args))
    ref_xyz = oracle.reproject(oracle.disp_to_float(ref), S.REFERENCE_Q, False)
    pl, pr = sdr.host_empty((H, W), np.uint8), sdr.host_empty((H, W), np.uint8)
    pl[:], pr[:] = L, R
    pd, px = sdr.host_empty((H, W), np.int16), sdr.host_empty((H, W, 3), np.float32)
    m = sdr.StereoSGBM.create(*args)
    for _ in range(2):
        pd[:] = 0
        px[:] = 0
        d, x = m.compute_reproject(pl, pr, S.REFERENCE_Q, False, disp=pd, xyz=px)
        assert d is pd and x is px
        assert np.array_equal(pd, ref) and np.array_equal(px.view(np.uint32), ref_xyz.view(np.uint32))
        assert np.array_equal(m.compute(pl, pr, pd), ref)
    m.close()


@pytest.mark.parametrize("paired", [True, False])
def test_class_device_paired_and_forked(oracle, paired):
    """sdr_stereo_class_depth_device on a batch of 2 frames: the left and right matcher run as one
    paired batch when they differ only in minDisparity (the class path's case), on a forked side
    stream otherwise (here: a right matcher with uniquenessRatio 3) -- both bit-exact against the
    oracle chain, including the fused convertTo(1/16) + computeDepth epilogue."""
    import ctypes

    from stereo_depth_ruler_amd._lib import lib
    from stereo_depth_ruler_amd.ximgproc import createDisparityWLSFilter

    h, w, F = 72, 240, 2
    pairs = [S.make_pair(h, w, 48, seed=200 + i)[:2] for i in range(F)]
    m = sdr.StereoSGBM.create(0, 48, 5, 600, 2400, 1, 63, 12, 200, 2, sdr.MODE_SGBM_3WAY)
    rm = sdr.createRightMatcher(m)
    wls = createDisparityWLSFilter(m)
    wls.setLambda(8000.0)
    wls.setSigmaColor(1.1)
    runiq = 0 if paired else 3
    rm.setUniquenessRatio(runiq)
    dev = torch.device("cuda", 0)
    sl = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    sr = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    out = torch.empty((F, h, w), dtype=torch.float32, device=dev)
    filt = torch.empty((F, h, w), dtype=torch.int16, device=dev)
    xyz = torch.empty((F, h, w, 3), dtype=torch.float32, device=dev)
    Q = (ctypes.c_double * 16)(*np.asarray(S.REFERENCE_Q, np.float64).ravel())
    L = lib()
    assert L.sdr_sgbm_set_stream(m._h, None) == 0
    assert L.sdr_stereo_class_depth_device(m._h, rm._h, wls._h, sl.data_ptr(), sr.data_ptr(), w, h, F,
                                           out.data_ptr(), filt.data_ptr(), None, Q, xyz.data_ptr()) == 0
    torch.cuda.synchronize()
    q = oracle.wls_params_for_sgbm(0, 48, 5, w, h, 8000.0, 1.1)
    for i, (gl, gr) in enumerate(pairs):
        ref_l = oracle.sgbm_compute(gl, gr, oracle.make_params(0, 48, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
        ref_r = oracle.sgbm_compute(gr, gl, oracle.make_params(-47, 48, 5, 600, 2400, 1000000, 63, runiq, 0, 2, 2))
        ref_f = oracle.wls_filter(ref_l, ref_r, gl, q)
        ref_o = oracle.disp_to_float(ref_f)
        assert np.array_equal(filt[i].cpu().numpy(), ref_f), i
        assert np.array_equal(out[i].cpu().numpy(), ref_o), i
        ref_xyz = oracle.reproject(ref_o, S.REFERENCE_Q, False)
        assert np.array_equal(xyz[i].cpu().numpy().view(np.uint32), ref_xyz.view(np.uint32)), i
    for o in (m, rm, wls):
        o.close()


def test_host_call_refused_before_upload(oracle):
    """A host-pointer call the engine refuses (the int16 cost domain) returns its error
    before staging anything; the handle's next call is bit-exact."""
    L, R, _ = S.make_pair(64, 160, 32, seed=55)
    m = sdr.StereoSGBM.create(0, 32, 5, 600, 20000, 1, 63, 12, 30, 2, 0)
    with pytest.raises(sdr.SDRError):
        m.compute(L, R)
    with pytest.raises(sdr.SDRError):
        m.compute_reproject(L, R, S.REFERENCE_Q, True)
    m.setP2(2400)
    ref = oracle.sgbm_compute(L, R, oracle.make_params(0, 32, 5, 600, 2400, 1, 63, 12, 30, 2, 0))
    assert np.array_equal(m.compute(L, R), ref)


def test_graph_capture_replay(oracle):
    """The device enqueue captured into a graph (torch.cuda.graph: hipStreamBeginCapture on a side
    stream) and replayed on new inputs: after a first call nothing is allocated, so the launches
    replay as captured.  Also a batched MODE_HH call, which takes k_paths' chains inside a capture
    (the row sweeps are not captured)."""
    dev = torch.device("cuda", 0)
    for args, F, (H, W, D) in (((0, 64, 5, 600, 2400, 1, 63, 12, 50, 2, 0), 2, (48, 200, 64)),
                               ((0, 32, 5, 600, 2400, 1, 63, 10, 0, 2, sdr.MODE_HH), 8, (24, 120, 32))):
        Ls, Rs = S.make_batch(F, H, W, D, seed0=500)
        Ld, Rd = torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)
        m = sdr.StereoSGBM.create(*args)
        m.compute(Ld, Rd)  # sizes the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m.compute(Ld, Rd)
        p = oracle.make_params(*args)
        for seed in (600, 700):
            L2, R2 = S.make_batch(F, H, W, D, seed0=seed)
            Ld.copy_(torch.from_numpy(L2))
            Rd.copy_(torch.from_numpy(R2))
            g.replay()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for i in range(F):
                assert np.array_equal(got[i], oracle.sgbm_compute(L2[i], R2[i], p)), (args[10], seed, i)
        # the handle is still usable directly after the capture
        again = m.compute(Ld, Rd)
        torch.cuda.synchronize()
        assert np.array_equal(again.cpu().numpy(), got)
        m.close()


def test_graph_capture_compute_reproject(oracle):
    """The fused pcd_write hot path (compute -> /16 -> reprojectImageTo3D with handleMissing, the
    frame minimum included) captured once and replayed on new frames, bit-exact."""
    dev = torch.device("cuda", 0)
    args, (H, W, D) = (0, 64, 5, 600, 2400, 1, 63, 12, 60, 2, 0), (56, 224, 64)
    L, R, _ = S.make_pair(H, W, D, seed=801)
    Ld, Rd = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    m = sdr.StereoSGBM.create(*args)
    m.compute_reproject(Ld, Rd, S.REFERENCE_Q, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        disp, xyz = m.compute_reproject(Ld, Rd, S.REFERENCE_Q, True)
    p = oracle.make_params(*args)
    for seed in (802, 803):
        L2, R2, _ = S.make_pair(H, W, D, seed=seed)
        Ld.copy_(torch.from_numpy(L2))
        Rd.copy_(torch.from_numpy(R2))
        g.replay()
        torch.cuda.synchronize()
        ref = oracle.sgbm_compute(L2, R2, p)
        assert np.array_equal(disp[0].cpu().numpy(), ref), seed
        ref_xyz = oracle.reproject(oracle.disp_to_float(ref), S.REFERENCE_Q, True)
        assert np.array_equal(xyz[0].cpu().numpy().view(np.uint32), ref_xyz.view(np.uint32)), seed
    m.close()


@pytest.mark.parametrize("mode,D,H,W,seed,batch", [
    (2, 80, 601, 701, 31, 1),     # 3WAY, padded lanes (D < 128), odd row and column chain counts
                                  # (one-chain last waves / workgroups)
    (2, 128, 576, 800, 32, 1),    # 3WAY at D = 128 (no padding)
    (3, 64, 520, 600, 33, 1),     # MODE_HH4: E, W and N chains
    (2, 48, 300, 420, 34, 4),     # a batch: 4 x 600 chains
])
def test_two_chain_paths(oracle, mode, D, H, W, seed, batch):
    """k_paths with two chains per wave (launches of E/W/N chains with more chains than SIMDs, D <=
    128: the class path's paired 640x360 matchers) and k_south_wta with two columns per workgroup
    (more than 8 x CUs column chains: the 3WAY cases here) against the oracle, frame by frame."""
    args = (0, D, 5, 600, 2400, 1, 63, 10, 0, 2, mode)
    Ls = np.empty((batch, H, W), np.uint8)
    Rs = np.empty((batch, H, W), np.uint8)
    for i in range(batch):
        Ls[i], Rs[i], _ = S.make_pair(H, W, D, seed=seed + i)
    dev = torch.device("cuda", 0)
    m = sdr.StereoSGBM.create(*args)
    out = m.compute(torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)).cpu().numpy()
    p = oracle.make_params(*args)
    for i in range(batch):
        ref = oracle.sgbm_compute(Ls[i], Rs[i], p)
        assert np.array_equal(out[i], ref), f"frame {i}: {(out[i] != ref).sum()} px differ"
    m.close()


def test_two_chain_paths_randomized(oracle):
    """Random shapes and parameters where the two-chain kernels engage (> 1024 E/W chains, > 2048
    3WAY column chains, D <= 128), adversarial pairs included (int16 extremes)."""
    pytest.importorskip("hypothesis")
    from hypothesis import HealthCheck, given, settings

    from conftest import hyp_examples
    from hypothesis import strategies as st

    @settings(max_examples=hyp_examples(6), deadline=None, derandomize=True, database=None,
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
    @given(D=st.integers(1, 8).map(lambda k: 16 * k), H=st.integers(520, 640), W1=st.integers(520, 760),
               mode=st.sampled_from([2, 3]), bs=st.sampled_from([3, 5, 7]), P1=st.integers(1, 600),
               P2x=st.integers(2, 6), kind=st.sampled_from(["textured", "noise", "binary", "steps"]),
               seed=st.integers(0, 10**6))
    def run(D, H, W1, mode, bs, P1, P2x, kind, seed):
        W = W1 + D
        args = (0, D, bs, P1, P1 * P2x, 1, 63, 10, 0, 2, mode)
        if kind == "textured":
            L, R, _ = S.make_pair(H, W, D, seed=seed)
        else:
            L, R = S.adversarial_pair(kind, H, W, D, seed=seed)
        dev = torch.device("cuda", 0)
        m = sdr.StereoSGBM.create(*args)
        out = m.compute(torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)).cpu().numpy()
        ref = oracle.sgbm_compute(L, R, oracle.make_params(*args))
        m.close()
        assert np.array_equal(out, ref), f"{(out != ref).sum()} px differ"

    run()
