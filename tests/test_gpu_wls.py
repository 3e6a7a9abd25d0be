"""GPU parity of the class path's post-filter: ximgproc DisparityWLSFilter
+ FastGlobalSmootherFilter on the HIP engine against the CPU restatement (oracle/wls_oracle.c).

The kernels evaluate every float operation in the oracle's order with contraction off, IEEE
division and the oracle's host-computed weight table, so the filtered int16 map, the confidence
map and raw FGS output are compared BIT FOR BIT -- for both line solvers: SDR_FGS_THOMAS
(ximgproc's sequential elimination, the default since round 5) against the oracle's fgs_line,
SDR_FGS_PCR (parallel cyclic reduction, opt-in) against its fgs_line_pcr.  The two solvers agree
within 1 int16 level on the reference's own frames (test_pcr_within_one_level_of_thomas) but not
where the confidence map is sparse (test_default_solver_hypothesis records how far PCR strays:
hundreds of levels on some pixels, profiles/r5_pcr_vs_thomas.json), which is why the default is
ximgproc's order.  Parity of the oracle itself against opencv_contrib is unpinned (no OpenCV in
this image, no fixtures in the reference): see oracle/wls_oracle.h and tests/test_oracle_wls.py
for how the restatement is pinned.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd.ximgproc import createDisparityWLSFilter, fastGlobalSmootherFilter  # noqa: E402
from stereo_depth_ruler_amd._lib import FGS_PCR, FGS_THOMAS  # noqa: E402

from fgs_cases import bits, hyp_case, make_filter, sgbm_pair_maps  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


SOLVERS = [FGS_PCR, FGS_THOMAS]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (29, 1), (40, 61), (64, 64), (65, 129),
                                   (97, 130), (200, 333), (3, 1000), (700, 5)])
@pytest.mark.parametrize("lam,sigma", [(8000.0, 1.1), (50.0, 5.0)])
def test_fgs_bit_exact(oracle, shape, lam, sigma, solver):
    rng = np.random.default_rng(sum(shape))
    g = rng.integers(0, 256, shape).astype(np.uint8)
    g[: shape[0] // 2] //= 8
    x = (rng.random(shape) * 1000).astype(np.float32)
    ref = oracle.fgs_filter(g, x, lam, sigma, solver=solver)
    got = fastGlobalSmootherFilter(g, x, lam, sigma, solver=solver)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("solver", SOLVERS)
def test_fgs_stack_and_iterations(oracle, solver):
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (70, 90)).astype(np.uint8)
    xs = (rng.random((3, 70, 90)) * 300).astype(np.float32)
    got = fastGlobalSmootherFilter(g, xs, 8000.0, 1.1, 0.25, 5, solver=solver)
    for i in range(3):
        ref = oracle.fgs_filter(g, xs[i], 8000.0, 1.1, 0.25, 5, solver=solver)
        assert np.array_equal(bits(got[i]), bits(ref))


@pytest.mark.parametrize("shape", [(2, 1500), (3, 3000), (2, 3840), (3840, 2), (3, 4096), (4096, 3)])
def test_pcr_long_lines(oracle, shape):
    """k_fgs_pcr on lines past 1024 samples (2 and 4 equations per thread) and past the 3413 whose
    double-buffered stages (48 B/sample) exceed a workgroup's 160 KiB of LDS, which then take the
    single-buffered form (24 B/sample): rows (w long) and columns (h long), up to the 4096 limit.
    A 4K frame's 3840-sample rows run here."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    g = rng.integers(0, 256, shape).astype(np.uint8)
    x = (rng.random(shape) * 1000).astype(np.float32)
    for lam, sigma in ((8000.0, 1.1), (50.0, 5.0)):
        ref = oracle.fgs_filter(g, x, lam, sigma, solver=FGS_PCR)
        got = fastGlobalSmootherFilter(g, x, lam, sigma, solver=FGS_PCR)
        assert np.array_equal(bits(got), bits(ref)), (shape, lam)


def test_pcr_line_limit():
    g = np.zeros((2, 4097), np.uint8)
    x = np.ones((2, 4097), np.float32)
    with pytest.raises(sdr.SDRError):
        fastGlobalSmootherFilter(g, x, 8000.0, 1.1, solver=FGS_PCR)
    assert np.allclose(fastGlobalSmootherFilter(g, x, 8000.0, 1.1, solver=FGS_THOMAS), 1.0, rtol=1e-3)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("h,w,numD,seed", [(360, 640, 80, 1), (90, 200, 32, 2), (50, 121, 16, 3)])
def test_wls_filter_bit_exact_on_sgbm_maps(oracle, h, w, numD, seed, solver):
    L, dl, dr = sgbm_pair_maps(oracle, h, w, numD, seed)
    q = oracle.wls_params_for_sgbm(0, numD, 5, w, h, 8000.0, 1.1)
    q.fgs_solver = solver
    ref, ref_conf = oracle.wls_filter(dl, dr, L, q, return_conf=True)
    f = make_filter(q, w, h)
    got = f.filter(dl, L, dr)
    assert np.array_equal(bits(f.getConfidenceMap()), bits(ref_conf))
    assert np.array_equal(got, ref)
    assert f.getROI(w, h) == (q.roi_x, q.roi_y, q.roi_w, q.roi_h)


@pytest.mark.parametrize("seed", list(range(1, 21)))
def test_pcr_within_one_level_of_thomas(oracle, seed):
    """The opt-in PCR solver against ximgproc's sequential one (the default) on the reference's own
    workload (C0: 640x360 d=80 3WAY left + right matcher maps of a live-loop frame): the north-star
    tolerance, <= 1 int16 level (1/16 px) everywhere.  Both come from the device."""
    from stereo_depth_ruler_amd.synthetic import sbs_bgr_color_frame
    frame = sbs_bgr_color_frame(720, 1280, 80, seed=seed)
    gl = oracle.resize_area_half(oracle.bgr2gray(frame[:, :1280]))
    gr = oracle.resize_area_half(oracle.bgr2gray(frame[:, 1280:]))
    dl = oracle.sgbm_compute(gl, gr, oracle.make_params(0, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    dr = oracle.sgbm_compute(gr, gl, oracle.make_params(-79, 80, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    q = oracle.wls_params_for_sgbm(0, 80, 5, 640, 360, 8000.0, 1.1)
    f = make_filter(q, 640, 360)
    f.setFgsSolver(FGS_PCR)
    pcr = f.filter(dl, gl, dr).astype(np.int32)
    f.setFgsSolver(FGS_THOMAS)
    tho = f.filter(dl, gl, dr).astype(np.int32)
    d = np.abs(pcr - tho)
    same = float((d == 0).mean())
    print(f"seed {seed}: max |PCR - THOMAS| = {d.max()} level(s), {100 * same:.3f} % bit-identical")
    assert d.max() <= 1
    assert same > 0.999


@pytest.mark.parametrize("solver", SOLVERS)
def test_wls_params_variants(oracle, solver):
    """radius, LRC threshold, lambda/sigma, minDisparity < 0 (both ROI offsets), ROI y offsets."""
    rng = np.random.default_rng(9)
    h, w = 77, 190
    base = rng.integers(2, 40, (h // 6 + 1, w // 6 + 1)) * 16
    dl = np.repeat(np.repeat(base, 6, 0), 6, 1)[:h, :w].astype(np.int16)
    dr = -np.roll(dl, -3, 1)
    dl[rng.random((h, w)) < 0.05] = -16
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    for (minD, numD, bs, lam, sig, thr) in ((0, 48, 5, 8000.0, 1.1, 24), (-10, 32, 3, 500.0, 3.0, 40),
                                            (4, 16, 9, 8000.0, 1.5, 8)):
        q = oracle.wls_params_for_sgbm(minD, numD, bs, w, h, lam, sig)
        q.lrc_thresh = thr
        q.roi_y, q.roi_h = 3, h - 7
        q.fgs_solver = solver
        ref, ref_conf = oracle.wls_filter(dl, dr, g, q, return_conf=True)
        f = make_filter(q, w, h)
        got = f.filter(dl, g, dr)
        assert np.array_equal(bits(f.getConfidenceMap()), bits(ref_conf)), (minD, numD, bs)
        assert np.array_equal(got, ref), (minD, numD, bs)


@pytest.mark.parametrize("radius", [1, 4, 5, 9, 10])
def test_wls_radius_paths(oracle, radius):
    """setDepthDiscontinuityRadius across the front end's paths: k_wls_prep with 4 (r <= 4) or 9
    (r <= 9) taps unrolled, and past 9 the per-pixel kernels with k_wls_final; with the default
    solver the first two write the outputs outside the ROI in k_wls_prep and the ROI's in the last
    FGS pass, the third in k_wls_final."""
    h, w = 61, 150
    L, dl, dr = sgbm_pair_maps(oracle, h, w, 32, 40 + radius)
    q = oracle.wls_params_for_sgbm(0, 32, 5, w, h, 8000.0, 1.1)
    q.depth_disc_radius = radius
    q.roi_y, q.roi_h = 2, h - 5
    ref, ref_conf = oracle.wls_filter(dl, dr, L, q, return_conf=True)
    f = make_filter(q, w, h)
    got = f.filter(dl, L, dr)
    assert np.array_equal(bits(f.getConfidenceMap()), bits(ref_conf))
    assert np.array_equal(got, ref), (got != ref).sum()


@pytest.mark.parametrize("solver", SOLVERS)
def test_wls_edge_cases(oracle, solver):
    h, w = 40, 120
    g = np.random.default_rng(1).integers(0, 256, (h, w)).astype(np.uint8)
    cases = [
        (np.full((h, w), 320, np.int16), np.full((h, w), -320, np.int16)),        # consistent
        (np.full((h, w), 512, np.int16), np.full((h, w), 80, np.int16)),          # all LR fail -> 0
        (np.full((h, w), -16, np.int16), np.full((h, w), -1280, np.int16)),       # all invalid
        (np.random.default_rng(2).integers(-32768, 32767, (h, w)).astype(np.int16),
         np.random.default_rng(3).integers(-32768, 32767, (h, w)).astype(np.int16)),  # extremes
    ]
    q = oracle.wls_params_for_sgbm(0, 32, 5, w, h, 8000.0, 1.1)
    q.fgs_solver = solver
    f = make_filter(q, w, h)
    for dl, dr in cases:
        ref, ref_conf = oracle.wls_filter(dl, dr, g, q, return_conf=True)
        got = f.filter(dl, g, dr)
        assert np.array_equal(bits(f.getConfidenceMap()), bits(ref_conf))
        assert np.array_equal(got, ref)
    # empty ROI (numDisparities >= width): everything is the fill value
    q2 = oracle.wls_params_for_sgbm(0, 128, 5, w, h)
    f2 = make_filter(q2, w, h)
    got = f2.filter(cases[0][0], g, cases[0][1])
    assert (got == -16).all()


def test_wls_device_batch_equals_frames(oracle):
    maps = [sgbm_pair_maps(oracle, 64, 160, 32, s) for s in (11, 12, 13)]
    q = oracle.wls_params_for_sgbm(0, 32, 5, 160, 64, 8000.0, 1.1)
    f = make_filter(q, 160, 64)
    dev = torch.device("cuda", 0)
    dl = torch.from_numpy(np.stack([m[1] for m in maps])).to(dev)
    dr = torch.from_numpy(np.stack([m[2] for m in maps])).to(dev)
    g = torch.from_numpy(np.stack([m[0] for m in maps])).to(dev)
    out = f.filter(dl, g, dr)
    torch.cuda.synchronize()
    for i, (L, a, b) in enumerate(maps):
        assert np.array_equal(out[i].cpu().numpy(), oracle.wls_filter(a, b, L, q))


def test_create_wls_mutates_matcher():
    m = sdr.StereoSGBM.create(0, 80, 5, 600, 2400, 1, 63, 12, 200, 2, sdr.MODE_SGBM_3WAY)
    f = createDisparityWLSFilter(m)
    assert (m.getDisp12MaxDiff(), m.getSpeckleWindowSize(), m.getUniquenessRatio()) == (1000000, 0, 0)
    p = m.params()
    assert (p.disp12MaxDiff, p.speckleWindowSize, p.uniquenessRatio) == (1000000, 0, 0)
    f.setLambda(8000.0)
    f.setSigmaColor(1.1)
    assert f.getLambda() == 8000.0 and abs(f.getSigmaColor() - 1.1) < 1e-12
    assert f.getDepthDiscontinuityRadius() == 3 and f.getROI(640, 360) == (80, 0, 560, 360)


def test_wls_wide_roi_fallback(oracle):
    """A ROI wider than k_wls_prep / k_fgs_pcr take (4096 columns): the per-pixel front end and the
    sequential solver (the default), still bit-exact; the opt-in PCR solver refuses it with
    SDR_ERR_SIZE."""
    rng = np.random.default_rng(4)
    h, w = 6, 4200
    base = rng.integers(2, 40, (h, w // 8 + 1)) * 16
    dl = np.repeat(base, 8, 1)[:, :w].astype(np.int16)
    dr = -np.roll(dl, -2, 1)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    q = oracle.wls_params_for_sgbm(0, 32, 5, w, h, 8000.0, 1.1)
    assert q.fgs_solver == FGS_THOMAS
    f = make_filter(q, w, h)
    ref, ref_conf = oracle.wls_filter(dl, dr, g, q, return_conf=True)
    got = f.filter(dl, g, dr)
    assert np.array_equal(bits(f.getConfidenceMap()), bits(ref_conf))
    assert np.array_equal(got, ref)
    f.setFgsSolver(FGS_PCR)
    with pytest.raises(sdr.SDRError):
        f.filter(dl, g, dr)


def test_default_solver_hypothesis(oracle):
    """The default filter (createDisparityWLSFilter's parameters, SDR_FGS_THOMAS) bit-exact with the
    oracle's sequential restatement over random shapes up to 4096-sample rows and columns, lambda in
    [10, 2e4], sigma in [0.5, 5], flat / binary-edge / noise / scene guides; and the opt-in PCR
    solver's distance from it on the same inputs, recorded (it exceeds 1 level on some cases:
    that is why the default is ximgproc's order)."""
    from hypothesis import HealthCheck, given, settings

    from conftest import hyp_examples
    from hypothesis import strategies as st

    worst = []

    @settings(max_examples=hyp_examples(24), deadline=None, derandomize=True,
              suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
    @given(shape=st.sampled_from([(40, 61), (97, 130), (8, 3840), (6, 4096), (3840, 3), (4096, 2), (160, 560),
                                  (33, 700)]),
           guide=st.sampled_from(["flat", "edge", "noise", "scene"]),
           loglam=st.floats(np.log(10.0), np.log(2e4)), sigma=st.floats(0.5, 5.0),
           seed=st.integers(0, 1 << 20))
    def run(shape, guide, loglam, sigma, seed):
        H, W = shape
        if guide == "scene" and (W < 100 or H < 8):
            guide = "noise"  # the matcher needs columns past numDisparities
        rng = np.random.default_rng(seed)
        g, dl, dr, q = hyp_case(oracle, rng, W, H, guide, float(np.exp(loglam)), sigma)
        assert q.fgs_solver == FGS_THOMAS  # the oracle's default is ximgproc's order
        ref = oracle.wls_filter(dl, dr, g, q)
        f = make_filter(q, W, H)
        assert f.getFgsSolver() == FGS_THOMAS
        got = f.filter(dl, g, dr)
        assert np.array_equal(got, ref), (shape, guide, (got != ref).sum())
        if max(W, H) <= 4096 and q.roi_w > 0 and q.roi_h > 0:
            f.setFgsSolver(FGS_PCR)
            pcr = f.filter(dl, g, dr).astype(np.int32)
            d = np.abs(pcr - ref.astype(np.int32))
            worst.append((int(d.max()), float((d > 1).mean()), shape, guide))

    run()
    worst.sort(reverse=True)
    print("PCR vs the sequential order, worst cases (levels, fraction > 1 level, shape, guide):", worst[:5])


def test_fgs_reciprocal_exact_every_mantissa():
    """The sequential solver's coefficient jobs take 1/den as v_rcp_f32 + one Newton step
    (sdr_fgs_seq.hip fgs_rcp) and its passes divide with that reciprocal (Markstein): bit-exactness rests
    on it being the IEEE quotient 1.0f / d for every d the jobs meet (1 <= d <= 1 + 2 lambda, lambda
    <= 2^100).  All 2^23 mantissas of d in [2^e, 2^(e+1)) on the device, for EVERY exponent the
    accepted parameters can reach, 0 <= e <= 125 (7 exponents were checked before)."""
    import ctypes

    from stereo_depth_ruler_amd import _lib

    failed = []
    for e in range(126):
        bad = ctypes.c_uint(123)
        assert _lib.lib().sdr_fgs_rcp_selftest(e, ctypes.byref(bad)) == 0
        if bad.value:
            failed.append((e, bad.value))
    assert not failed, failed
