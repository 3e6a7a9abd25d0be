"""GPU: the plane search (sdr_find_planes*, csrc/sdr_plane.hip) through every layer, exact against
the numpy restatement (tests/plane_search_ref.py): records as bit patterns (PR.assert_planes_equal),
counts, rounds and labels exactly."""
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

import plane_ref as PR  # noqa: E402
import plane_search_ref as SR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import PLANE_DISTANCE_DTYPE, PLANE_DTYPE, as_queries  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def to_s16(d):
    return np.nan_to_num(d * 16, nan=-16.0, posinf=32767.0, neginf=-32768.0).clip(-32768, 32767).astype(np.int16)


def make_scene(rng, H, W, planes=2, holes=0.2, outliers=0.1, sigma=0.2, weird=0.0):
    """`planes` tilted planes in vertical bands, noise on the 1/16 px grid, holes (-1), uniform
    outliers in [1, 80), a few NaN / inf / 0 / -0 / 2048."""
    ys, xs = np.mgrid[0:H, 0:W]
    band = (xs * planes) // max(W, 1)
    d = np.zeros((H, W))
    for i in range(planes):
        a, b = rng.uniform(-0.1, 0.1, 2)
        d = np.where(band == i, rng.uniform(15, 60) + a * xs + b * ys, d)
    d = (np.round((d + rng.normal(0, sigma, (H, W))) * 16) / 16).astype(np.float32)
    u = rng.random((H, W))
    d[u < holes] = -1.0
    pick = (u >= holes) & (u < holes + outliers)
    d[pick] = (np.floor(rng.uniform(1, 80, int(pick.sum())) * 16) / 16).astype(np.float32)
    pick = (u >= holes + outliers) & (u < holes + outliers + weird)
    d[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2048.0], np.float32), int(pick.sum()))
    return d[None]


def unpack(out):
    rec, count, rounds, lab = out
    torch.cuda.synchronize()
    return (rec.cpu().numpy().reshape(-1).view(PLANE_DTYPE), int(count.cpu()[0]), rounds.cpu().numpy(),
            lab.cpu().numpy() if lab is not None else None)


def search_device(disp, reg, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0, labels=True, **kw):
    r = sdr.Ruler(Qm, min_disp=min_disp, conf_min=conf_min)
    d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    return unpack(r.find_planes_device(d, reg, conf=c, labels=labels, **kw))


def assert_search_equal(got, want):
    PR.assert_planes_equal(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])
    SR.assert_rounds_equal(got[2], want[2])
    if got[3] is not None:
        bad = got[3] != want[3]
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4])


def check_search(disp, reg, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0, trace=None, **kw):
    """Device planes, count, rounds and labels == the restatement's."""
    got = search_device(disp, reg, conf=conf, Qm=Qm, min_disp=min_disp, conf_min=conf_min, **kw)
    want = SR.find_planes(disp, reg, Qm, conf=conf, min_disp=min_disp, conf_min=conf_min, trace=trace, **kw)
    assert_search_equal(got, want)
    for i in range(got[1]):  # the label histogram is the records' n_inliers
        assert int((got[3] == i).sum()) == got[0]["n_inliers"][i]
    assert int((got[3] != 255).sum()) == int(got[0]["n_inliers"].sum())
    return got


# ---- borders and tiny shapes ----
@pytest.mark.parametrize("H, W", [(5, 7), (24, 40)])
def test_borders_and_tiny_shapes(H, W):
    rng = np.random.default_rng(H)
    disp = make_scene(rng, H, W, holes=0.1, outliers=0.05)
    x1, y1 = W - 1, H - 1
    kw = dict(min_inliers=3, hypotheses=48, max_planes=3, iterations=2)
    for reg in ((0, 0, 0, 1, 1), (0, x1 - 1, y1 - 1, x1, y1), (0, 0, y1 - 1, 1, y1)):  # 2 x 2 corners
        got = check_search(disp, reg, **kw)
        assert got[0]["area"].tolist() == [4] * 3
    for reg in ((0, 0, 0, x1, 0), (0, 0, y1, x1, y1), (0, 2, 2, 2, 2), (0, 0, 0, 0, y1), (0, x1, 0, x1, y1)):
        got = check_search(disp, reg, **kw)  # N x 1, a single pixel, 1 x N: C == 0 in every hypothesis
        assert got[1] == 0 and got[2][0].tolist() == [-1, 0, 48, SR.NO_HYPOTHESIS]
        assert (got[0]["flags"] == PR.DEGENERATE).all() and (got[3] == 255).all()
    whole = check_search(disp, (0, 0, 0, x1, y1), **kw)
    assert whole[1] >= 1 and whole[0]["area"][0] == H * W
    for reg in ((0, x1, y1, 0, 0), (0, x1, 0, 0, y1), (0, 0, y1, x1, 0)):  # corners in every order
        assert_search_equal(check_search(disp, reg, **kw), whole)
    for reg in ((0, W, 0, 1, 1), (1, 0, 0, 3, 3), (0, 0, -1, 3, 3), (-1, 0, 0, 3, 3), (0, 0, 0, 3, H)):
        got = check_search(disp, reg, **kw)
        assert got[1] == 0 and (got[0]["flags"] == PR.OUT_OF_RANGE).all() and not got[0]["area"].any()
        assert (got[2][:, 3] == SR.NOT_RUN).all() and (got[3] == 255).all()


# ---- wave and workgroup remainders of the draw, score and pick kernels ----
@pytest.mark.parametrize("M", [1, 63, 65, 257, 4096])
def test_hypothesis_count_edges(M):
    disp, _, _ = SR.three_surface_scene(33, 47)
    got = check_search(disp, (0, 0, 0, 46, 32), hypotheses=M, min_inliers=40, seed=3)
    if M >= 63:
        assert got[1] >= 2
    check_search(to_s16(disp), (0, 46, 32, 2, 1), hypotheses=M, min_inliers=40, seed=4, iterations=1)


# ---- the tie rule ----
def two_parallel_planes(H=32, W=48):
    ys, xs = np.mgrid[0:H, 0:W]
    return (30.0 + 0.125 * xs - 0.0625 * ys + 10.0 * (xs >= W // 2)).astype(np.float32)[None]


def test_ties_go_to_the_lowest_index():
    """Two parallel on-grid planes 10 px apart on equal halves: the pure hypotheses of either half
    score the half's pixel count exactly.  With a seed whose first and last top-scoring hypotheses
    lie in different halves, any other tie rule picks another plane."""
    disp = two_parallel_planes()
    H, W = disp.shape[1:]
    reg = (0, 0, 0, W - 1, H - 1)
    kw = dict(hypotheses=64, min_inliers=50, max_planes=2)
    chosen = None
    for seed in range(64):
        trace = []
        SR.find_planes(disp, reg, Q, seed=seed, trace=trace, **kw)
        tab, sc = trace[0]["table"], trace[0]["scores"]
        top = np.nonzero(sc == sc.max())[0]
        side = tab["pts"][top, 0, 0] >= W // 2  # a top scorer's points all lie in one half
        if len(top) >= 2 and sc.max() == H * W // 2 and side[0] != side[-1]:
            chosen = (seed, int(top[0]), int(top[-1]), bool(side[0]))
            break
    assert chosen is not None
    seed, first, last, right = chosen
    got = check_search(disp, reg, seed=seed, **kw)
    assert got[1] == 2 and got[2][0].tolist() == [first, H * W // 2, got[2][0][2], SR.RAN] and first != last
    assert got[0]["coef"][0].tolist() == [0.125, -0.0625, 40.0 if right else 30.0]
    assert (got[3][:, W // 2:] == (0 if right else 1)).all() and (got[3][:, :W // 2] == (1 if right else 0)).all()


# ---- residuals exactly on the integer band ----
@pytest.mark.parametrize("inlier_px", [1.0, 0.53])
def test_integer_residuals_on_the_band(inlier_px):
    """Pixels planted so that their integer residual against round 0's winner is exactly Tq * |C|
    (an inlier of the score) and Tq * |C| + 1 (not one), found with the restatement's table."""
    H, W = 24, 40
    reg = (0, 0, 0, W - 1, H - 1)
    Tq = int(np.floor(np.float64(np.float32(inlier_px)) * 16.0))
    kw = dict(hypotheses=32, min_inliers=20, max_planes=2, inlier_px=inlier_px)
    found = None
    for seed in range(32):
        rng = np.random.default_rng(100 + seed)
        d16 = to_s16(make_scene(rng, H, W, planes=1, holes=0.1, outliers=0.05, sigma=0.3))
        trace = []
        SR.find_planes(d16, reg, Q, seed=seed, trace=trace, **kw)
        tab, h = trace[0]["table"], trace[0]["winner"]
        if h < 0:
            continue
        A, B, C, D = (int(tab[k][h]) for k in "ABCD")
        drawn = set(map(tuple, tab["pts"][:, :, :2].reshape(-1, 2).tolist()))
        planted = {0: 0, 1: 0}
        for v in range(H):
            for u in range(W):
                if (u, v) in drawn or d16[0, v, u] <= -16:
                    continue
                for extra in (0, 1):
                    for sign in (1, -1):
                        num = sign * (Tq * abs(C) + extra) + D - A * u - B * v
                        if planted[extra] < 3 and num % C == 0 and -32000 < num // C < 32000 and num // C > -16:
                            d16[0, v, u] = num // C
                            planted[extra] += 1
                            break
                    else:
                        continue
                    break
        trace = []
        SR.find_planes(d16, reg, Q, seed=seed, trace=trace, **kw)
        tab, h, t = trace[0]["table"], trace[0]["winner"], trace[0]
        if h < 0:
            continue
        e = np.abs(SR.integer_residuals(tab, h, t["u"], t["v"], t["q"]))
        edge = Tq * abs(int(tab["C"][h]))
        if (e == edge).any() and (e == edge + 1).any():
            found = (seed, d16, int((e <= edge).sum()))
            break
    assert found is not None
    seed, d16, score = found
    got = check_search(d16, reg, seed=seed, **kw)
    assert got[2][0][1] == score and got[2][0][3] == SR.RAN


# ---- products and sums past 32 bits ----
@pytest.mark.parametrize("H, W, M", [(3, 8192, 512), (600, 1024, 48)])
def test_wide_products(H, W, M):
    """int16 maps alternating near +-32767 with two on-plane runs.  8192 x 3: the widest rows the
    guards admit, B = dq1*du2 - du1*dq2 near 2^29 and the moment sums far past 2^32 (three rows
    keep dv <= 2, so a hypothesis' own terms stay near 2^31).  1024 x 600: A * u, B * v and the
    integer residuals themselves pass 2^32."""
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:H, 0:W]
    d16 = np.where(xs % 2 == 0, 32767 - rng.integers(0, 4, (H, W)), -32768 + rng.integers(0, 4, (H, W)))
    run = ((xs >= W // 16) & (xs < 3 * W // 16)) | ((xs >= 10 * W // 16) & (xs < 12 * W // 16))
    d16 = np.where(run, 50 + 2 * xs + 5 * ys, d16).astype(np.int16)[None]
    trace = []
    kw = dict(hypotheses=M, min_inliers=64, max_planes=3, iterations=2, min_disp=-3000.0)
    got = check_search(d16, (0, 0, 0, W - 1, H - 1), trace=trace, **kw)
    tab, t = trace[0]["table"], trace[0]
    wide = max(int(np.abs(tab["A"]).max()), int(np.abs(tab["B"]).max()))
    worst = max(int(np.abs(SR.integer_residuals(tab, int(h), t["u"], t["v"], t["q"])).max())
                for h in np.argsort(-np.maximum(np.abs(tab["A"]), np.abs(tab["B"])))[:8])
    mom = PR.moments(t["u"], t["v"], t["q"])
    print("max |A|, |B| %d, max |residual| %d, Suu %d, Suq %d" % (wide, worst, mom[4], mom[7]))
    assert mom[4] > 2 ** 36 and abs(mom[7]) > 2 ** 36
    assert wide > 2 ** 28 if H == 3 else worst > 2 ** 32
    assert got[1] == 3 and int(run.sum()) in got[0]["n_inliers"].tolist()
    k = got[0]["n_inliers"].tolist().index(int(run.sum()))
    assert got[0]["coef"][k].tolist()[:2] == [0.125, 0.3125]


# ---- validity ----
def test_validity_plants():
    H, W = 9, 30
    ys, xs = np.mgrid[0:H, 0:W]
    d = (30.0 + 0.125 * xs - 0.0625 * ys).astype(np.float32)[None]
    c = np.full((1, H, W), 100.0, np.float32)
    d[0, 1, 1:7] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2048.0], np.float32)
    d[0, 3, 2:5] = 7.0                                                       # equal to min_disp below
    d[0, 5, 3], d[0, 5, 4] = np.float32(2047.9375), np.float32(-2047.9375)  # the largest magnitudes on the grid
    c[0, 7, 10], c[0, 7, 11], c[0, 7, 12], c[0, 7, 13] = 50.0, np.float32(49.999), np.nan, np.float32(50.001)
    reg = (0, 0, 0, W - 1, H - 1)
    kw = dict(min_inliers=3, hypotheses=64, max_planes=3)
    got = check_search(d, reg, conf=c, min_disp=7.0, conf_min=50.0, **kw)
    # NaN, +-inf, 0, -0 (<= 7), 2048, three sevens, -2047.9375, and the confidences 49.999 and NaN
    assert got[0]["n_valid"][0] == H * W - (6 + 3 + 1 + 2)
    got = check_search(d, reg, conf=c, min_disp=-1.0, conf_min=50.0, **kw)
    assert got[0]["n_valid"][0] == H * W - (4 + 1 + 2)  # 0 and -0 are valid now, the sevens too
    got = check_search(d, reg, min_disp=-3000.0, iterations=1, **kw)
    assert got[0]["n_valid"][0] == H * W - 4            # the non-finite values and 2048
    check_search(d, reg, conf_min=float("nan"), **kw)   # no part without a confidence map
    got = check_search(d, reg, conf=c, conf_min=float("nan"), **kw)
    assert got[1] == 0 and got[2][0].tolist() == [-1, 0, 64, SR.NO_HYPOTHESIS]
    d16 = to_s16(d)
    d16[0, 5, 3], d16[0, 5, 4], d16[0, 3, 2:5] = 32767, -32768, 112
    got = check_search(d16, reg, conf=c, min_disp=7.0, conf_min=50.0, **kw)
    assert got[0]["n_valid"][0] == int(((d16[0] > 112) & ~(c[0] < 50.0) & ~np.isnan(c[0])).sum())


# ---- the whole frame ----
@pytest.fixture(scope="module")
def frame():
    """One 360 x 640 three-surface frame, its restatement at M = 256 computed once."""
    disp, truth, _ = SR.three_surface_scene(360, 640)
    reg = (0, 0, 0, 639, 359)
    kw = dict(hypotheses=256, min_inliers=1000, max_planes=4)
    return disp, reg, kw, SR.find_planes(disp, reg, Q, **kw), truth


def test_whole_frame(frame):
    disp, reg, kw, want, truth = frame
    got = search_device(disp, reg, **kw)
    assert_search_equal(got, want)
    assert got[1] == 3 and got[2][3][3] in (SR.LOW_SCORE, SR.NO_HYPOTHESIS)
    hist = np.bincount(got[3].reshape(-1), minlength=256)
    assert hist[:3].tolist() == got[0]["n_inliers"][:3].tolist() and hist[3:255].sum() == 0
    # (at this size the floor and the box cross inside the box's rectangle, so purity is not asked
    # here: test_plane_search_cpu.py checks it on the 320 x 240 scene)
    assert (got[3][truth < 0] == 255).mean() > 0.9
    # again, and without a label map: the same records
    assert_search_equal(search_device(disp, reg, **kw), want)
    again = search_device(disp, reg, labels=False, **kw)
    assert again[3] is None
    assert_search_equal(again, want)
    # rows and frames padded: the same
    pad = torch.full((2, 364, 650), -7.0, dtype=torch.float32, device=dev())
    pad[1, :360, :640] = torch.from_numpy(disp[0]).to(dev())
    view = pad[:, :360, :640]
    assert view.stride(1) == 650 and view.stride(0) == 364 * 650
    out = unpack(sdr.Ruler(Q).find_planes_device(view, (1, 0, 0, 639, 359), labels=True, **kw))
    w1 = want[0].copy()
    w1["frame"] = 1
    assert_search_equal(out, (w1,) + want[1:])


# ---- the stop codes ----
def find_stop_scenes():
    """Scenes (seed, map, min_inliers) whose round 0 passes the pick with min_inliers equal to the
    winner's score and then stops in a refit (fewer pixels in a later set) and in the statistics."""
    found = {}
    for seed in range(400):
        rng = np.random.default_rng(1000 + seed)
        disp = make_scene(rng, 20, 30, planes=2, holes=0.2, outliers=0.3, sigma=0.8)
        trace = []
        SR.find_planes(disp, (0, 0, 0, 29, 19), Q, hypotheses=32, seed=seed, min_inliers=3, max_planes=1,
                       trace=trace)
        s0 = int(trace[0]["scores"].max())
        _, count, rounds, _ = SR.find_planes(disp, (0, 0, 0, 29, 19), Q, hypotheses=32, seed=seed, min_inliers=s0,
                                             max_planes=2)
        code = int(rounds["stop"][0])
        if code in (SR.REFIT_DEGENERATE, SR.FEW_INLIERS) and code not in found:
            found[code] = (seed, disp, s0)
        if len(found) == 2:
            break
    return found


def test_every_stop_code():
    seen = set()
    scenes = find_stop_scenes()
    assert set(scenes) == {SR.REFIT_DEGENERATE, SR.FEW_INLIERS}
    for code, (seed, disp, s0) in scenes.items():
        got = check_search(disp, (0, 0, 0, 29, 19), hypotheses=32, seed=seed, min_inliers=s0, max_planes=2)
        assert got[1] == 0 and got[2][0][3] == code and got[2][0][0] >= 0 and got[2][0][1] == s0
        assert (got[3] == 255).all() and (got[0]["flags"] == PR.DEGENERATE).all()
        seen |= set(got[2][:, 3].tolist())
    disp, _, _ = SR.three_surface_scene(33, 47)
    got = check_search(disp, (0, 0, 0, 46, 32), hypotheses=40, min_inliers=2000, max_planes=3)
    assert got[1] == 0 and got[2][0][3] == SR.LOW_SCORE and got[2][0][0] >= 0 and 3 <= got[2][0][1] < 2000
    seen |= set(got[2][:, 3].tolist())
    got = check_search(np.full((1, 33, 47), -1.0, np.float32), (0, 0, 0, 46, 32), hypotheses=40, max_planes=3)
    seen |= set(got[2][:, 3].tolist())
    got = check_search(disp, (0, 0, 0, 46, 32), hypotheses=40, min_inliers=100, max_planes=2)
    assert got[1] == 2
    seen |= set(got[2][:, 3].tolist())
    assert seen == {SR.RAN, SR.NO_HYPOTHESIS, SR.LOW_SCORE, SR.REFIT_DEGENERATE, SR.FEW_INLIERS, SR.NOT_RUN}


def test_eight_rounds_on_two_planes():
    disp = two_parallel_planes()
    got = check_search(disp, (0, 0, 0, 47, 31), hypotheses=64, min_inliers=50, max_planes=8)
    assert got[1] == 2 and (got[0]["flags"][:2] == PR.OK).all() and (got[0]["flags"][2:] == PR.DEGENERATE).all()
    assert np.isnan(got[0]["coef"][2:]).all() and (got[0]["area"] == 32 * 48).all() and not got[0]["n_valid"][2:].any()
    assert got[2][2].tolist() == [-1, 0, 64, SR.NO_HYPOTHESIS]  # every pixel is claimed: nothing to draw
    assert (got[2][3:] == [-1, 0, 0, SR.NOT_RUN]).all() and (got[3] != 255).all()


# ---- layers and chaining ----
def test_host_abi_and_tensor_forms():
    rng = np.random.default_rng(14)
    H, W = 27, 45
    disp = make_scene(rng, H, W, planes=3, weird=0.02)
    disp = np.concatenate([make_scene(rng, H, W), disp])  # the region's frame is 1
    conf = rng.uniform(0, 255, (2, H, W)).astype(np.float32)
    reg = (1, 2, 1, W - 1, H - 2)
    kw = dict(iterations=2, inlier_px=1.5, min_inliers=12, hypotheses=100, seed=77, max_planes=5)
    got = check_search(disp, reg, conf=conf, conf_min=30.0, **kw)
    assert got[1] >= 2
    r = sdr.Ruler(Q, conf_min=30.0)
    full = r.find_planes_full(disp, reg, conf=conf, labels=True, **kw)
    assert_search_equal((full[0], full[1], full[2].view(np.int32).reshape(-1, 4), full[3]), got)
    nolab = r.find_planes_full(disp, reg, conf=conf, **kw)
    assert nolab[3] is None
    PR.assert_planes_equal(nolab[0], got[0])
    wide = np.full((2, H, W + 3), np.nan, np.float32)  # a strided host map
    wide[:, :, :W] = disp
    planes, lab = r.find_planes(wide[:, :, :W], reg, conf=conf, labels=True, **kw)
    PR.assert_planes_equal(planes, got[0][:got[1]])
    assert np.array_equal(lab, got[3])
    t_planes, t_lab = r.find_planes(torch.from_numpy(disp).to(dev()), reg, conf=torch.from_numpy(conf).to(dev()),
                                    labels=True, **kw)
    PR.assert_planes_equal(t_planes, planes)
    assert np.array_equal(t_lab, lab)
    PR.assert_planes_equal(r.find_planes(torch.from_numpy(disp).to(dev()), reg, conf=torch.from_numpy(conf).to(dev()),
                                         **kw), planes)
    # region=None is all of frame 0; an int16 map through the host ABI
    d16 = to_s16(disp)
    h16 = sdr.Ruler(Q).find_planes_full(d16, None, labels=True, **kw)
    w16 = SR.find_planes(d16, (0, 0, 0, W - 1, H - 1), Q, **kw)
    assert_search_equal((h16[0], h16[1], h16[2].view(np.int32).reshape(-1, 4), h16[3]), w16)
    # a label tensor of the caller's
    mine = torch.zeros((H, W), dtype=torch.uint8, device=dev())
    out = r.find_planes_device(torch.from_numpy(disp).to(dev()), reg, conf=torch.from_numpy(conf).to(dev()),
                               labels_out=mine, **kw)
    assert out[3] is mine
    assert_search_equal(unpack(out), got)


def test_search_and_queries_chain_on_one_stream():
    """The planes tensor of find_planes_device feeds plane_distance_device on the same side stream
    with no host round trip (records past the count are not PLANE_OK: NO_PLANE)."""
    disp, _, _ = SR.three_surface_scene(60, 80)
    rng = np.random.default_rng(13)
    pts = as_queries([(0, int(x), int(y), int(p)) for x, y, p in
                      zip(rng.integers(0, 80, 64), rng.integers(0, 60, 64), rng.integers(0, 5, 64))])
    r = sdr.Ruler(Q, radius=1, min_count=2)
    d = torch.from_numpy(disp).to(dev())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(hypotheses=128, min_inliers=200, max_planes=4)
    out = r.find_planes_device(d, None, stream=side, labels=True, **kw)
    dist_t = r.plane_distance_device(d, out[0], pts, stream=side)
    side.synchronize()
    want = SR.find_planes(disp, (0, 0, 0, 79, 59), Q, **kw)
    assert_search_equal(unpack(out), want)
    assert want[1] == 3
    PR.assert_distances_equal(dist_t.cpu().numpy().reshape(-1).view(PLANE_DISTANCE_DTYPE),
                              PR.plane_distance(disp, want[0], pts, Q, radius=1, min_count=2))


def test_live_loop_find_planes_on_the_frame_stream():
    from stereo_depth_ruler_amd.pipeline import LiveLoop
    from stereo_depth_ruler_amd.rectify import StereoRectifier

    sbs = S.sbs_bgr_frame(96, 400, 80, seed=21)
    H, W = sbs.shape[0], sbs.shape[1] // 2
    K = np.array([[700.0, 0, W / 2], [0, 700.0, H / 2], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    cfg = types.SimpleNamespace(imageSize=(W, H), cameraMatrixLeft=K, cameraMatrixRight=K, distCoeffsLeft=None,
                                distCoeffsRight=None, R1=np.eye(3), R2=np.eye(3), P1=P, P2=P)
    rect = StereoRectifier(cfg)
    frame = torch.from_numpy(sbs[None]).to(dev())
    plain = LiveLoop(rect, Q, 1)
    with pytest.raises(RuntimeError):
        plain.find_planes(None, torch.cuda.current_stream(dev()))
    plain.close()
    loop = LiveLoop(rect, Q, 1, ruler=dict(radius=1, min_count=2, conf_min=100.0))
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(max_planes=3, hypotheses=96, iterations=2, inlier_px=2.0, min_inliers=30)
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        out = loop.find_planes(None, side, labels=True, **kw)
        reg_out = loop.find_planes((0, 150, 30, 60, 10), side, **kw)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    got = unpack(out)
    full = loop.ruler.find_planes_full(disp, None, conf=conf, labels=True, **kw)
    assert_search_equal(got, (full[0], full[1], full[2], full[3]))
    assert_search_equal(got, SR.find_planes(disp, (0, 0, 0, loop.w2 - 1, loop.h2 - 1), Q, conf=conf,
                                            min_disp=loop.ruler.min_disp, conf_min=100.0, **kw))
    assert_search_equal(unpack(reg_out), SR.find_planes(disp, (0, 150, 30, 60, 10), Q, conf=conf,
                                                        min_disp=loop.ruler.min_disp, conf_min=100.0, **kw)[:3] + (None,))
    assert got[0]["n_valid"][0] > 0
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()


def test_cpp_facade_plane_search(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::find_planes gives Python's records, rounds and labels as
    bytes (tests/cpp/facade_plane_search.cpp)."""
    exe = tmp_path / "facade_plane_search"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_plane_search.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    rng = np.random.default_rng(15)
    H, W = 29, 43
    disp = make_scene(rng, H, W, planes=2, weird=0.02)
    conf = rng.uniform(0, 255, (1, H, W)).astype(np.float32)
    disp[0].tofile(tmp_path / "disp.bin")
    conf[0].tofile(tmp_path / "conf.bin")
    np.asarray(Q, np.float64).tofile(tmp_path / "q.bin")
    reg = (0, W - 1, 1, 2, H - 1)
    res = subprocess.run([str(exe), str(W), str(H), *(str(t) for t in reg[1:]), "5", "70", "4000000000",
                          str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "no_labels_equal=1" in res.stdout and "bad_max_planes_code=-1" in res.stdout
    want = search_device(disp, reg, conf=conf, conf_min=10.0, max_planes=5, hypotheses=70, seed=4000000000,
                         iterations=2, inlier_px=1.5, min_inliers=6)
    assert want[1] >= 2 and f"count={want[1]} rounds=5" in res.stdout
    assert (tmp_path / "planes.bin").read_bytes() == want[0][:want[1]].tobytes()
    assert (tmp_path / "rounds.bin").read_bytes() == np.ascontiguousarray(want[2]).tobytes()
    assert (tmp_path / "labels.bin").read_bytes() == want[3].tobytes()


# ---- hypothesis ----
@settings(max_examples=hyp_examples(30), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(1, 64), W=st.integers(1, 64), M=st.integers(1, 96), iterations=st.integers(1, 8),
       max_planes=st.integers(1, 8), min_inliers=st.integers(3, 40), inlier_q=st.integers(1, 64),
       with_conf=st.booleans(), i16=st.booleans(), seed=st.integers(0, 2 ** 32 - 1))
def test_hypothesis_random_scenes(H, W, M, iterations, max_planes, min_inliers, inlier_q, with_conf, i16, seed):
    rng = np.random.default_rng(seed)
    disp = make_scene(rng, H, W, planes=int(rng.integers(1, 4)), holes=float(rng.uniform(0, 0.6)),
                      outliers=float(rng.uniform(0, 0.3)), sigma=float(rng.uniform(0, 1.0)), weird=0.02)
    F = int(rng.integers(1, 3))
    if F == 2:
        disp = np.concatenate([disp[:, ::-1].copy(), disp])
    if i16:
        disp = to_s16(disp)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32) if with_conf else None
    reg = [int(rng.integers(0, F)), int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, W)),
           int(rng.integers(0, H))]
    if rng.random() < 0.5:
        reg[1:] = [0, 0, W - 1, H - 1]
    if rng.random() < 0.2:
        reg[int(rng.integers(0, 5))] = int(rng.choice([-1, 100]))
    check_search(disp, tuple(reg), conf=conf, conf_min=float(rng.uniform(0, 200)), hypotheses=M, seed=seed,
                 iterations=iterations, max_planes=max_planes, inlier_px=inlier_q / 8.0, min_inliers=min_inliers)
