"""GPU: the footprint (sdr_plane_footprint*, csrc/sdr_footprint.hip) through every layer, every
record compared bit for bit with the numpy restatement (tests/footprint_ref.py)."""
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

import footprint_ref as FR  # noqa: E402
import plane_ref as PR  # noqa: E402
import plane_search_ref as SR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import FOOTPRINT_DTYPE, PLANE_DTYPE, as_relief_queries  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q
EYE = np.eye(4)
SLICE = 2048  # pixels a workgroup of the sweeps (csrc/sdr_region.hpp, kRegionSlice)
TILE = 16     # cells a side of a workgroup's tile in the cell pass (kFootTile)
BATCH = 256   # queries a batch at most (kFootBatch); fewer when their grids would pass 64 MiB


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def to_s16(d):
    return np.nan_to_num(d * 16, nan=-16.0, posinf=32767.0, neginf=-32768.0).clip(-32768, 32767).astype(np.int16)


def records(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(-1).view(FOOTPRINT_DTYPE)


def check_foot(disp, planes, regions, labels=None, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0, **kw):
    """Device records == the restatement's, on every bit."""
    r = sdr.Ruler(Qm, min_disp=min_disp, conf_min=conf_min)
    d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev()) if labels is not None else None
    got = records(r.footprint_device(d, planes, regions, labels=lab, conf=c, **kw))
    want = FR.footprint(disp, planes, regions, Qm, labels=labels, conf=conf, min_disp=min_disp, conf_min=conf_min,
                        **kw)
    FR.assert_footprints_equal(got, want)
    return got


def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """With Q the identity and this record s = x, t = y and h = d + offset."""
    p = np.zeros(1, PLANE_DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def planted(H, W, pts, d=5.0):
    m = np.full((1, H, W), -1.0, np.float32)
    for x, y in pts:
        m[0, y, x] = d
    return m


def rect_pts(x0, y0, x1, y1):
    return [(x, y) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]


# ---- planted maps, Q the identity ----
@pytest.mark.parametrize("H,W", [(8, 8), (48, 64)])
def test_planted_identities(H, W):
    pl = flat_plane()
    whole = [(0, 0, 0, W - 1, H - 1, 0, -1)]
    kw = dict(Qm=EYE, cell=1.0, support=1)
    x1, y1 = W - 3, H - 2
    full = planted(H, W, rect_pts(2, 1, x1, y1))
    for grid in (16, 17, 33, 65, 512):  # cell-pass tiles end mid-grid
        got = check_foot(full, pl, whole, grid=grid, **kw)
        if grid >= W:
            assert got["angle_deg"][0] == 0 and got["side"][0].tolist() == [x1 - 1.0, y1 - 0.0] and got["fill"][0] == 1.0
            assert got["corner"][0].tolist() == [[2, 1, 0], [x1 + 1, 1, 0], [x1 + 1, y1 + 1, 0], [2, y1 + 1, 0]]
        else:
            assert got["flags"][0] == FR.VALID | FR.CLIPPED and got["n_outside"][0] > 0
    # kept cells on all four grid borders: the support neighbours outside the grid count 0
    ring = planted(H, W, rect_pts(0, 0, W - 1, H - 1))
    for support in (1, 4, 6, 9):
        got = check_foot(ring, pl, whole, Qm=EYE, cell=1.0, support=support, grid=16)
        assert got["n_cells_raw"][0] == min(16, W) * min(16, H)
    if W > 16:  # borders of the grid, not of the map: rows and columns 0 and 15 of a clipped set
        assert check_foot(ring, pl, whole, Qm=EYE, cell=1.0, support=6, grid=16)["n_cells"][0] == 256 - 4
    else:
        assert check_foot(ring, pl, whole, Qm=EYE, cell=1.0, support=6, grid=16)["n_cells"][0] == H * W - 4
    # all members in one cell; one member; no member; no cell with support
    lab = np.zeros((1, H, W), np.uint8)
    lab[0, 3, 4] = 7
    got = check_foot(planted(H, W, rect_pts(4, 4, 7, 7)), pl, whole, Qm=EYE, cell=4.0, support=1, grid=16)
    assert got["side"][0].tolist() == [4.0, 4.0] and got["n_cells"][0] == 1 and got["n"][0] == 16
    got = check_foot(planted(H, W, [(4, 3)]), pl, whole, grid=16, **kw)
    assert got["side"][0].tolist() == [1.0, 1.0] and got["corner"][0][0].tolist() == [4.0, 3.0, 0.0]
    got = check_foot(full, pl, [(0, 0, 0, W - 1, H - 1, 0, 7)], labels=lab, grid=16, **kw)  # under a label
    assert got["n"][0] == 1 and got["n_masked"][0] == 1 and got["flags"][0] == FR.VALID
    got = check_foot(planted(H, W, []), pl, whole, grid=16, **kw)
    assert got["flags"][0] == FR.EMPTY and got["n"][0] == 0
    got = check_foot(planted(H, W, [(1, 1), (5, 6)]), pl, whole, Qm=EYE, cell=1.0, support=2, grid=16)
    assert got["flags"][0] == FR.EMPTY and got["n"][0] == 2 and got["n_cells_raw"][0] == 2
    # support 9 drops an isolated block, h_range excludes by height, negative s and exact boundaries
    m = planted(H, W, rect_pts(0, 0, 1, 1) + rect_pts(3, 3, 7, 7), d=5.0)
    m[0, 0:2, 0:2] = 9.0
    got = check_foot(m, pl, whole, Qm=EYE, cell=1.0, support=9, grid=16)
    assert got["n_cells"][0] == 9 and got["side"][0].tolist() == [3.0, 3.0]
    got = check_foot(m, pl, whole, Qm=EYE, cell=1.0, support=1, grid=16, h_range=(4.0, 6.0))
    assert got["n"][0] == 25 and got["n_valid"][0] == 29 and got["side"][0].tolist() == [5.0, 5.0]
    Qs = np.eye(4)
    Qs[0, 3], Qs[1, 3] = -4.0, -3.5
    got = check_foot(m, flat_plane(-5.0), whole, Qm=Qs, cell=2.0, support=1, grid=16)
    assert got["i0"][0] == -2 and got["j0"][0] == -2 and got["corner"][0][0].tolist() == [-4.0, -4.0, 5.0]


def test_directions_on_turned_shapes():
    """Shapes whose best direction is not 0: a diamond (45), slanted strips, with tiles ending mid-grid."""
    H, W = 60, 90
    pl = flat_plane()
    whole = [(0, 0, 0, W - 1, H - 1, 0, -1)]
    pts = [(45 + a, 30 + b) for a in range(-20, 21) for b in range(-20, 21) if abs(a) + abs(b) <= 20]
    got = check_foot(planted(H, W, pts), pl, whole, Qm=EYE, cell=1.0, support=1, grid=64)
    assert got["angle_deg"][0] == 45
    angles = []
    for slope in (0.2, 0.5, 1.7, 4.0):
        pts = [(x, y) for x in range(W) for y in range(H) if abs((y - 5) - slope * (x - 10)) <= 3 and 10 <= x <= 80]
        for cell, grid in ((1.0, 128), (2.5, 37)):
            got = check_foot(planted(H, W, pts), pl, whole, Qm=EYE, cell=cell, support=2, grid=grid)
            angles.append(int(got["angle_deg"][0]))
    assert len(set(angles)) >= 4 and all(0 < a < 90 for a in angles)


# ---- shapes and edges ----
def ramp_scene(rng, F, H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    d = (30.0 + 0.05 * xs - 0.03 * ys)[None] + rng.normal(0, 0.4, (F, H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    d[rng.random((F, H, W)) < 0.15] = -1.0
    return d


@pytest.mark.parametrize("W", [63, 64, 65])
def test_region_shapes_and_corner_orders(W):
    rng = np.random.default_rng(W)
    H = 37
    d = ramp_scene(rng, 1, H, W)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1)], Q)
    x1, y1 = W - 1, H - 1
    regs = [(0, 0, 0, 0, 0), (0, x1, y1, x1, y1), (0, 5, 7, 5, 7),           # 1 x 1
            (0, 0, 3, x1, 3), (0, 0, y1, x1, y1), (0, 4, 0, 4, y1), (0, x1, 0, x1, y1),  # 1 x N, N x 1
            (0, 0, 0, x1, y1), (0, x1, y1, 0, 0), (0, x1, 0, 0, y1), (0, 0, y1, x1, 0),  # the frame, every order
            (0, 3, 30, 50, 2), (0, 50, 2, 3, 30)]
    got = check_foot(d, planes, [r + (0, -1) for r in regs], cell=16.0, grid=64, support=2)
    for i in (8, 9, 10):
        assert got[i].tobytes() == got[7].tobytes()
    assert got[11].tobytes() == got[12].tobytes() and got["area"][7] == H * W and got["area"][0] == 1
    assert got["flags"][7] == FR.VALID
    check_foot(to_s16(d), planes, [r + (0, -1) for r in regs], cell=16.0, grid=64, support=2)


def test_slice_edges_and_larger_frames():
    rng = np.random.default_rng(7)
    W, H = SLICE + 1, 3
    d = ramp_scene(rng, 1, H, W)
    planes = PR.fit_planes(d, [(0, 0, 0, 200, H - 1)], Q)
    assert planes["flags"][0] == PR.OK
    # one slice - 1, one slice, one slice + 1, in one row and in two; the frame
    regs = [(0, 0, 1, SLICE - 2, 1, 0, -1), (0, 0, 1, SLICE - 1, 1, 0, -1), (0, 0, 1, SLICE, 1, 0, -1),
            (0, 0, 0, SLICE // 2 - 1, 1, 0, -1), (0, 0, 0, SLICE // 2, 1, 0, -1), (0, 0, 0, W - 1, H - 1, 0, -1)]
    got = check_foot(d, planes, regs, cell=16.0, grid=1024, support=1)
    assert got["area"].tolist() == [SLICE - 1, SLICE, SLICE + 1, SLICE, SLICE + 2, 3 * W]
    assert (got["flags"] & FR.VALID).all()
    # 320 x 240, and one 640 x 360 frame, with truth labels
    for Hs, Ws in ((240, 320), (360, 640)):
        disp, truth, _ = SR.three_surface_scene(Hs, Ws)
        planes = PR.fit_planes(disp, [(0, 0, (Hs * 3) // 4, Ws - 1, Hs - 1)], Q)  # the floor's lower part
        assert planes["flags"][0] == PR.OK
        lab = np.where(truth < 0, 255, truth).astype(np.uint8)
        got = check_foot(disp, planes, [(0, 0, 0, Ws - 1, Hs - 1, 0, -1), (0, 0, 0, Ws - 1, Hs - 1, 0, 1),
                                        (0, Ws // 4, Hs // 4, Ws // 2, Hs // 2, 0, 255)], labels=lab, cell=16.0)
        assert got["n"][1] == int((truth == 1).sum()) and got["n"][0] > got["n"][1] > 0
        assert got["flags"][1] == FR.VALID


# ---- records by flag ----
def test_records_by_flag():
    rng = np.random.default_rng(3)
    F, H, W = 3, 20, 30
    d = ramp_scene(rng, F, H, W)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (0, 0, 0, 0, H - 1), (1, 2, 2, W - 3, H - 3)], Q)
    assert planes["flags"].tolist() == [PR.OK, PR.DEGENERATE, PR.OK]
    lab = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    lab[:, :4] = 255
    whole = (0, 0, W - 1, H - 1)
    kw = dict(cell=16.0, grid=64, support=2)
    bad = [(3,) + whole + (0, -1), (-1,) + whole + (0, -1), (0, 0, 0, W, H - 1, 0, -1), (0, -1, 0, 3, 3, 0, -1),
           (0, 0, 0, 3, H, 0, -1), (0,) + whole + (0, 256), (0,) + whole + (0, -2)]
    got = check_foot(d, planes, bad, labels=lab, **kw)
    assert (got["flags"] == FR.OUT_OF_RANGE).all() and not got["area"].any()
    noplane = [(0,) + whole + (-1, -1), (0,) + whole + (3, -1), (0,) + whole + (1, 0)]
    got = check_foot(d, planes, noplane, labels=lab, **kw)
    assert (got["flags"] == FR.NO_PLANE).all() and (got["area"] == H * W).all() and not got["n_masked"].any()
    got = check_foot(d, planes[:0], [(0,) + whole + (0, -1)], **kw)  # no plane record at all
    assert got["flags"][0] == FR.NO_PLANE
    nf = np.concatenate([planes[:1], flat_plane(normal=(np.nan, 0.0, 1.0)), flat_plane(normal=(np.inf, 1.0, 0.0))])
    got = check_foot(d, nf, [(0,) + whole + (1, -1), (0,) + whole + (2, -1), (0,) + whole + (0, -1)], **kw)
    assert got["flags"].tolist() == [FR.NO_PLANE, FR.NO_PLANE, FR.VALID]  # a basis that is not finite
    # a label without a label map is refused per record, the query beside it runs
    got = check_foot(d, planes, [(0,) + whole + (0, 1), (0,) + whole + (0, -1)], **kw)
    assert got["flags"].tolist() == [FR.OUT_OF_RANGE, FR.VALID]
    # EMPTY (a label that matches nothing, all holes), one member, CLIPPED
    holes = d.copy()
    holes[2] = -1.0
    holes[2, 5, 6] = 33.0
    regs = [(0,) + whole + (0, 255), (0,) + whole + (0, 77), (2, 0, 0, 4, 4, 0, -1), (2,) + whole + (0, -1),
            (2, 6, 5, 6, 5, 2, -1)]
    got = check_foot(holes, planes, regs, labels=lab, cell=16.0, grid=64, support=1)
    assert got["flags"].tolist() == [FR.VALID, FR.EMPTY, FR.EMPTY, FR.VALID, FR.VALID]
    assert got["n_masked"].tolist() == [4 * W, 0, 25, H * W, 1] and got["n"].tolist()[2:] == [0, 1, 1]
    got = check_foot(d, planes, [(0,) + whole + (0, -1)], cell=0.5, grid=16, support=1)
    assert got["flags"][0] & FR.CLIPPED and got["n_outside"][0] > 0 and got["span_s"][0] > 16
    # an offset that is not finite: no height is finite, no member
    got = check_foot(np.full((1, 6, 8), 5.0, np.float32), flat_plane(np.inf), [(0, 0, 0, 7, 5, 0, -1)], Qm=EYE,
                     cell=1.0, grid=16, support=1, h_range=(-np.inf, np.inf))
    assert got["flags"][0] == FR.EMPTY and got["n_valid"][0] == 48
    # K = 0
    r = sdr.Ruler(Q)
    dt = torch.from_numpy(d).to(dev())
    assert tuple(r.footprint_device(dt, planes, []).shape) == (0, 256) and r.footprint(d, planes, []).shape == (0,)
    # K = 9 overlapping queries with different planes, labels and frames
    nine = [(0, 0, 0, 29, 19, 0, -1), (1, 5, 5, 25, 15, 2, 0), (2, 29, 19, 0, 0, 0, 1), (0, 3, 3, 20, 18, 2, 2),
            (1, 0, 0, 29, 19, 0, 255), (2, 10, 0, 19, 19, 2, -1), (0, 0, 10, 29, 10, 0, 1), (1, 7, 7, 7, 7, 2, -1),
            (2, 0, 0, 29, 19, 1, -1)]
    got = check_foot(d, planes, nine, labels=lab, cell=6.0, grid=48, support=3)
    assert got["flags"][8] == FR.NO_PLANE and (got["flags"][:8] & (FR.VALID | FR.EMPTY)).all()


@pytest.mark.parametrize("grid,K", [(16, 3 * BATCH + 7), (512, 3 * 64 + 7)])
def test_more_queries_than_a_batch(grid, K):
    """The queries run in batches through one scratch block (256 of them, or as many as 64 MiB of
    grids hold: 64 at grid 512), so that later batches reuse the grids the first left behind."""
    rng = np.random.default_rng(9)
    F, H, W = 2, 12, 17
    d = ramp_scene(rng, F, H, W)
    lab = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (1, 0, 0, W - 1, H - 1)], Q, min_inliers=3)
    regs = np.stack([rng.integers(0, F, K), rng.integers(0, W, K), rng.integers(0, H, K), rng.integers(0, W, K),
                     rng.integers(0, H, K), rng.integers(-1, 3, K), rng.integers(-1, 4, K)], axis=1)
    regs[::50, 1] = W  # a refused query here and there
    got = check_foot(d, planes, regs, labels=lab, cell=4.0 if grid == 512 else 32.0, grid=grid, support=2)
    flags = set(got["flags"].tolist())
    assert {FR.VALID, FR.OUT_OF_RANGE, FR.NO_PLANE} <= flags
    assert (got["flags"][K - 70:] & FR.VALID).sum() > 10


# ---- inputs ----
def test_inputs_strides_and_confidence():
    rng = np.random.default_rng(11)
    F, H, W = 2, 41, 67
    d = ramp_scene(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    conf[rng.random((F, H, W)) < 0.05] = np.nan
    planes = PR.fit_planes(d, [(1, 0, 0, W - 1, H - 1)], Q)
    regs = [(1, 0, 0, W - 1, H - 1, 0, -1), (0, 5, 5, 60, 30, 0, -1)]
    kw = dict(cell=16.0, grid=64, support=2)
    for disp in (d, to_s16(d)):
        a = check_foot(disp, planes, regs, conf=conf, conf_min=80.0, **kw)
        assert (a["n_valid"] < a["n_masked"]).all() and (a["flags"] == FR.VALID).all()
        e = check_foot(disp, planes, regs, conf=conf, conf_min=float("nan"), **kw)  # nothing passes: EMPTY
        assert (e["flags"] == FR.EMPTY).all()
    # rows and frames padded
    pad = torch.full((F, H + 3, W + 9), -7.0, dtype=torch.float32, device=dev())
    pad[:, :H, :W] = torch.from_numpy(d).to(dev())
    view = pad[:, :H, :W]
    assert view.stride(1) == W + 9 and view.stride(0) == (H + 3) * (W + 9)
    r = sdr.Ruler(Q)
    FR.assert_footprints_equal(records(r.footprint_device(view, planes, regs, **kw)),
                               FR.footprint(d, planes, regs, Q, **kw))
    wide = np.full((F, H, W + 5), np.nan, np.float32)  # a strided host map
    wide[:, :, :W] = d
    FR.assert_footprints_equal(r.footprint(wide[:, :, :W], planes, regs, **kw), FR.footprint(d, planes, regs, Q, **kw))


def test_reference_calibration_with_found_planes():
    """The real pipeline: the reference calibration's Q (tests/golden/stereo.yaml), planes and labels
    found on the device, the footprint of every label in every found plane."""
    from stereo_depth_ruler_amd.config import StereoConfiguration

    cfg = StereoConfiguration()
    assert cfg.loadFromFile(os.path.join(ROOT, "tests", "golden", "stereo.yaml"))
    Qc = np.asarray(cfg.Q, np.float64).reshape(4, 4)
    disp, _, _ = SR.three_surface_scene(120, 160)
    r = sdr.Ruler(Qc)
    planes, lab = r.find_planes(torch.from_numpy(disp).to(dev()), None, hypotheses=128, min_inliers=300, labels=True)
    assert len(planes) == 3
    regs = [(0, 0, 0, 159, 119, p, l) for p in range(3) for l in (0, 1, 2, -1)]
    got = check_foot(disp, planes, regs, labels=lab, Qm=Qc, cell=16.0, grid=512, support=3)
    assert (got["flags"] & (FR.VALID | FR.EMPTY)).all() and (got["flags"][[0, 5, 10]] & FR.VALID).all()
    for p in range(3):  # a label's pixels are the plane's inliers, all of them valid
        assert got["n_valid"][4 * p + p] == got["n_masked"][4 * p + p] == planes["n_inliers"][p]


def test_box_scene_on_the_device():
    """The feature's scene (tests/test_footprint_cpu.py): search and footprint on the device."""
    Qw = FR.scene_q(Q)
    disp, truth, _ = FR.box_scene(Qw, 300.0, 200.0, 25.0)
    r = sdr.Ruler(Qw)
    planes, lab = r.find_planes(torch.from_numpy(disp).to(dev()), None, max_planes=3, hypotheses=256,
                                min_inliers=1000, seed=0, labels=True)
    assert len(planes) == 2
    box = int(np.argmax([((lab == i) & (truth == 1)).sum() for i in range(2)]))
    regs = [(0, 0, 0, 319, 239, 1 - box, box)]
    got = check_foot(disp, planes, regs, labels=lab, Qm=Qw)  # the defaults: cell 4, grid 512, support 4
    assert got["angle_deg"][0] == 25 and abs(max(got["side"][0]) - 300) < 22 and abs(min(got["side"][0]) - 200) < 22
    one = check_foot(disp, planes, regs, labels=lab, Qm=Qw, support=1)
    assert max(one["side"][0]) > 400


# ---- chaining and layers ----
def test_search_and_footprint_chain_on_one_stream():
    disp, _, _ = SR.three_surface_scene(60, 80)
    r = sdr.Ruler(Q)
    d = torch.from_numpy(disp).to(dev())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(hypotheses=128, min_inliers=200, max_planes=4)
    fk = dict(cell=16.0, grid=128, support=3)
    regs = [(0, 0, 0, 79, 59, 0, 1), (0, 0, 0, 79, 59, 0, 2), (0, 0, 0, 79, 59, 1, 0), (0, 10, 10, 70, 50, 3, -1)]
    out = r.find_planes_device(d, None, stream=side, labels=True, **kw)
    foot = r.footprint_device(d, out[0], regs, labels=out[3], stream=side, **fk)  # no synchronisation between
    side.synchronize()
    want = SR.find_planes(disp, (0, 0, 0, 79, 59), Q, **kw)
    assert want[1] == 3
    PR.assert_planes_equal(out[0].cpu().numpy().reshape(-1).view(PLANE_DTYPE), want[0])
    got = records(foot)
    FR.assert_footprints_equal(got, FR.footprint(disp, want[0], regs, Q, labels=want[3], **fk))
    assert (got["flags"][:3] & FR.VALID).all() and got["flags"][3] == FR.NO_PLANE  # the record past the count


def test_host_abi_and_tensor_forms():
    rng = np.random.default_rng(14)
    F, H, W = 2, 27, 45
    d = ramp_scene(rng, F, H, W)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    lab = rng.integers(0, 4, (F, H, W)).astype(np.uint8)
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (1, 0, 0, W - 1, H - 1)], Q, conf=conf, conf_min=30.0)
    regs = [(1, 2, 1, W - 1, H - 2, 1, 3), (0, 0, 0, W - 1, H - 1, 0, -1), (1, 0, 0, 9, 9, 0, 2)]
    kw = dict(cell=6.0, grid=40, support=2, h_range=(-50.0, 60.0))
    want = FR.footprint(d, planes, regs, Q, labels=lab, conf=conf, conf_min=30.0, **kw)
    r = sdr.Ruler(Q, conf_min=30.0)
    FR.assert_footprints_equal(r.footprint(d, planes, regs, labels=lab, conf=conf, **kw), want)       # host ABI
    FR.assert_footprints_equal(r.footprint(to_s16(d), planes, regs, labels=lab, conf=conf, **kw),
                               FR.footprint(to_s16(d), planes, regs, Q, labels=lab, conf=conf, conf_min=30.0, **kw))
    t = lambda a: torch.from_numpy(a).to(dev())  # noqa: E731
    FR.assert_footprints_equal(r.footprint(t(d), planes, regs, labels=t(lab), conf=t(conf), **kw), want)  # tensors
    pt = t(np.ascontiguousarray(planes).view(np.uint8).reshape(-1, 128))
    qt = t(as_relief_queries(regs))
    FR.assert_footprints_equal(records(r.footprint_device(t(d), pt, qt, labels=lab, conf=t(conf), **kw)), want)
    FR.assert_footprints_equal(r.footprint(d, pt, regs, labels=t(lab), conf=conf, **kw), want)  # device planes
    one = sdr.Ruler(Q).footprint(d[0], planes, (0, 0, 0, W - 1, H - 1))  # an (H, W) map, one tuple, the defaults
    FR.assert_footprints_equal(one, FR.footprint(d[:1], planes, [(0, 0, 0, W - 1, H - 1)], Q))
    length, width = sdr.footprint_length_width(one)
    assert length[0] == max(one["side"][0]) and width[0] == min(one["side"][0])


def test_live_loop_footprint_on_the_frame_stream():
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
    loop = LiveLoop(rect, Q, 1, ruler=dict(radius=1, min_count=2, conf_min=100.0))
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(max_planes=3, hypotheses=96, iterations=2, inlier_px=2.0, min_inliers=30)
    fk = dict(cell=32.0, grid=256, support=2)
    w2, h2 = loop.w2, loop.h2
    regs = [(0, 0, 0, w2 - 1, h2 - 1, 0, 0), (0, 0, 0, w2 - 1, h2 - 1, 0, -1), (0, 150, 30, 60, 10, 1, 255)]
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        planes, count, _, lab = loop.find_planes(None, side, labels=True, **kw)
        foot = loop.footprint(planes, regs, side, labels=lab, **fk)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    pl = planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    got = records(foot)
    FR.assert_footprints_equal(got, FR.footprint(disp, pl, regs, Q, labels=lab.cpu().numpy(), conf=conf,
                                                 min_disp=loop.ruler.min_disp, conf_min=100.0, **fk))
    assert int(count.cpu()[0]) >= 1 and got["flags"][0] & FR.VALID and got["n_valid"][0] == pl["n_inliers"][0]
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()


def test_cpp_facade_footprint(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::footprint gives Python's records as bytes
    (tests/cpp/facade_footprint.cpp)."""
    exe = tmp_path / "facade_footprint"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_footprint.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    disp, _, _ = SR.three_surface_scene(45, 61)
    rng = np.random.default_rng(15)
    H, W = disp.shape[1:]
    conf = rng.uniform(0, 255, (1, H, W)).astype(np.float32)
    disp[0].tofile(tmp_path / "disp.bin")
    conf[0].tofile(tmp_path / "conf.bin")
    np.asarray(Q, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), "4", "90", "12345", str(tmp_path)], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    r = sdr.Ruler(Q, conf_min=10.0)
    planes, lab = r.find_planes(disp, None, conf=conf, max_planes=4, hypotheses=90, seed=12345, iterations=2,
                                inlier_px=1.5, min_inliers=6, labels=True)
    n = len(planes)
    assert n >= 2 and f"planes={n} footprints={2 * n}" in res.stdout
    assert "single_equal=1" in res.stdout and "bad_grid_code=-1" in res.stdout
    assert (tmp_path / "planes.bin").read_bytes() == planes.tobytes()
    assert (tmp_path / "labels.bin").read_bytes() == lab.tobytes()
    regs = [q for i in range(n) for q in ((0, W - 1, 0, 0, H - 1, 0, i), (0, 0, 0, W - 1, H - 1, i, -1))]
    want = FR.footprint(disp, planes, regs, Q, labels=lab, conf=conf, conf_min=10.0, cell=8.0, grid=128, support=3,
                        h_range=(-500.0, 500.0))
    assert (tmp_path / "footprint.bin").read_bytes() == want.tobytes()
    assert (r.footprint(disp, planes, regs, labels=lab, conf=conf, cell=8.0, grid=128, support=3,
                        h_range=(-500.0, 500.0)).tobytes() == want.tobytes())


# ---- hypothesis ----
@settings(max_examples=hyp_examples(20), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(3, 96), W=st.integers(3, 96), with_conf=st.booleans(), with_labels=st.booleans(),
       i16=st.booleans(), cell=st.sampled_from([0.5, 1.0, 3.7, 16.0]), grid=st.integers(16, 64),
       support=st.integers(1, 9), seed=st.integers(0, 2 ** 32 - 1))
def test_hypothesis_random_scenes(H, W, with_conf, with_labels, i16, cell, grid, support, seed):
    rng = np.random.default_rng(seed)
    F = int(rng.integers(1, 3))
    d = ramp_scene(rng, F, H, W)
    weird = rng.random((F, H, W)) < 0.03
    d[weird] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2048.0], np.float32), int(weird.sum()))
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (F - 1, 0, 0, W // 2, H // 2)], Q, min_inliers=3)
    disp = to_s16(d) if i16 else d
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32) if with_conf else None
    lab = rng.choice(np.array([0, 1, 2, 255], np.uint8), (F, H, W)) if with_labels else None
    regs = []
    for _ in range(int(rng.integers(1, 5))):
        reg = [int(rng.integers(0, F)), int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, W)),
               int(rng.integers(0, H)), int(rng.integers(0, 2)), int(rng.choice([-1, -1, 0, 1, 255]))]
        if rng.random() < 0.4:
            reg[1:5] = [0, 0, W - 1, H - 1]
        if rng.random() < 0.15:
            reg[int(rng.integers(0, 6))] = int(rng.choice([-1, 100]))
        regs.append(tuple(reg))
    h_range = None if rng.random() < 0.5 else (float(rng.uniform(-40, 0)), float(rng.uniform(0, 40)))
    check_foot(disp, planes, regs, labels=lab, conf=conf, conf_min=float(rng.uniform(0, 200)), cell=cell, grid=grid,
               support=support, h_range=h_range)
