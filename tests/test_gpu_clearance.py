"""GPU: the clearance of two labelled things (sdr_clearance*, csrc/sdr_clearance.hip) through every
layer: every record compared bit for bit with the numpy restatement (tests/clearance_ref.py)."""
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

import clearance_ref as CR  # noqa: E402
import footprint_ref as FR  # noqa: E402
import objects_ref as OR  # noqa: E402
import plane_ref as PR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import DEBUG_CLEARANCE_PRUNE, check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import (CLEARANCE_DTYPE, OBJECT_DTYPE, OBJECT_SCAN_DTYPE, PLANE_DTYPE,  # noqa: E402
                                          as_clearance_queries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q
EYE = np.eye(4)
B = 256  # csrc/sdr_clearance.hip, kClrBlock
G = 16  # csrc/sdr_clearance.hip, kClrGroups: the workgroups a block of A, each with every 16th block of B
SLICE = 2048  # csrc/sdr_region.hpp, kRegionSlice
X0, Y0 = 3, 5  # a planted rectangle's origin in its map
A, Bl, NONE = 0, 1, 255  # the planted labels


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """With Q the identity and this record, a pixel's point is (x, y, d) and hf is d."""
    p = np.zeros(1, PLANE_DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def host(rec):
    torch.cuda.synchronize()
    return rec.cpu().numpy().reshape(-1).view(CLEARANCE_DTYPE)


def check_clearance(disp, planes, pairs, labels, conf=None, Qm=Q, radius=0, min_count=1, min_disp=-1.0, conf_min=0.0,
                    h_range=None):
    """Device records == the restatement's, on every bit.  disp: a numpy map (a view with a row
    stride is passed on as one)."""
    r = sdr.Ruler(Qm, radius=radius, min_count=min_count, min_disp=min_disp, conf_min=conf_min)
    base = disp.base if disp.base is not None and disp.base.ndim == disp.ndim else None
    if base is not None:  # keep the stride: the same slice of the tensor
        d = torch.from_numpy(np.ascontiguousarray(base)).to(dev())[..., :disp.shape[-1]]
        assert d.stride(-2) > d.shape[-1]
    else:
        d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev())
    got = host(r.clearance_device(d, planes, pairs, lab, conf=c, h_range=h_range))
    want = CR.clearance(disp, planes, pairs, Qm, labels, conf=conf, radius=radius, min_count=min_count,
                        h_range=h_range, min_disp=min_disp, conf_min=conf_min)
    CR.assert_clearances_equal(got, want)
    return got


def embed(rect, lab, fill=20.0, lab_fill=A, dtype=np.float32, pad=7):
    """The (rh, rw) map `rect` with its labels at (X0, Y0) of frame 1 of a (2, rh + 9, rw + 8) map
    whose rows are rw + 8 + pad apart; the rest holds `fill` with the label `lab_fill`: pixels of a
    set just outside the rectangle, which would change a median if the window were clipped to the
    image.  Returns (the strided disparity view, the dense labels, the rectangle's corners)."""
    rh, rw = rect.shape
    full = np.full((2, rh + 9, rw + 8 + pad), fill, dtype)
    view = full[:, :, :rw + 8]
    view[1, Y0:Y0 + rh, X0:X0 + rw] = rect
    labels = np.full((2, rh + 9, rw + 8), lab_fill, np.uint8)
    labels[1, Y0:Y0 + rh, X0:X0 + rw] = lab
    return view, labels, (1, X0, Y0, X0 + rw - 1, Y0 + rh - 1)


PLANTED = dict(Qm=EYE, min_disp=-3e38)


def planted(rect, lab, la=A, lb=Bl, plane=None, **kw):
    """One query over a planted rectangle; returns its record."""
    view, labels, reg = embed(np.asarray(rect, np.float32), np.asarray(lab, np.uint8))
    return check_clearance(view, flat_plane() if plane is None else plane, [reg + (0, la, lb)], labels,
                           **dict(PLANTED, **kw))[0]


def scatter(rng, H, W, na, nb, levels=6):
    """na pixels of A and nb of B at random places of an (H, W) rectangle, integer disparities."""
    lab = np.full(H * W, NONE, np.uint8)
    where = rng.permutation(H * W)[:na + nb]
    lab[where[:na]] = A
    lab[where[na:]] = Bl
    d = rng.integers(10, 10 + levels, (H, W)).astype(np.float32)
    return d, lab.reshape(H, W)


# ---- sizes ----
@pytest.mark.parametrize("na,nb", [(1, 1), (B - 1, B + 1), (B, B), (B + 1, B - 1), (2 * B + 1, 1), (1, 2 * B + 1),
                                   (2 * B + 1, 2 * B + 1)])
def test_set_sizes_around_the_block(na, nb):
    rng = np.random.default_rng(na * 1000 + nb)
    d, lab = scatter(rng, 36, 40, na, nb)
    r = planted(d, lab)
    assert r["flags"] == CR.VALID and (r["n_a"], r["n_b"], r["m_a"], r["m_b"]) == (na, nb, na, nb)
    r = planted(d, lab, radius=1, min_count=1)
    assert (r["m_a"], r["m_b"]) == (na, nb)


@pytest.mark.parametrize("H,W", [(23, 89), (32, 64), (3, 683), (1, 1), (1, 70), (70, 1)])
def test_rectangles_around_the_slice(H, W):
    assert H * W in (SLICE - 1, SLICE, SLICE + 1, 1, 70)
    rng = np.random.default_rng(H * 1000 + W)
    d = rng.integers(10, 14, (H, W)).astype(np.float32)
    lab = rng.choice(np.array([A, Bl, NONE], np.uint8), (H, W))
    for radius, mc in ((0, 1), (2, 3)):
        r = planted(d, lab, radius=radius, min_count=mc)
        assert r["area"] == H * W and r["n_a"] == int((lab == A).sum()) and r["n_b"] == int((lab == Bl).sum())
    # the last pixel of the rectangle alone against the first
    lab[:] = NONE
    lab[0, 0], lab[-1, -1] = A, Bl
    r = planted(d, lab)
    if H * W > 1:
        assert r["flags"] == CR.VALID and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0, Y0, X0 + W - 1, Y0 + H - 1)
    else:
        assert r["flags"] == CR.EMPTY and (r["n_a"], r["n_b"]) == (0, 1)


def test_window_is_clipped_to_the_rectangle():
    """Outside the rectangle lie pixels of A with another disparity: a window clipped to the image
    would take them into the medians of A's border pixels."""
    H, W = 12, 20
    d = np.full((H, W), 30.0, np.float32)
    lab = np.full((H, W), A, np.uint8)
    lab[:, 12:] = Bl
    for radius in (1, 2, 4):
        r = planted(d, lab, radius=radius, min_count=1)
        assert r["d_a"] == 30.0 and r["d_b"] == 30.0 and r["distance"] == 1.0  # the fill is 20
        # the corner pixel's window holds (radius + 1)^2 pixels of the rectangle
        r = planted(d, lab, radius=radius, min_count=(radius + 1) ** 2 + 1)
        assert r["m_a"] < r["n_a"]


# ---- ties ----
def test_ties_go_to_the_lower_indices():
    H, W = 80, 64  # 2.5 slices
    d = np.full((H, W), 20.0, np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    lab[:, :10] = A    # 800 points: four blocks
    lab[:, 20:30] = Bl
    r = planted(d, lab)  # every row holds a pair of s = 121: the block pairs' bounds equal the minimum
    assert r["distance"] == 11.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 9, Y0, X0 + 20, Y0)
    # one point of A, a ring of B at s = 25 and many far points of B: the lowest index of B wins
    lab[:] = NONE
    lab[40, 30] = A
    for dy, dx in ((-5, 0), (-4, -3), (-4, 3), (-3, -4), (-3, 4), (0, -5), (0, 5), (3, -4), (3, 4), (4, -3), (4, 3), (5, 0)):
        lab[40 + dy, 30 + dx] = Bl
    lab[:20, :] = Bl
    lab[60:, :] = Bl
    r = planted(d, lab)
    assert r["distance"] == 5.0 and (r["xb"], r["yb"]) == (X0 + 30, Y0 + 35)
    lab[35, 30] = NONE
    r = planted(d, lab)
    assert r["distance"] == 5.0 and (r["xb"], r["yb"]) == (X0 + 27, Y0 + 36)
    # three pairs of s = 25 in different slices, one of them through the depth: the lowest ip wins
    lab[:] = NONE
    lab[10, 10], lab[10, 15] = A, Bl          # dx = 5
    lab[40, 5], lab[40, 8] = A, Bl            # dx = 3, dz = 4
    d[40, 8] = 24.0
    lab[70, 50], lab[73, 54] = A, Bl          # dx = 4, dy = 3
    r = planted(d, lab)
    assert r["distance"] == 5.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 10, Y0 + 10, X0 + 15, Y0 + 10)
    lab[10, 10] = NONE
    r = planted(d, lab)
    assert r["distance"] == 5.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 5, Y0 + 40, X0 + 8, Y0 + 40)
    assert r["along"] == 4.0 and r["across"] == 3.0


def test_a_block_bound_equal_to_the_minimum_is_not_pruned():
    """A's blocks find s = 100 against B's near cluster at once; the winner's tie partner with the
    lower index lies in a block of B whose bound equals 100: a prune on >= would drop it."""
    H, W = 96, 96
    d = np.full((H, W), 20.0, np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    lab[40:56, 20:36] = A            # 256 points, x <= 35
    lab[40:56, 45:61] = Bl           # x >= 45: gap 10 on the x axis, s = 100 on every row, a bound of 100
    lab[0:16, 45:61] = Bl            # far above: bounds beyond 100
    lab[80:96, 45:61] = Bl           # far below
    r = planted(d, lab)
    assert r["distance"] == 10.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 35, Y0 + 40, X0 + 45, Y0 + 40)
    # the same with the sets exchanged, and a plane whose normal lies along the gap
    r = planted(d, lab, la=Bl, lb=A, plane=flat_plane(0.0, (1.0, 0.0, 0.0)), h_range=(-1e5, 1e5))
    assert r["distance"] == 10.0 and r["along"] == -10.0 and r["across"] == 0.0
    assert (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 45, Y0 + 40, X0 + 35, Y0 + 40)


# ---- pruning ----
def test_distant_clusters_and_a_late_answer():
    H, W = 100, 100
    rng = np.random.default_rng(8)
    d = rng.integers(20, 23, (H, W)).astype(np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    lab[2:30, 2:30] = A       # far from everything of B
    lab[2:30, 70:98] = Bl
    lab[70:98, 2:30] = Bl
    lab[72:96, 60:84] = A     # the last rows: the closest pair lies here
    lab[75:93, 88:99] = Bl
    r = planted(d, lab)
    assert r["flags"] == CR.VALID and r["ya"] >= Y0 + 72 and r["xb"] >= X0 + 88 and r["distance"] < 8.0
    r = planted(d, lab, radius=2, min_count=5)
    assert r["ya"] >= Y0 + 72 and r["xb"] >= X0 + 88


# ---- more than one block of B a workgroup: B holds more than G * B points, so that a workgroup streams
# several blocks through LDS, chooses its nearest among them and decides the prune for the rest ----
@pytest.mark.parametrize("na,nb", [(300, G * B - 1), (300, G * B), (300, G * B + 1), (300, 2 * G * B + 1),
                                   (G * B + 1, G * B + 1), (2 * G * B + 1, 300)])
def test_set_sizes_around_the_groups(na, nb):
    rng = np.random.default_rng(na * 7 + nb)
    d, lab = scatter(rng, 100, 100, na, nb, levels=12)
    r = planted(d, lab)
    assert r["flags"] == CR.VALID and (r["m_a"], r["m_b"]) == (na, nb)


def test_ties_across_many_blocks_of_b():
    """Every row holds a pair of s = 121 and B has 55 blocks: every block of B in the rows of a block
    of A has a bound equal to the minimum, and the lowest ip, then the lowest iq win."""
    H, W = 140, 128
    d = np.full((H, W), 20.0, np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    lab[:, :10] = A
    lab[:, 20:120] = Bl  # 14000 points
    r = planted(d, lab)
    assert r["m_b"] == 14000 > 3 * G * B
    assert r["distance"] == 11.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 9, Y0, X0 + 20, Y0)
    r = planted(d, lab, la=Bl, lb=A)
    assert r["distance"] == 11.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 20, Y0, X0 + 9, Y0)


def test_a_late_block_whose_bound_equals_the_minimum_holds_the_winner():
    """Q gives every pixel Y = 0, so a point is (x, 0, d) and the image row only decides where a pixel
    comes in the lists.  A is two pixels at X = 7: the first at Z = 20, the second at Z = 1020.  B is
    16742 points (66 blocks, four or five a workgroup) at X >= 20: its first pixel (X = 20, Z = 1020)
    pairs with A's SECOND pixel at s = 169 and lies in one of B's first sixteen blocks, each of which
    is its workgroup's first, so 169 is found at once; rows of decoys (Z alternating 10 and 30: a
    bound of 169 against A's block, no pair below 269) keep every workgroup busy; B's LAST pixel
    (X = 20, Z = 20) pairs with A's FIRST pixel at s = 169 too.  That pair has the lower ip and must
    win, and it lies in a block its workgroup reaches fourth or fifth, with a bound of exactly 169:
    a prune on >= skips it once 169 has been found.  The lists' order is the order the sample
    sweep's workgroups finish in, so the first slice holds the fewest members and the last the
    most; the record is the same in any order, and the case bites in that one."""
    H, W = 208, 128  # 13 slices of 16 rows
    d = np.full((H, W), 20.0, np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    decoy = np.where(np.arange(W) % 2 == 0, 10.0, 30.0).astype(np.float32)[None, :]
    lab[0, 7], lab[1, 7] = A, A
    d[1, 7] = 1020.0
    lab[2, 20] = Bl
    d[2, 20] = 1020.0
    lab[3:192, 20:100] = Bl     # 80 a row: 1040 in the first slice, 1280 in the next eleven
    lab[192:207, 20:128] = Bl   # 108 a row: 1620 in the last slice
    d[3:207] = np.where(lab[3:207] == Bl, decoy, d[3:207])
    lab[207, 20] = Bl           # Z = 20
    Qm = np.eye(4)
    Qm[1, 1] = 0.0
    r = planted(d, lab, Qm=Qm)
    assert r["m_b"] == 16742 and r["distance"] == 13.0
    assert (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 7, Y0, X0 + 20, Y0 + 207)
    # exchanged: the lower ip is now B's first pixel
    r = planted(d, lab, la=Bl, lb=A, Qm=Qm)
    assert r["distance"] == 13.0 and (r["xa"], r["ya"], r["xb"], r["yb"]) == (X0 + 20, Y0 + 2, X0 + 7, Y0 + 1)


def clusters():
    """Two distant dense clusters a set in 180 x 180, B 14050 points (55 blocks); the closest pair lies
    between the clusters that come last in the lists."""
    H, W = 180, 180
    rng = np.random.default_rng(8)
    d = rng.integers(20, 23, (H, W)).astype(np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    lab[5:45, 5:45] = A          # far from everything of B
    lab[0:90, 120:180] = Bl
    lab[95:180, 0:70] = Bl
    lab[130:170, 80:120] = A     # the last rows: the closest pair lies here
    lab[125:175, 126:180] = Bl
    return d, lab


def test_distant_clusters_and_a_late_answer_over_many_blocks():
    d, lab = clusters()
    r = planted(d, lab)
    assert r["m_b"] == 14050 and r["flags"] == CR.VALID
    assert r["ya"] >= Y0 + 130 and r["xa"] == X0 + 119 and r["xb"] == X0 + 126 and r["distance"] < 8.0
    r = planted(d, lab, radius=2, min_count=5)
    assert r["ya"] >= Y0 + 130 and r["xb"] >= X0 + 126


# ---- inputs ----
def test_int16_confidence_min_disp_band_and_min_count():
    rng = np.random.default_rng(12)
    F, H, W = 2, 45, 75
    d16 = rng.integers(16 * 10, 16 * 14, (F, H, W)).astype(np.int16)
    d16[rng.random((F, H, W)) < 0.1] = -16
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    conf[rng.random((F, H, W)) < 0.1] = np.nan
    lab = rng.choice(np.array([0, 7, 255], np.uint8), (F, H, W))
    pairs = [(1, 2, 1, W - 3, H - 2, 0, 0, 7), (0, W - 1, H - 1, 0, 0, 0, 7, 255), (1, 10, 10, 30, 30, 0, 255, 0)]
    for radius, mc in ((0, 1), (1, 3), (4, 20)):
        got = check_clearance(d16, flat_plane(), pairs, lab, conf=conf, Qm=EYE, conf_min=60.0, radius=radius,
                              min_count=mc)
        assert (got["m_a"] <= got["n_a"]).all() and (mc > 3 or (got["flags"] == CR.VALID).all())
    # min_disp is strict; a band takes B away entirely: EMPTY with m_b == 0 and the counts as found
    d = (d16.astype(np.float32) * np.float32(0.0625))
    got = check_clearance(d, flat_plane(), pairs[:1], lab, Qm=EYE, min_disp=12.0)
    assert got["flags"][0] == CR.VALID and got["d_a"][0] > 12.0
    d[1][lab[1] == 7] = 50.0
    got = check_clearance(d, flat_plane(), pairs[:1], lab, Qm=EYE, h_range=(0.0, 40.0))[0]
    assert got["flags"] == CR.EMPTY and got["n_b"] == 0 and got["m_b"] == 0 and got["n_a"] > 0 and got["xa"] == -1
    got = check_clearance(d, flat_plane(), pairs[:1], lab, Qm=EYE, h_range=(40.0, 60.0))[0]
    assert got["flags"] == CR.EMPTY and got["n_a"] == 0 and got["n_b"] > 0
    # min_count above a set's size
    small = np.full((20, 30), NONE, np.uint8)
    small[5, 5:9] = A
    small[10:16, 12:20] = Bl
    r = planted(np.full((20, 30), 20.0, np.float32), small, radius=2, min_count=5)
    assert r["flags"] == CR.EMPTY and (r["n_a"], r["m_a"]) == (4, 0) and r["m_b"] > 0
    r = planted(np.full((20, 30), 20.0, np.float32), small, radius=2, min_count=4)
    assert r["flags"] == CR.VALID and r["m_a"] == 2  # the two middle pixels see all four


def test_infinite_s_and_nan_parts():
    """A scale of Q that takes every difference of X past the floats: s = +inf for every pair, the
    lowest indices win, along = 0 * inf is the canonical NaN and across 0."""
    H, W = 24, 40
    d = np.full((H, W), 20.0, np.float32)
    lab = np.full((H, W), NONE, np.uint8)
    lab[:, :6] = A
    lab[:, W - 6:] = Bl
    view, labels, reg = embed(d, lab, lab_fill=NONE)
    cx = X0 + (W - 1) / 2.0
    Qm = np.eye(4)
    Qm[0, 0], Qm[0, 3] = 1.5e37, -1.5e37 * cx  # X = 1.5e37 * (x - cx): finite, the sets' difference is not
    got = check_clearance(view, flat_plane(), [reg + (0, A, Bl)], labels, Qm=Qm, min_disp=-3e38)[0]
    assert got["flags"] == CR.VALID and np.isinf(got["distance"]) and got["across"] == 0.0
    assert np.float64(got["along"]).view(np.uint64) == 0x7ff8000000000000
    assert (got["xa"], got["ya"], got["xb"], got["yb"]) == (X0, Y0, X0 + W - 6, Y0)


# ---- refusals ----
def test_refusal_records_and_query_counts():
    rng = np.random.default_rng(3)
    F, H, W = 2, 12, 40
    d = rng.integers(10, 14, (F, H, W)).astype(np.float32)
    lab = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    pl = np.concatenate([flat_plane(), flat_plane(flags=PR.DEGENERATE)])
    rows = [(2, 0, 0, 7, 5, 0, 0, 1), (-1, 0, 0, 7, 5, 0, 0, 1), (0, 0, 0, 40, 5, 0, 0, 1), (0, 0, -1, 7, 5, 0, 0, 1),
            (0, 0, 0, 7, 12, 0, 0, 1), (0, 0, 0, 7, 5, 0, -1, 1), (0, 0, 0, 7, 5, 0, 0, 256), (0, 0, 0, 7, 5, 0, 2, 2),
            (0, 0, 0, 7, 5, -1, 0, 1), (0, 0, 0, 7, 5, 2, 0, 1), (1, 7, 5, 0, 0, 1, 0, 1)]
    got = check_clearance(d, pl, rows, lab, Qm=EYE)
    assert got["flags"].tolist() == [CR.OUT_OF_RANGE] * 8 + [CR.NO_PLANE] * 3
    assert (got["area"][:8] == 0).all() and (got["area"][8:] == 48).all() and (got["xa"] == -1).all()
    # no plane record at all
    got = check_clearance(d, np.zeros(0, PLANE_DTYPE), [(0, 0, 0, 7, 5, 0, 0, 1)], lab, Qm=EYE)
    assert got["flags"][0] == CR.NO_PLANE and got["area"][0] == 48
    # several queries in one call: refused ones among valid ones, one rectangle shared by three pairs
    # of labels, corners in any order, another rectangle and the other frame
    rows = [(0, 0, 0, W - 1, H - 1, 0, 0, 1), rows[0], (0, W - 1, H - 1, 0, 0, 0, 1, 2), (0, 0, H - 1, W - 1, 0, 0, 2, 0),
            rows[8], (1, 5, 2, 30, 9, 0, 0, 1), (1, 30, 9, 5, 2, 0, 1, 0)]
    got = check_clearance(d, pl, rows, lab, Qm=EYE, radius=1, min_count=2)
    assert got["flags"].tolist() == [1, 2, 1, 1, 4, 1, 1]
    assert got["distance"][5] == got["distance"][6] and got["xa"][5] == got["xb"][6]
    # K = 0, K at the cap and above it
    r = sdr.Ruler(EYE)
    dt, lt = torch.from_numpy(d).to(dev()), torch.from_numpy(lab).to(dev())
    assert r.clearance_device(dt, pl, [], lt).shape == (0, 128) and r.clearance(d, pl, [], lab).shape == (0,)
    many = [(k % 2, 0, 0, 8 + k % 30, 3 + k % 8, 0, k % 3, (k + 1) % 3) for k in range(CR.MAX_QUERIES)]
    check_clearance(d, pl, many, lab, Qm=EYE)
    for call in (lambda: r.clearance_device(dt, pl, many + many[:1], lt), lambda: r.clearance(d, pl, many + many[:1], lab)):
        with pytest.raises(sdr.SDRError) as e:
            call()
        assert e.value.code == -1


# ---- hypothesis ----
@settings(max_examples=hyp_examples(25), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(1, 40), W=st.integers(1, 48), density=st.floats(0.3, 1.0), levels=st.integers(1, 6),
       radius=st.integers(0, 4), min_count=st.sampled_from([1, 2, 5, 12]), i16=st.booleans(), real_q=st.booleans(),
       seed=st.integers(0, 2 ** 32 - 1))
def test_hypothesis_random_maps(H, W, density, levels, radius, min_count, i16, real_q, seed):
    rng = np.random.default_rng(seed)
    d = (20.0 + 0.75 * rng.integers(0, levels, (H, W))).astype(np.float32)
    d[rng.random((H, W)) >= density] = -1.0
    lab = rng.choice(np.array([A, Bl, NONE], np.uint8), (H, W), p=[0.45, 0.45, 0.1])
    dt = np.int16 if i16 else np.float32
    view, labels, reg = embed((d * 16).astype(np.int16) if i16 else d, lab, fill=320 if i16 else 20.0, dtype=dt)
    plane = flat_plane(900.0, (0.0, -0.6, -0.8)) if real_q else flat_plane()
    check_clearance(view, plane, [reg + (0, A, Bl), reg + (0, Bl, A)], labels, Qm=Q if real_q else EYE, radius=radius,
                    min_count=min_count, h_range=(-1e5, 1e5))


# ---- the entries ----
def test_host_abi_forms():
    rng = np.random.default_rng(14)
    F, H, W = 2, 40, 70
    d = (20.0 + 0.75 * rng.integers(0, 3, (F, H, W))).astype(np.float32)
    d[rng.random((F, H, W)) < 0.3] = -1.0
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    lab = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    pl = flat_plane(900.0, (0.0, -0.6, -0.8))
    pairs = [(1, 2, 1, W - 2, H - 3, 0, 1, 2), (0, 0, 0, W - 1, H - 1, 0, 0, 1)]
    r = sdr.Ruler(Q, radius=1, min_count=3, conf_min=30.0)
    kw = dict(radius=1, min_count=3, conf_min=30.0, h_range=(-5000.0, 5000.0))
    for disp in (d, (d * 16).astype(np.int16)):
        want = CR.clearance(disp, pl, pairs, Q, lab, conf=conf, **kw)
        assert (want["flags"] == CR.VALID).all()
        got = r.clearance(disp, pl, pairs, lab, conf=conf, h_range=kw["h_range"])  # host pointers
        CR.assert_clearances_equal(got, want)
        t = lambda a: torch.from_numpy(a).to(dev())  # noqa: E731
        got = r.clearance(t(disp), pl, pairs, t(lab), conf=t(conf), h_range=kw["h_range"])  # tensors
        CR.assert_clearances_equal(got, want)
        pt = t(np.ascontiguousarray(pl).view(np.uint8).reshape(-1, 128))
        got = host(r.clearance_device(t(disp), pt, t(as_clearance_queries(pairs)), lab, conf=t(conf),
                                      h_range=kw["h_range"]))
        CR.assert_clearances_equal(got, want)
    # an (H, W) map with an (H, W) label map, one row
    one = sdr.Ruler(Q).clearance(d[0], pl, (0, 0, 0, W - 1, H - 1, 0, 0, 1), lab[0])
    CR.assert_clearances_equal(one, CR.clearance(d[:1], pl, [(0, 0, 0, W - 1, H - 1, 0, 0, 1)], Q, lab[:1]))


def scene():
    Qw = FR.scene_q(Q)
    d, truth, info = OR.two_object_scene(Qw)
    return Qw, d, truth


def test_chain_on_a_side_stream():
    """find_planes_device -> find_objects_device -> clearance_device on a stream that is not the
    default one, planes and labels as tensors, no synchronise in between."""
    Qw, d, truth = scene()
    H, W = truth.shape
    r = sdr.Ruler(Qw, radius=2, min_count=9)
    dt = torch.from_numpy(d).to(dev())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(h_range=(10.0, 1000.0), min_pixels=64, max_objects=4)
    whole = (0, 0, 0, W - 1, H - 1, 0, 255)
    pairs = [(0, 0, 0, W - 1, H - 1, 0, 0, 1), (0, 0, 0, W - 1, H - 1, 0, 1, 0), (0, 0, 0, W - 1, H - 1, 0, 0, 3)]
    with torch.cuda.stream(side):
        planes, count, _, plab = r.find_planes_device(dt, None, max_planes=1, hypotheses=256, min_inliers=1000, seed=0,
                                                      labels=True, stream=side)
        rec, scan_t, lab_t = r.find_objects_device(dt, planes, whole, labels=plab, stream=side, labels_out=True, **kw)
        clr = r.clearance_device(dt, planes, pairs, lab_t, stream=side)
    side.synchronize()
    pl = planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    lab = lab_t.cpu().numpy()
    scan = scan_t.cpu().numpy().view(OBJECT_SCAN_DTYPE)[0]
    objs = rec.cpu().numpy().reshape(-1).view(OBJECT_DTYPE)
    got = clr.cpu().numpy().reshape(-1).view(CLEARANCE_DTYPE)
    CR.assert_clearances_equal(got, CR.clearance(d, pl, pairs, Qw, lab, radius=2, min_count=9))
    assert scan["count"] == 2 and got["flags"].tolist() == [CR.VALID, CR.VALID, CR.EMPTY]
    assert got["n_a"][0] == objs["n"][0] and got["n_b"][0] == objs["n"][1]
    assert got["distance"][0] == got["distance"][1] and got["along"][0] == -got["along"][1]
    assert 110.0 < got["distance"][0] < 135.0  # the CPU scene test's truth is 122.16 mm
    ends = {int(truth[got["ya"][0], got["xa"][0]]), int(truth[got["yb"][0], got["xb"][0]])}
    assert ends == {1, 2}
    # the host-pointer entry on the copied maps: the same records
    CR.assert_clearances_equal(r.clearance(d, pl, pairs, lab), got)


def test_live_loop_clearance_on_the_frame_stream():
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
    w2, h2 = loop.w2, loop.h2
    pairs = [(0, 0, 0, w2 - 1, h2 - 1, 0, 0, 255), (0, 0, 0, w2 - 1, h2 - 1, 0, 255, 0), (0, 0, 0, w2 - 1, h2 - 1, 0, 0, 1)]
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        planes, count, _, plab = loop.find_planes(None, side, labels=True, **kw)
        clr = loop.clearance(planes, pairs, side, plab)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    pl = planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    got = clr.cpu().numpy().reshape(-1).view(CLEARANCE_DTYPE)
    want = CR.clearance(disp, pl, pairs, Q, plab.cpu().numpy(), conf=conf, radius=1, min_count=2,
                        min_disp=loop.ruler.min_disp, conf_min=100.0)
    CR.assert_clearances_equal(got, want)
    assert int(count.cpu()[0]) >= 1 and got["flags"][0] in (CR.VALID, CR.EMPTY) and got["n_a"][0] > 0
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()


def test_prune_switch_changes_no_record():
    """sdr_clearance_debug_knob(SDR_DEBUG_CLEARANCE_PRUNE, 0) runs every block pair (the measurement
    switch of scripts/clearance_bench.py): the same bytes, on sets whose workgroups hold several
    blocks of B each, so that the pruned run does skip some."""
    d, lab = clusters()
    want = planted(d, lab, radius=1, min_count=2)
    view, labels, reg = embed(d, lab)
    r = sdr.Ruler(EYE, radius=1, min_count=2, min_disp=-3e38)
    dt = torch.from_numpy(np.ascontiguousarray(view)).to(dev())
    lt = torch.from_numpy(labels).to(dev())
    assert lib().sdr_clearance_debug_knob(DEBUG_CLEARANCE_PRUNE, 0) == 0
    try:
        got = host(r.clearance_device(dt, flat_plane(), [reg + (0, A, Bl)], lt))[0]
    finally:
        assert lib().sdr_clearance_debug_knob(DEBUG_CLEARANCE_PRUNE, 1) == 0
    assert got.tobytes() == want.tobytes()
    assert lib().sdr_clearance_debug_knob(2, 0) == -1 and lib().sdr_clearance_debug_knob(0, 1) == -1


def test_cpp_facade_clearance(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::clearance gives Python's records as bytes
    (tests/cpp/facade_clearance.cpp)."""
    exe = tmp_path / "facade_clearance"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_clearance.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    Qw, d, truth = scene()
    H, W = truth.shape
    d[0].tofile(tmp_path / "disp.bin")
    np.asarray(Qw, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    r = sdr.Ruler(Qw, radius=2, min_count=9)
    planes, plab = r.find_planes(d, None, max_planes=1, hypotheses=256, seed=0, min_inliers=1000, labels=True)
    whole = (0, 0, 0, W - 1, H - 1, 0, 255)
    objs, scan, lab = r.find_objects(d, planes, whole, labels=plab, h_range=(10.0, 1000.0), min_pixels=64, max_objects=4)
    pairs = [(0, 0, 0, W - 1, H - 1, 0, 0, 1), (0, 0, 0, W - 1, H - 1, 0, 1, 0)]
    got = r.clearance(d, planes, pairs, lab)
    CR.assert_clearances_equal(got, CR.clearance(d, planes, pairs, Qw, lab, radius=2, min_count=9))
    assert f"objects={len(objs)} valid=1" in res.stdout and len(objs) == 2
    assert "single_equal=1" in res.stdout and "same_label_flags=2" in res.stdout
    assert "bad_labels_code=-5" in res.stdout  # a map that is no CV_8U label map: the facade's type error
    assert (tmp_path / "clearance.bin").read_bytes() == got.tobytes()
