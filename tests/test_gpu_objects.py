"""GPU: the objects of a region (sdr_find_objects*, csrc/sdr_objects.hip) through every layer: every
record, the scan record and the label map compared bit for bit with the numpy restatement
(tests/objects_ref.py)."""
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
import objects_ref as OR  # noqa: E402
import plane_ref as PR  # noqa: E402
import plane_search_ref as SR  # noqa: E402
import relief_ref as LR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import (FOOTPRINT_DTYPE, OBJECT_DTYPE, OBJECT_SCAN_DTYPE, PLANE_DTYPE,  # noqa: E402
                                          RELIEF_DTYPE, as_relief_queries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = S.REFERENCE_Q
EYE = np.eye(4)
TILE = 32  # csrc/sdr_objects.hip, kObjTile
X0, Y0 = 3, 5  # a planted rectangle's origin in its map


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def flat_plane(offset=0.0, normal=(0.0, 0.0, 1.0), flags=PR.OK):
    """With Q the identity and this record, hf is the float disparity itself (+0 for -0)."""
    p = np.zeros(1, PLANE_DTYPE)
    p["normal"], p["offset"], p["flags"] = normal, offset, flags
    return p


def host(rec, scan, lab):
    torch.cuda.synchronize()
    return (rec.cpu().numpy().reshape(-1).view(OBJECT_DTYPE), scan.cpu().numpy().view(OBJECT_SCAN_DTYPE)[0],
            lab.cpu().numpy() if lab is not None else None)


def check_objects(disp, planes, region, labels=None, conf=None, Qm=Q, min_disp=-1.0, conf_min=0.0, **kw):
    """Device records, scan and labels == the restatement's, on every bit.  disp: a numpy map (a view
    with a row stride is passed on as one)."""
    r = sdr.Ruler(Qm, min_disp=min_disp, conf_min=conf_min)
    base = disp.base if disp.base is not None and disp.base.ndim == disp.ndim else None
    if base is not None:  # keep the stride: the same slice of the tensor
        d = torch.from_numpy(np.ascontiguousarray(base)).to(dev())[..., :disp.shape[-1]]
        assert d.stride(-2) > d.shape[-1]
    else:
        d = torch.from_numpy(np.ascontiguousarray(disp)).to(dev())
    c = torch.from_numpy(np.ascontiguousarray(conf)).to(dev()) if conf is not None else None
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev()) if labels is not None else None
    got = host(*r.find_objects_device(d, planes, region, labels=lab, conf=c, labels_out=True, **kw))
    want = OR.find_objects(disp, planes, region, Qm, labels=labels, conf=conf, min_disp=min_disp, conf_min=conf_min,
                           **kw)
    OR.assert_objects_equal(got, want[:3])
    return got


def embed(rect, fill, dtype=np.float32, pad=7):
    """The (rh, rw) map `rect` at (X0, Y0) of frame 1 of a (2, rh + 9, rw + 8) map whose rows are
    rw + 8 + pad apart; the rest holds `fill` (members that would join across the rectangle's edge
    if the rectangle did not bound adjacency).  Returns (the strided view, the region's corners)."""
    rh, rw = rect.shape
    full = np.full((2, rh + 9, rw + 8 + pad), fill, dtype)
    view = full[:, :, :rw + 8]
    view[1, Y0:Y0 + rh, X0:X0 + rw] = rect
    return view, (1, X0, Y0, X0 + rw - 1, Y0 + rh - 1)


PLANTED = dict(Qm=EYE, min_disp=-3e38, h_range=(0.0, 100000.0))


def planted(rect, fill=20.0, plane=None, label=-1, **kw):
    view, reg = embed(np.asarray(rect, np.float32), fill)
    args = dict(PLANTED, **kw)
    return check_objects(view, flat_plane() if plane is None else plane, reg + (0, label), **args)


def holes(H, W):
    return np.full((H, W), -1.0, np.float32)


# ---- sizes ----
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1), (31, 65), (33, 33), (64, 64), (97, 67)])
def test_sizes(H, W):
    rng = np.random.default_rng(H * 100 + W)
    d = (20.0 + 0.75 * rng.integers(0, 3, (H, W))).astype(np.float32)
    d[rng.random((H, W)) < 0.35] = -50.0  # below the band
    for conn in (4, 8):
        objs, scan, lab = planted(d, connectivity=conn, min_pixels=1, max_objects=64, max_diff=0.75)
        assert scan["area"] == H * W and scan["n"] == int((d > 0).sum()) and scan["n_valid"] == H * W
    # every pixel one value: one component that touches every border
    objs, scan, lab = planted(np.full((H, W), 20.0, np.float32), min_pixels=1)
    assert scan["count"] == 1 and objs["n"][0] == H * W and objs["root"][0] == 0 and objs["flags"][0] == 3
    assert (objs["x0"][0], objs["y0"][0], objs["x1"][0], objs["y1"][0]) == (X0, Y0, X0 + W - 1, Y0 + H - 1)


# ---- patterns ----
def test_checkerboard():
    H, W = 34, 66
    vv, uu = np.mgrid[0:H, 0:W]
    d = np.where((vv + uu) % 2 == 0, 20.0, -50.0).astype(np.float32)
    n = int((d > 0).sum())
    objs, scan, _ = planted(d, connectivity=4, min_pixels=1, max_objects=64)
    assert scan["n_components"] == n == scan["n_kept"] and scan["flags"] == OR.VALID | OR.TRUNCATED
    assert objs["n"].tolist() == [1] * 64 and objs["root"].tolist() == np.flatnonzero(d > 0)[:64].tolist()
    objs, scan, _ = planted(d, connectivity=8, min_pixels=1, max_objects=64)
    assert scan["n_components"] == 1 and objs["n"][0] == n and scan["flags"] == OR.VALID


def spiral(H, W):
    """A one-pixel-wide spiral from (0, 0) inwards: its cells in walking order."""
    m = np.zeros((H, W), bool)
    v = u = 0
    dv, du = 0, 1
    m[0, 0] = True
    order = [(0, 0)]
    while True:
        for _ in range(2):  # forward, else one turn to the right
            nv, nu = v + dv, u + du
            fv, fu = nv + dv, nu + du
            if 0 <= nv < H and 0 <= nu < W and not m[nv, nu] and not (0 <= fv < H and 0 <= fu < W and m[fv, fu]):
                v, u = nv, nu
                m[v, u] = True
                order.append((v, u))
                break
            dv, du = du, -dv
        else:
            return order


def serpentine(H, W):
    """Every other row in full, joined at alternating ends: its cells in walking order."""
    order = []
    for v in range(H):
        if v % 2 == 0:
            us = range(W) if (v // 2) % 2 == 0 else range(W - 1, -1, -1)
            order += [(v, u) for u in us]
        else:
            order.append((v, W - 1 if (v // 2) % 2 == 0 else 0))
    return order


@pytest.mark.parametrize("H,W", [(64, 64), (97, 67)])
@pytest.mark.parametrize("path", [spiral, serpentine])
def test_one_chain_through_every_tile(path, H, W):
    order = path(H, W)
    d = holes(H, W)
    # a step of exactly max_diff along the chain: only consecutive cells are joined
    for i, (v, u) in enumerate(order):
        d[v, u] = 20.0 + 0.25 * i
    for conn in (4, 8):
        objs, scan, lab = planted(d, fill=-1.0, connectivity=conn, min_pixels=1, max_diff=0.25)
        assert scan["n_components"] == 1 and objs["n"][0] == len(order) and objs["root"][0] == 0
        assert int((lab == 0).sum()) == len(order)
    # one step in the middle is a hair too large: two chains
    k = len(order) // 2
    for v, u in order[k:]:
        d[v, u] = np.nextafter(np.float32(d[v, u] + 0.25), np.float32(np.inf))
    objs, scan, _ = planted(d, fill=-1.0, connectivity=4, min_pixels=1, max_diff=0.25)
    assert scan["n_components"] >= 2 and objs["n"][0] >= k and objs["n"][:2].sum() <= len(order)


def test_combs_joined_in_the_last_row():
    for H, W in ((66, 70), (33, 97)):
        d = holes(H, W)
        d[:, ::2] = 20.0
        d[H - 1, :] = 20.0
        objs, scan, _ = planted(d, fill=-1.0, connectivity=4, min_pixels=1)
        assert scan["n_components"] == 1 and objs["n"][0] == int((d > 0).sum())
        d[H - 1, :] = -1.0  # without the back: the teeth alone
        objs, scan, _ = planted(d, fill=-1.0, connectivity=8, min_pixels=1, max_objects=64)
        assert scan["n_components"] == (W + 1) // 2 and (objs["n"][:scan["count"]] == H - 1).all()
        assert objs["root"][:scan["count"]].tolist() == list(range(0, W, 2))[:scan["count"]]  # equal sizes: by root
        # upside down: the teeth join in the first row
        d = np.ascontiguousarray(d[::-1])
        d[0, :] = 20.0
        objs, scan, _ = planted(d, fill=-1.0, connectivity=4, min_pixels=1)
        assert scan["n_components"] == 1 and objs["root"][0] == 0


def test_diagonals_through_a_tile_corner():
    for H, W in ((64, 64), (33, 40)):
        for a, b in (((TILE - 1, TILE - 1), (TILE, TILE)), ((TILE - 1, TILE), (TILE, TILE - 1))):  # (v, u)
            d = holes(H, W)
            d[a] = d[b] = 20.0
            objs, scan, _ = planted(d, fill=-1.0, connectivity=8, min_pixels=1)
            assert scan["n_components"] == 1 and objs["n"][0] == 2 and objs["root"][0] == a[0] * W + a[1]
            objs, scan, _ = planted(d, fill=-1.0, connectivity=4, min_pixels=1)
            assert scan["n_components"] == 2 and objs["n"][:2].tolist() == [1, 1]
            # and one pixel off the corner, across one border only
            d = holes(H, W)
            d[a[0], a[1] - 1 if a[1] < TILE else a[1] + 1] = d[b] = 20.0
            planted(d, fill=-1.0, connectivity=8, min_pixels=1)


# ---- the join threshold ----
def test_join_threshold_float():
    H, W = 3, 40
    md = 0.75
    a = np.float32(20.0)
    exact, above = np.float32(20.75), np.nextafter(np.float32(20.75), np.float32(np.inf))
    assert np.float32(exact - a) == np.float32(md) and np.float32(above - a) > np.float32(md)
    for conn in (4, 8):
        d = holes(H, W)
        d[1, 3], d[1, 4] = a, exact       # joined
        d[1, 10], d[1, 11] = a, above     # not joined
        d[0, 30], d[1, 31] = exact, a     # a diagonal pair at exactly max_diff
        objs, scan, _ = planted(d, fill=-1.0, connectivity=conn, min_pixels=1, max_diff=md)
        assert scan["n_components"] == (4 if conn == 8 else 5) and objs["n"][0] == 2
    # max_diff = 0: only equal disparities
    d = np.full((H, W), 20.0, np.float32)
    d[:, 20:] = np.nextafter(np.float32(20.0), np.float32(np.inf))
    d[1, 5] = -0.0  # hf = +0 is inside a band that starts at 0; -0.0 == 0.0 joins nothing here
    objs, scan, _ = planted(d, connectivity=8, min_pixels=1, max_diff=0.0)
    assert scan["n_components"] == 3 and sorted(objs["n"][:3].tolist()) == [1, 20 * H - 1, 20 * H]


def test_join_threshold_int16():
    H, W = 4, 36
    full = np.full((2, H + 9, W + 8 + 6), -16, np.int16)
    view = full[:, :, :W + 8]
    rect = view[1, Y0:Y0 + H, X0:X0 + W]
    rect[1, 2], rect[1, 3] = 320, 336          # 16 * max_diff apart: joined
    rect[1, 10], rect[1, 11] = 320, 337        # one more: not joined
    rect[2, 20], rect[3, 21] = 336, 320        # a diagonal pair
    reg = (1, X0, Y0, X0 + W - 1, Y0 + H - 1, 0, -1)
    for conn in (4, 8):
        objs, scan, _ = check_objects(view, flat_plane(), reg, Qm=EYE, h_range=(0.0, 1000.0), connectivity=conn,
                                      min_pixels=1, max_diff=1.0)
        assert scan["n_components"] == (4 if conn == 8 else 5) and scan["n"] == 6
    objs, scan, _ = check_objects(view, flat_plane(), reg, Qm=EYE, h_range=(0.0, 1000.0), min_pixels=1, max_diff=0.0)
    assert scan["n_components"] == 6


# ---- ranking ----
def blobs(H, W, boxes, value=20.0):
    d = holes(H, W)
    for x, y, w, h in boxes:
        d[y:y + h, x:x + w] = value
    return d


def test_ranking():
    H, W = 40, 90
    # equal sizes are ordered by root, larger ones first
    boxes = [(50, 2, 3, 4), (2, 20, 4, 3), (70, 20, 2, 6), (20, 1, 5, 5), (40, 30, 4, 3), (10, 10, 6, 2)]
    d = blobs(H, W, boxes)
    objs, scan, lab = planted(d, fill=-1.0, min_pixels=12, max_objects=8)
    assert scan["n_kept"] == 6 and objs["n"][:6].tolist() == [25] + [12] * 5
    assert objs["root"][:6].tolist() == [1 * W + 20, 2 * W + 50, 10 * W + 10, 20 * W + 2, 20 * W + 70, 30 * W + 40]
    assert not (objs["flags"][:6] & OR.OBJECT_CUT).any() and objs["n"][6] == 0 and objs["root"][6] == -1
    # sizes min_pixels and min_pixels - 1
    objs, scan, _ = planted(d, fill=-1.0, min_pixels=13, max_objects=8)
    assert scan["n_kept"] == 1 and scan["largest_dropped"] == 12 and scan["n_components"] == 6
    objs, scan, _ = planted(d, fill=-1.0, min_pixels=26, max_objects=8)
    assert scan["flags"] == OR.EMPTY and scan["largest_dropped"] == 25 and scan["count"] == 0
    # more kept than max_objects: TRUNCATED; max_objects 1 and 64
    for mo in (1, 3, 64):
        objs, scan, lab = planted(d, fill=-1.0, min_pixels=1, max_objects=mo)
        assert scan["count"] == min(mo, 6) and bool(scan["flags"] & OR.TRUNCATED) == (mo < 6)
        assert len(objs) == mo and int((lab != 255).sum()) == int(objs["n"].sum())
    # 70 singletons and max_objects 64; candidates in more than one slice of 2048 pixels
    d = holes(70, 70)
    d[::9, ::8] = 20.0
    objs, scan, _ = planted(d, fill=-1.0, min_pixels=1, max_objects=64)
    assert scan["n_kept"] == 72 and scan["count"] == 64 and scan["flags"] == OR.VALID | OR.TRUNCATED


# ---- members ----
def test_band_edges_and_invalid_values():
    H, W = 6, 40
    d = np.full((H, W), 50.0, np.float32)
    below, above = np.nextafter(np.float32(10.0), np.float32(0)), np.nextafter(np.float32(90.0), np.float32(99))
    d[0, :8] = [10.0, below, 90.0, above,
                np.nan, np.inf, -np.inf, -0.0]
    objs, scan, lab = planted(d, fill=50.0, h_range=(10.0, 90.0), min_pixels=1, max_diff=40.0)
    assert scan["n_valid"] == H * W - 3 and scan["n"] == H * W - 6  # NaN, +-inf invalid; two outside the band; -0 below
    assert lab[Y0, X0] == 0 and lab[Y0, X0 + 1] == 255 and lab[Y0, X0 + 2] == 0 and lab[Y0, X0 + 3] == 255
    assert objs["h_min"][0] == 10.0 and objs["h_max"][0] == 90.0
    # a band that starts at 0 takes -0.0 as +0; h_lo == h_hi takes exactly that height
    objs, scan, lab = planted(d, fill=50.0, h_range=(0.0, 1.0), min_pixels=1)
    assert scan["n"] == 1 and objs["h_min"].view(np.uint32)[0] == 0 and objs["sum256"][0] == 0
    objs, scan, _ = planted(d, fill=50.0, h_range=(90.0, 90.0), min_pixels=1)
    assert scan["n"] == 1 and objs["x0"][0] == X0 + 2
    # an offset plane moves the band; min_disp is strict
    planted(d, fill=50.0, plane=flat_plane(-40.0), h_range=(10.0, 50.0), min_pixels=1, max_diff=40.0)
    objs, scan, _ = planted(d, fill=50.0, min_disp=50.0, min_pixels=1)
    assert scan["n_valid"] == 2 and scan["n"] == 2


def test_confidence_and_label_masks():
    rng = np.random.default_rng(9)
    F, H, W = 2, 45, 75
    d = (20.0 + 0.75 * rng.integers(0, 3, (F, H, W))).astype(np.float32)
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    conf[rng.random((F, H, W)) < 0.1] = np.nan
    lab_in = rng.choice(np.array([0, 7, 255], np.uint8), (F, H, W))
    for label in (-1, 0, 7, 255, 3):
        reg = (1, 2, 1, W - 3, H - 2, 0, label)
        objs, scan, lab = check_objects(d, flat_plane(), reg, labels=lab_in, conf=conf, Qm=EYE, conf_min=60.0,
                                        h_range=(0.0, 100.0), min_pixels=2, max_diff=0.75)
        want_masked = (W - 4) * (H - 2) if label < 0 else int((lab_in[1, 1:H - 1, 2:W - 2] == label).sum())
        assert scan["n_masked"] == want_masked and scan["n"] <= scan["n_valid"] < max(want_masked, 1)
    # a label >= 0 without a map is out of range
    objs, scan, lab = check_objects(d, flat_plane(), (1, 2, 1, W - 3, H - 2, 0, 7), Qm=EYE, h_range=(0.0, 100.0))
    assert scan["flags"] == OR.OUT_OF_RANGE


# ---- refusals ----
def test_refusal_records():
    d = np.full((2, 12, 40), 5.0, np.float32)
    lab_in = np.zeros((2, 12, 40), np.uint8)
    pl = np.concatenate([flat_plane(), flat_plane(flags=PR.DEGENERATE)])
    kw = dict(Qm=EYE, h_range=(0.0, 10.0), min_pixels=1, max_objects=3, min_disp=-3e38)
    for reg, flag in (((2, 0, 0, 7, 5, 0, -1), OR.OUT_OF_RANGE), ((0, 0, 0, 40, 5, 0, -1), OR.OUT_OF_RANGE),
                      ((0, 0, -1, 7, 5, 0, -1), OR.OUT_OF_RANGE), ((0, 0, 0, 7, 5, 0, 256), OR.OUT_OF_RANGE),
                      ((0, 0, 0, 7, 5, 0, -2), OR.OUT_OF_RANGE), ((0, 0, 0, 7, 5, -1, -1), OR.NO_PLANE),
                      ((0, 0, 0, 7, 5, 2, -1), OR.NO_PLANE), ((1, 7, 5, 0, 0, 1, 0), OR.NO_PLANE)):
        objs, scan, lab = check_objects(d, pl, reg, labels=lab_in, **kw)
        assert scan["flags"] == flag and (lab == 255).all() and (objs["root"] == -1).all()
    # no plane record at all
    objs, scan, _ = check_objects(d, np.zeros(0, PLANE_DTYPE), (0, 0, 0, 7, 5, 0, -1), **kw)
    assert scan["flags"] == OR.NO_PLANE and scan["area"] == 48
    # EMPTY: no member; members but none kept
    objs, scan, _ = check_objects(d, pl, (0, 0, 0, 7, 5, 0, -1), **dict(kw, h_range=(6.0, 10.0)))
    assert scan["flags"] == OR.EMPTY and (scan["n_valid"], scan["n"], scan["n_components"]) == (48, 0, 0)
    objs, scan, _ = check_objects(d, pl, (0, 0, 0, 7, 5, 0, -1), **dict(kw, min_pixels=49))
    assert scan["flags"] == OR.EMPTY and (scan["n"], scan["n_components"], scan["largest_dropped"]) == (48, 1, 48)
    # corners in any order give one answer
    a = check_objects(d, pl, (1, 30, 9, 3, 2, 0, -1), **kw)
    b = check_objects(d, pl, (1, 3, 2, 30, 9, 0, -1), **kw)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])


# ---- hypothesis ----
@settings(max_examples=hyp_examples(25), deadline=None, derandomize=True, database=None,
          suppress_health_check=list(HealthCheck))
@given(H=st.integers(1, 100), W=st.integers(1, 100), density=st.floats(0.3, 0.9), levels=st.integers(2, 6),
       conn=st.sampled_from([4, 8]), i16=st.booleans(), min_pixels=st.sampled_from([1, 2, 5, 20]),
       max_objects=st.sampled_from([1, 4, 16, 64]), seed=st.integers(0, 2 ** 32 - 1))
def test_hypothesis_random_maps(H, W, density, levels, conn, i16, min_pixels, max_objects, seed):
    rng = np.random.default_rng(seed)
    d = (20.0 + 0.75 * rng.integers(0, levels, (H, W))).astype(np.float32)
    d[rng.random((H, W)) >= density] = -1.0
    dt = np.int16 if i16 else np.float32
    view, reg = embed((d * 16).astype(np.int16) if i16 else d, -16 if i16 else -1.0, dtype=dt)
    check_objects(view, flat_plane(), reg + (0, -1), Qm=EYE, h_range=(0.0, 100.0), connectivity=conn,
                  min_pixels=min_pixels, max_objects=max_objects, max_diff=0.75)


# ---- a frame ----
def test_one_640x360_frame_of_blobs():
    rng = np.random.default_rng(4)
    H, W = 360, 640
    d = holes(H, W)
    vv, uu = np.mgrid[0:H, 0:W]
    for _ in range(60):
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(4, 60), rng.integers(4, 90)
        inside = ((vv - cy) / ry) ** 2 + ((uu - cx) / rx) ** 2 <= 1.0
        d[inside] = np.float32(20.0 + 1.5 * rng.integers(0, 12)) + (0.0625 * rng.integers(0, 4, (H, W)))[inside]
    d[rng.random((H, W)) < 0.1] = -1.0
    objs, scan, lab = check_objects(d[None], flat_plane(), (0, 0, 0, W - 1, H - 1, 0, -1), Qm=EYE, h_range=(0.0, 100.0),
                                    min_pixels=64, max_objects=16)
    assert scan["count"] >= 4 and scan["n_components"] > scan["count"]
    assert (np.diff(objs["n"][:scan["count"]]) <= 0).all()


# ---- the feature's scene on the device, and the chain find_planes -> find_objects -> relief / footprint ----
def test_two_object_scene_feeds_relief_and_footprint():
    Qw = FR.scene_q(Q)
    d, truth, info = OR.two_object_scene(Qw)
    H, W = truth.shape
    planes, count, _, plab = SR.find_planes(d, (0, 0, 0, W - 1, H - 1), Qw, max_planes=3, hypotheses=256,
                                            min_inliers=1000, seed=0)
    floor_i = int(np.argmax([((plab == i) & (truth == 0)).sum() for i in range(count)]))
    whole = (0, 0, 0, W - 1, H - 1, floor_i, -1)
    kw = dict(h_range=(10.0, 1000.0), max_diff=1.0, connectivity=8, min_pixels=64)
    r = sdr.Ruler(Qw)
    dt = torch.from_numpy(d).to(dev())
    rec, scan_t, lab_t = r.find_objects_device(dt, planes, whole, labels_out=True, **kw)
    regs = [(0, 0, 0, W - 1, H - 1, floor_i, k) for k in range(2)]
    rel = r.relief_device(dt, planes, regs, labels=lab_t)
    foot = r.footprint_device(dt, planes, regs, labels=lab_t)
    objs, scan, lab = host(rec, scan_t, lab_t)
    OR.assert_objects_equal((objs, scan, lab), OR.find_objects(d, planes, whole, Qw, **kw)[:3])
    assert scan["n_kept"] == 2 and scan["count"] == 2 and scan["largest_dropped"] < 64
    rel = rel.cpu().numpy().reshape(-1).view(RELIEF_DTYPE)
    foot = foot.cpu().numpy().reshape(-1).view(FOOTPRINT_DTYPE)
    for k in range(2):
        assert rel["n"][k] == objs["n"][k] and rel["sum256"][k] == objs["sum256"][k]
        assert rel["h_min"][k] == objs["h_min"][k] and rel["h_max"][k] == objs["h_max"][k]
        assert foot["flags"][k] & FR.VALID and foot["n"][k] == objs["n"][k]
    LR.assert_reliefs_equal(rel, LR.relief(d, planes, regs, Qw, labels=lab))
    box_k = int(np.argmax([((lab == k) & (truth == 1)).sum() for k in range(2)]))
    length, width = sdr.footprint_length_width(foot[box_k:box_k + 1])
    assert abs(length[0] - 150.0) < 25.0 and abs(width[0] - 100.0) < 25.0  # the footprint test's bound is 21.6 mm
    # the host-pointer entry, the tensor form of find_objects, and no label map: the same records
    got = r.find_objects(d, planes, whole, **kw)
    assert got[0].tobytes() == objs[:2].tobytes() and got[1].tobytes() == scan.tobytes() and np.array_equal(got[2], lab)
    got = r.find_objects(dt, planes, whole, labels_out=False, **kw)
    assert got[0].tobytes() == objs[:2].tobytes() and got[1].tobytes() == scan.tobytes() and got[2] is None
    bare = host(*r.find_objects_device(dt, planes, whole, labels_out=None, **kw))
    assert bare[0].tobytes() == objs.tobytes() and bare[1].tobytes() == scan.tobytes() and bare[2] is None
    out = torch.zeros((H, W), dtype=torch.uint8, device=dev())
    same = host(*r.find_objects_device(dt, planes, whole, labels_out=out, **kw))
    assert same[2] is not None and np.array_equal(out.cpu().numpy(), lab)
    with pytest.raises(sdr.SDRError):
        r.find_objects_device(dt, planes, whole, labels=out, labels_out=out, **kw)


def test_host_abi_forms():
    rng = np.random.default_rng(14)
    F, H, W = 2, 40, 70
    d = (20.0 + 0.75 * rng.integers(0, 3, (F, H, W))).astype(np.float32)
    d[rng.random((F, H, W)) < 0.3] = -1.0
    conf = rng.uniform(0, 255, (F, H, W)).astype(np.float32)
    lab_in = rng.integers(0, 2, (F, H, W)).astype(np.uint8)
    pl = flat_plane()
    reg = (1, 2, 1, W - 2, H - 3, 0, 1)
    kw = dict(h_range=(0.0, 100.0), max_diff=0.75, connectivity=4, min_pixels=3, max_objects=5)
    r = sdr.Ruler(EYE, conf_min=30.0)
    for disp in (d, (d * 16).astype(np.int16)):
        want = OR.find_objects(disp, pl, reg, EYE, labels=lab_in, conf=conf, conf_min=30.0, **kw)
        n = int(want[1]["count"])
        got = r.find_objects(disp, pl, reg, labels=lab_in, conf=conf, **kw)  # host pointers
        OR.assert_objects_equal(got, (want[0][:n], want[1], want[2]))
        t = lambda a: torch.from_numpy(a).to(dev())  # noqa: E731
        got = r.find_objects(t(disp), pl, reg, labels=t(lab_in), conf=t(conf), **kw)  # tensors
        OR.assert_objects_equal(got, (want[0][:n], want[1], want[2]))
        pt = t(np.ascontiguousarray(pl).view(np.uint8).reshape(-1, 128))
        qt = t(as_relief_queries(reg))
        got = host(*r.find_objects_device(t(disp), pt, qt, labels=lab_in, conf=t(conf), labels_out=True, **kw))
        OR.assert_objects_equal(got, want[:3])
    # an (H, W) map, a region of 5 entries
    one = sdr.Ruler(EYE).find_objects(d[0], pl, (0, 0, 0, W - 1, H - 1), h_range=(0.0, 100.0))
    OR.assert_objects_equal(one, (lambda w: (w[0][:w[1]["count"]], w[1], w[2]))(
        OR.find_objects(d[:1], pl, (0, 0, 0, W - 1, H - 1), EYE, h_range=(0.0, 100.0))))


def test_chain_on_a_side_stream():
    """find_planes_device -> find_objects_device(label 255, planes and labels as tensors) -> relief_device
    on a stream that is not the default one, no synchronise in between."""
    Qw = FR.scene_q(Q)
    d, truth, info = OR.two_object_scene(Qw)
    H, W = truth.shape
    r = sdr.Ruler(Qw)
    dt = torch.from_numpy(d).to(dev())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    kw = dict(h_range=(10.0, 1000.0), min_pixels=64, max_objects=4)
    whole = (0, 0, 0, W - 1, H - 1, 0, 255)
    regs = [(0, 0, 0, W - 1, H - 1, 0, k) for k in range(4)]
    with torch.cuda.stream(side):
        planes, count, _, plab = r.find_planes_device(dt, None, max_planes=2, hypotheses=256, min_inliers=1000, seed=0,
                                                      labels=True, stream=side)
        rec, scan_t, lab_t = r.find_objects_device(dt, planes, whole, labels=plab, stream=side, labels_out=True, **kw)
        rel = r.relief_device(dt, planes, regs, labels=lab_t, stream=side)
    side.synchronize()
    pl = planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    objs, scan, lab = host(rec, scan_t, lab_t)
    OR.assert_objects_equal((objs, scan, lab), OR.find_objects(d, pl, whole, Qw, labels=plab.cpu().numpy(), **kw)[:3])
    rel = rel.cpu().numpy().reshape(-1).view(RELIEF_DTYPE)
    # two planes leave the hemisphere unclaimed: the one object of label 255
    assert scan["count"] == 1 and scan["n_masked"] == int((plab.cpu().numpy() == 255).sum())
    for k in range(4):
        assert rel["n"][k] == objs["n"][k] and rel["sum256"][k] == objs["sum256"][k]
        assert (rel["flags"][k] == LR.VALID) == (k < scan["count"])


def test_live_loop_find_objects_on_the_frame_stream():
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
    ok = dict(h_range=(-1048576.0, 1048576.0), max_diff=1.0, min_pixels=8, max_objects=6)
    w2, h2 = loop.w2, loop.h2
    whole = (0, 0, 0, w2 - 1, h2 - 1, 0, 255)
    with torch.cuda.stream(side):
        loop.enqueue(frame, side)
        planes, count, _, plab = loop.find_planes(None, side, labels=True, **kw)
        rec, scan_t, lab_t = loop.find_objects(planes, whole, side, labels=plab, **ok)
        rel = loop.relief(planes, [(0, 0, 0, w2 - 1, h2 - 1, 0, 0)], side, labels=lab_t)
    side.synchronize()
    disp, conf = loop.disp.cpu().numpy(), loop.conf.cpu().numpy()
    pl = planes.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    objs, scan, lab = host(rec, scan_t, lab_t)
    want = OR.find_objects(disp, pl, whole, Q, labels=plab.cpu().numpy(), conf=conf, min_disp=loop.ruler.min_disp,
                           conf_min=100.0, **ok)
    OR.assert_objects_equal((objs, scan, lab), want[:3])
    assert int(count.cpu()[0]) >= 1
    rel = rel.cpu().numpy().reshape(-1).view(RELIEF_DTYPE)
    assert rel["n"][0] == objs["n"][0]
    check(lib().sdr_rectifier_reset_stream(rect._h))
    loop.close()


def test_cpp_facade_objects(tmp_path):
    """include/sdr/stereo.hpp: sdr::Ruler::find_objects gives Python's records as bytes
    (tests/cpp/facade_objects.cpp)."""
    exe = tmp_path / "facade_objects"
    libdir = os.path.join(ROOT, "stereo_depth_ruler_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_objects.cpp"), "-L", libdir, "-lsdr",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    Qw = FR.scene_q(Q)
    d, truth, info = OR.two_object_scene(Qw)
    H, W = truth.shape
    d[0].tofile(tmp_path / "disp.bin")
    np.asarray(Qw, np.float64).tofile(tmp_path / "q.bin")
    res = subprocess.run([str(exe), str(W), str(H), "2", "256", "0", str(tmp_path)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    r = sdr.Ruler(Qw)
    planes, plab = r.find_planes(d, None, max_planes=2, hypotheses=256, seed=0, min_inliers=1000, labels=True)
    whole = (0, 0, 0, W - 1, H - 1, 0, 255)
    kw = dict(h_range=(10.0, 1000.0), min_pixels=64, max_objects=4)
    objs, scan, lab = r.find_objects(d, planes, whole, labels=plab, **kw)
    want = OR.find_objects(d, planes, whole, Qw, labels=plab, **kw)
    OR.assert_objects_equal((objs, scan, lab), (want[0][:scan["count"]], want[1], want[2]))
    assert f"planes={len(planes)} objects={len(objs)} count={len(objs)}" in res.stdout and len(objs) >= 1
    assert "single_equal=1" in res.stdout and "no_labels_equal=1" in res.stdout
    assert "bad_connectivity_code=-1" in res.stdout
    assert (tmp_path / "planes.bin").read_bytes() == planes.tobytes()
    assert (tmp_path / "objects.bin").read_bytes() == objs.tobytes()
    assert (tmp_path / "scan.bin").read_bytes() == scan.tobytes()
    assert (tmp_path / "labels.bin").read_bytes() == lab.tobytes()
    regs = [(0, 0, 0, W - 1, H - 1, 0, k) for k in range(len(objs))]
    assert (tmp_path / "relief.bin").read_bytes() == LR.relief(d, planes, regs, Qw, labels=lab).tobytes()
