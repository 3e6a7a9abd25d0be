"""GPU: a ruler call addresses a frame's maps by one rule (csrc/sdr_ruler_shared.hpp, RegionMaps): the
disparity by its row and frame strides, the dense confidence and label maps by H * W a frame, a
rectangle by its origin in each.  The same query goes to each of the eight device entries twice: on
frame 2 of a strided view of a larger buffer, beside dense confidence and label maps of three
frames, and on frame 0 of dense copies of that frame's three maps.  Every byte of the two results
must be equal but the records' `frame` field.  Whatever a wrong offset would reach instead holds
something else: the buffer around the view a confident-looking 60 px, frames 0 and 1 a constant
5 px with confidence 0 and label 7."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import plane_ref as PR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd import ruler as R  # noqa: E402

Q = S.REFERENCE_Q
# 3500 pixels: two slices of 2048 (csrc/sdr_region.hpp, kRegionSlice), the second ragged, and 2 x 3
# tiles of 32 x 32 (csrc/sdr_objects.hip) with ragged edges
F, H, W = 3, 50, 70
PAD_H, PAD_W = 2, 5  # stride(1) = W + 5, stride(0) = (H + 2)(W + 5) > stride(1) * H
WHOLE = (0, 0, W - 1, H - 1)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def scene():
    """(disparity of frame 2 in px, a plane fitted to it, conf (3, H, W), labels (3, H, W)): frame 2 a
    ramp with noise, 15 % holes and a few zeros (valid, but their points are not finite: n < n_valid),
    confidences with NaNs, labels in 0..2; frames 0 and 1 confidence 0 and label 7."""
    rng = np.random.default_rng(29)
    ys, xs = np.mgrid[0:H, 0:W]
    d = (30.0 + 0.05 * xs - 0.03 * ys) + rng.normal(0, 0.4, (H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    d[rng.random((H, W)) < 0.15] = -1.0
    d[rng.random((H, W)) < 0.05] = 0.0
    planes = PR.fit_planes(d[None], [(0,) + WHOLE], Q)
    assert planes["flags"].tolist() == [PR.OK]
    conf = np.zeros((F, H, W), np.float32)
    conf[2] = rng.random((H, W))
    conf[2][rng.random((H, W)) < 0.1] = np.nan
    labels = np.full((F, H, W), 7, np.uint8)
    labels[2] = rng.integers(0, 3, (H, W))
    return d, planes, conf, labels


def _maps(scene, s16):
    """((view, conf, labels) of three frames, (dense, conf, labels) of frame 2 alone) on the device."""
    d, _, conf, labels = scene
    dev = torch.device("cuda", 0)
    buf = np.full((F, H + PAD_H, W + PAD_W), 60.0, np.float32)
    buf[:2, :H, :W] = 5.0
    buf[2, :H, :W] = d
    if s16:
        buf = (buf * 16).astype(np.int16)
    view = torch.from_numpy(buf).to(dev)[:, :H, :W]
    assert view.stride(1) == W + PAD_W and view.stride(0) == (H + PAD_H) * (W + PAD_W) > view.stride(1) * H
    c, lab = torch.from_numpy(conf).to(dev), torch.from_numpy(labels).to(dev)
    return (view, c, lab), (view[2].contiguous(), c[2].contiguous(), lab[2].contiguous())


def _host(t, dtype=None):
    """A result tensor (or None) as host bytes, or as records with their `frame` field cleared."""
    if t is None:
        return None
    a = t.cpu().numpy()
    if dtype is None:
        return a
    a = a.reshape(-1).view(dtype).copy()
    if "frame" in dtype.names:
        a["frame"] = 0
    return a


# each entry: (ruler, disparity, conf, labels, planes, frame) -> the call's outputs on the host
def _measure(r, d, c, lab, planes, f):
    rec, prof = r.measure_device(d, [(f,) + WHOLE, (f, W - 1, 0, 2, H - 1)], c)
    return [_host(rec, R.MEASUREMENT_DTYPE), _host(prof)]


def _fit_plane(r, d, c, lab, planes, f):
    return [_host(r.fit_plane_device(d, [(f,) + WHOLE, (f, W - 1, H - 1, 7, 9)], c), R.PLANE_DTYPE)]


def _find_planes(r, d, c, lab, planes, f):
    rec, count, rounds, out = r.find_planes_device(d, (f,) + WHOLE, c, max_planes=2, hypotheses=64, seed=5,
                                                   min_inliers=64, labels=True)
    return [_host(rec, R.PLANE_DTYPE), _host(count), _host(rounds), _host(out)]


def _plane_distance(r, d, c, lab, planes, f):
    return [_host(r.plane_distance_device(d, planes, [(f, 10, 11, 0), (f, W - 1, H - 1, 0), (f, 0, H - 1, 0)], c),
                  R.PLANE_DISTANCE_DTYPE)]


def _regions(f):
    return [(f,) + WHOLE + (0, -1), (f,) + WHOLE + (0, 1), (f, W - 1, H - 1, 33, 31, 0, 2)]


def _relief(r, d, c, lab, planes, f):
    return [_host(r.relief_device(d, planes, _regions(f), lab, c), R.RELIEF_DTYPE)]


def _footprint(r, d, c, lab, planes, f):
    # 70 x 50 px at 30 px of disparity are about 280 x 200 of Q's units: cells of 16, and no support
    # rule (a label's members are every sixth pixel), keep the sparse label queries' cells
    return [_host(r.footprint_device(d, planes, _regions(f), lab, c, cell=16.0, grid=64, support=1),
                  R.FOOTPRINT_DTYPE)]


def _find_objects(r, d, c, lab, planes, f):
    rec, scan, out = r.find_objects_device(d, planes, (f,) + WHOLE + (0, -1), lab, c, min_pixels=4, labels_out=True)
    return [_host(rec, R.OBJECT_DTYPE), _host(scan, R.OBJECT_SCAN_DTYPE), _host(out)]


def _clearance(r, d, c, lab, planes, f):
    return [_host(r.clearance_device(d, planes, [(f,) + WHOLE + (0, 1, 2), (f, 3, 2, W - 2, H - 3, 0, 2, 0)], lab, c),
                  R.CLEARANCE_DTYPE)]


def _decided(name, out, labels2):
    """The rule had something to decide in the result `out` of entry `name` on frame 2."""
    a = out[0]
    area = H * W
    if name == "measure":
        assert (a["flags"] & 3).tolist() == [3, 3] and (a["n0"] > 0).all() and (a["n1"] > 0).all()
        assert (a["n0"] < 9).all()  # both segments start in a corner: a window of 9, with holes
        assert (a["path_valid"] > 0).all() and a["path_samples"].tolist() == [W, W - 2]
    elif name == "fit_plane":
        assert a["flags"].tolist() == [R.PLANE_OK] * 2 and a["area"][0] == area
        assert ((0 < a["n_inliers"]) & (a["n_inliers"] <= a["n_valid"]) & (a["n_valid"] < a["area"])).all()
    elif name == "find_planes":
        assert int(out[1][0]) > 0 and a["flags"][0] == R.PLANE_OK and 0 < a["n_inliers"][0] <= a["n_valid"][0] < area
        assert 0 < int((out[3] == 0).sum()) < area and int((out[3] == 255).sum()) > 0
    elif name == "plane_distance":
        assert (a["flags"] & R.PDIST_VALID).all() and (a["n"] > 0).all()
    elif name in ("relief", "footprint"):
        valid = R.RELIEF_VALID if name == "relief" else R.FOOTPRINT_VALID
        assert (a["flags"] & valid).all() and a["area"].tolist() == [area, area, (W - 33) * (H - 31)]
        assert ((0 < a["n"]) & (a["n"] < a["n_valid"]) & (a["n_valid"] < a["n_masked"])).all()
        assert a["n_masked"][0] == area and a["n_masked"][1] == int((labels2 == 1).sum())
    elif name == "find_objects":
        scan = out[1][0]
        assert scan["flags"] & R.OBJECTS_VALID and scan["count"] > 0 and scan["area"] == area
        assert 0 < scan["n"] < scan["n_valid"] < area
        assert (a["flags"][:scan["count"]] & R.OBJECT_VALID).all() and int((out[2] != 255).sum()) == a["n"].sum()
    else:
        assert a["flags"].tolist() == [R.CLEARANCE_VALID] * 2 and a["area"][0] == area
        for k in ("n_a", "n_b", "m_a", "m_b"):
            assert (a[k] > 0).all(), k
        assert (a["n_a"] + a["n_b"] < a["area"]).all()


ENTRIES = {"measure": _measure, "fit_plane": _fit_plane, "find_planes": _find_planes,
           "plane_distance": _plane_distance, "relief": _relief, "footprint": _footprint,
           "find_objects": _find_objects, "clearance": _clearance}


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_frame_of_a_strided_view_is_its_dense_copy(scene, name, s16):
    (view, conf, labels), (dense, conf2, labels2) = _maps(scene, s16)
    planes = scene[1]
    r = sdr.Ruler(Q, radius=2, conf_min=0.5, profile=True)
    got = ENTRIES[name](r, view, conf, labels, planes, 2)
    want = ENTRIES[name](r, dense, conf2, labels2, planes, 0)
    other = ENTRIES[name](r, view, conf, labels, planes, 0)
    assert len(got) == len(want) == len(other)
    differs = False
    for i, (g, w, o) in enumerate(zip(got, want, other)):
        assert g.dtype == w.dtype and g.shape == w.shape
        same = g.tobytes() == w.tobytes()
        print(name, "output", i, g.dtype.names or g.dtype, g.shape, "equal" if same else "DIFFERS")
        assert same, f"{name}: output {i} of frame 2 of the view is not that of its dense copy"
        differs = differs or g.tobytes() != o.tobytes()
    _decided(name, got, scene[3][2])
    assert differs, f"{name}: frame 0 of the view gives frame 2's result"
