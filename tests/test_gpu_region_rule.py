"""GPU: the relief and the footprint apply one region rule (csrc/sdr_region.hpp).  The same queries
go to relief_device and to footprint_device without a band of heights: both must count the same
pixels and refuse the same queries.  Each side is compared with its numpy restatement by
test_gpu_relief.py and test_gpu_footprint.py; this test compares the two sides with each other, so
that a later copy of the rule in one of them is caught."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import plane_ref as PR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.ruler import (FOOTPRINT_DTYPE, FOOTPRINT_NO_PLANE, FOOTPRINT_OUT_OF_RANGE,  # noqa: E402
                                          RELIEF_DTYPE, RELIEF_NO_PLANE, RELIEF_OUT_OF_RANGE)

Q = S.REFERENCE_Q
H, W = 50, 70  # 3500 pixels: two slices of 2048 (csrc/sdr_region.hpp, kRegionSlice), the second ragged


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def scene():
    """The ramp with noise and holes of test_gpu_relief.py, a plane fitted to it and a record that is
    not a plane, a confidence map with NaNs, a label map."""
    rng = np.random.default_rng(11)
    ys, xs = np.mgrid[0:H, 0:W]
    d = (30.0 + 0.05 * xs - 0.03 * ys)[None] + rng.normal(0, 0.4, (1, H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    d[rng.random((1, H, W)) < 0.15] = -1.0
    planes = PR.fit_planes(d, [(0, 0, 0, W - 1, H - 1), (0, 0, 0, 0, H - 1)], Q)
    assert planes["flags"].tolist() == [PR.OK, PR.DEGENERATE]
    conf = rng.random((1, H, W)).astype(np.float32)
    conf[rng.random((1, H, W)) < 0.1] = np.nan
    labels = rng.integers(0, 3, (1, H, W)).astype(np.uint8)
    return d, planes, conf, labels


@pytest.mark.parametrize("with_conf", [False, True])
@pytest.mark.parametrize("s16", [False, True])
def test_relief_and_footprint_count_and_refuse_alike(scene, s16, with_conf):
    d, planes, conf, labels = scene
    whole = (0, 0, 0, W - 1, H - 1)
    regs = [whole + (0, -1),            # the whole frame
            (0, 5, 7, 5, 7, 0, -1),     # 1 x 1
            whole + (0, 1),             # one label
            (0, 3, 3, W, H - 1, 0, -1),  # a corner outside
            whole + (2, -1),            # a plane index past P
            whole + (1, -1)]            # a record without SDR_PLANE_OK
    dev = torch.device("cuda", 0)
    dm = torch.from_numpy((d * 16).astype(np.int16) if s16 else d).to(dev)
    c = torch.from_numpy(conf).to(dev) if with_conf else None
    lab = torch.from_numpy(labels).to(dev)
    r = sdr.Ruler(Q, conf_min=0.5)
    rel = r.relief_device(dm, planes, regs, labels=lab, conf=c)
    foot = r.footprint_device(dm, planes, regs, labels=lab, conf=c, grid=64, h_range=None)
    torch.cuda.synchronize()
    rel = rel.cpu().numpy().reshape(-1).view(RELIEF_DTYPE)
    foot = foot.cpu().numpy().reshape(-1).view(FOOTPRINT_DTYPE)
    for f in ("area", "n_masked", "n_valid", "n"):
        print(f, rel[f].tolist(), foot[f].tolist())
        assert rel[f].tolist() == foot[f].tolist(), f
    refused = [0, 0, 0, RELIEF_OUT_OF_RANGE, RELIEF_NO_PLANE, RELIEF_NO_PLANE]
    assert (rel["flags"] & (RELIEF_OUT_OF_RANGE | RELIEF_NO_PLANE)).tolist() == refused
    assert (foot["flags"] & (FOOTPRINT_OUT_OF_RANGE | FOOTPRINT_NO_PLANE)).tolist() == refused
    # the rule had something to decide: holes, (with a map) low and NaN confidences, a label's share
    assert rel["area"].tolist() == [H * W, 1, H * W, 0, H * W, H * W]
    assert 0 < rel["n"][2] < rel["n"][0] <= rel["n_valid"][0] < rel["n_masked"][0] == H * W
    assert rel["n_masked"][2] == int((labels == 1).sum())
