"""A filter call is told its stream and refuses before it launches: the class path leaves the
filter handle's stream binding alone, and a refused sdr_wls_filter_device writes nothing."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import FGS_PCR, FGS_THOMAS, lib  # noqa: E402
from stereo_depth_ruler_amd.ximgproc import createDisparityWLSFilter  # noqa: E402

from fgs_cases import bits, make_filter  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def test_class_path_leaves_the_filters_stream(oracle):
    """sdr_stereo_class_compute_device runs the filter on the matcher's stream; the handle's own
    binding is what it was, and the handle's next filter() is bit-exact."""
    h, w, D = 64, 160, 32
    gl, gr, _ = S.make_pair(h, w, D, seed=77)
    m = sdr.StereoSGBM.create(0, D, 5, 600, 2400, 1, 63, 12, 200, 2, sdr.MODE_SGBM_3WAY)
    rm = sdr.createRightMatcher(m)
    wls = createDisparityWLSFilter(m)
    wls.setLambda(8000.0)
    wls.setSigmaColor(1.1)
    L = lib()
    before = L.sdr_wls_get_stream(wls._h)
    assert before  # the handle's own stream
    dev = torch.device("cuda", 0)
    sl, sr = torch.from_numpy(gl[None]).to(dev), torch.from_numpy(gr[None]).to(dev)
    out = torch.empty((1, h, w), dtype=torch.float32, device=dev)
    filt = torch.empty((1, h, w), dtype=torch.int16, device=dev)
    assert L.sdr_sgbm_set_stream(m._h, None) == 0  # the class path's stream: not the filter's
    assert L.sdr_stereo_class_compute_device(m._h, rm._h, wls._h, sl.data_ptr(), sr.data_ptr(), w, h, 1,
                                             out.data_ptr(), filt.data_ptr(), None) == 0
    assert L.sdr_wls_get_stream(wls._h) == before
    torch.cuda.synchronize()
    ref_l = oracle.sgbm_compute(gl, gr, oracle.make_params(0, D, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    ref_r = oracle.sgbm_compute(gr, gl, oracle.make_params(-(D - 1), D, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    q = oracle.wls_params_for_sgbm(0, D, 5, w, h, 8000.0, 1.1)
    ref, ref_conf = oracle.wls_filter(ref_l, ref_r, gl, q, return_conf=True)
    assert np.array_equal(filt[0].cpu().numpy(), ref)
    got = wls.filter(ref_l, gl, ref_r)
    assert L.sdr_wls_get_stream(wls._h) == before
    assert np.array_equal(got, ref)
    assert np.array_equal(bits(wls.getConfidenceMap()), bits(ref_conf))
    for o in (m, rm, wls):
        o.close()


def test_refused_call_writes_nothing(oracle):
    """SDR_FGS_PCR on a ROI past 4096 columns: SDR_ERR_SIZE with the output and the confidence map
    untouched; the same handle on SDR_FGS_THOMAS then matches the oracle."""
    rng = np.random.default_rng(4)
    h, w = 6, 4200
    base = rng.integers(2, 40, (h, w // 8 + 1)) * 16
    dl = np.repeat(base, 8, 1)[:, :w].astype(np.int16)
    dr = -np.roll(dl, -2, 1)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    q = oracle.wls_params_for_sgbm(0, 32, 5, w, h, 8000.0, 1.1)
    f = make_filter(q, w, h)
    f.setFgsSolver(FGS_PCR)
    dev = torch.device("cuda", 0)
    ddl, ddr, dg = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (dl, dr, g))
    out = torch.full((h, w), 12345, dtype=torch.int16, device=dev)
    conf = torch.full((h, w), -7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = lib().sdr_wls_filter_device(f._h, ddl.data_ptr(), ddr.data_ptr(), dg.data_ptr(), w, h, w, w * h, 1,
                                     out.data_ptr(), conf.data_ptr())
    assert rc == -4  # SDR_ERR_SIZE
    assert ctypes.c_void_p(lib().sdr_wls_get_stream(f._h)).value
    torch.cuda.synchronize()
    assert bool((out == 12345).all()) and bool((conf == -7.5).all())
    f.setFgsSolver(FGS_THOMAS)
    ref, ref_conf = oracle.wls_filter(dl, dr, g, q, return_conf=True)
    got = f.filter(ddl, dg, ddr)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(bits(f.getConfidenceMap().cpu().numpy()), bits(ref_conf))
