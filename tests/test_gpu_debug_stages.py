"""sdr_sgbm_debug_stage follows the handle's last call: the slack, the record layout and the LR
rule it reads its buffers with are that call's plan, whatever the calls before it were."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402

H, W, D = 40, 192, 128
W1 = W - D


def args_of(d12, mode=0):
    return (0, D, 5, 600, 2400, d12, 63, 12, 0, 0, mode)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def stages_0_4(m):
    # stage 4 up to the 12-bit records' size: inside the buffer under either record format
    return m.debug_stage(0, (H, W1, D), np.int16), m.debug_stage(4, (H, W1, 4, D * 3 // 4), np.int16)


def test_debug_stages_follow_the_last_call(oracle):
    L, R = S.make_pair(H, W, D, seed=11)[:2]
    want = {}
    for d12 in (1, 128):  # 128 >= D: the LR check is skipped, stage 2 is rebuilt from the WTA map
        f = sdr.StereoSGBM.create(*args_of(d12))
        f.compute(L, R)
        want[d12] = (oracle.sgbm_compute(L, R, oracle.make_params(*args_of(d12)), stages=0),) + stages_0_4(f)
        f.close()
    assert not np.array_equal(want[1][0], want[128][0])
    m = sdr.StereoSGBM.create(*args_of(1))
    for d12 in (1, 128, 1):
        m.setDisp12MaxDiff(d12)
        m.compute(L, R)
        assert np.array_equal(m.debug_stage(2, (H, W), np.int16), want[d12][0]), d12
        c, l = stages_0_4(m)
        assert np.array_equal(c, want[d12][1]) and np.array_equal(l, want[d12][2]), d12

    # then a 3WAY call of another shape: stage 6, the stripe-start rows.  Stripe 0 starts at row 0
    # and keeps none (its band is never written); stripes 1..3 keep SH2 = 2 rows each
    H3, W3 = 100, 320
    L3, R3 = S.make_pair(H3, W3, D, seed=12)[:2]
    band = (4, 2, W3 - D, D)
    f = sdr.StereoSGBM.create(*args_of(1, mode=2), nstripes=4)
    f.compute(L3, R3)
    ref6 = f.debug_stage(6, band, np.int16)
    f.close()
    m.setMode(2)
    m.compute(L3, R3)
    assert np.array_equal(m.debug_stage(6, band, np.int16)[1:], ref6[1:]) and ref6[1:].any()
    m.close()
