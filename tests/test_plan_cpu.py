"""The plan of a matcher call without a GPU (csrc/sdr_plan.hip through sdr_sgbm_scratch_bytes_ex):
the scratch formula and the MODE_SGBM_3WAY stripe layout restated here, and the stripe limits the
plan refuses as compute does."""
import ctypes
import itertools
import math

import pytest

from stereo_depth_ruler_amd import _lib

SGBM, HH, WAY3, HH4 = 0, 1, 2, 3
NPATHS = {SGBM: 5, HH: 8, WAY3: 3, HH4: 4}
MAX_PATH_DIRS, MAX_COST_AUX = 24, 16  # sdr_internal.hpp kMaxPathDirs, kMaxCostAux


def stripes_of(H, nstripes, bs, SH2):
    """SGBM3WayMainLoop's stripes as (s0, end, out0, aux_rows): chain rows [s0, end), output rows
    [out0, end), the stripe's first aux_rows cost rows in a band of their own."""
    sz = math.ceil(H / nstripes)
    overlap = (bs // 2 + 1) + math.ceil(0.1 * sz)
    out = []
    for s in range(nstripes):
        out0 = s * sz
        if out0 >= H:
            break
        s0 = max(min(s * sz - overlap, H), 0)
        end = min((s + 1) * sz, H)
        ylim = max(H - 1 - SH2, s0)
        aux = 0 if s0 == 0 else SH2 if ylim >= s0 + SH2 else end - s0
        out.append((s0, end, out0, aux))
    return out


def scratch_bytes(W, H, minD, D, bs, mode, nstripes, cn, F):
    """The formula test_scratch_bytes_unchanged_for_c2 spells out, with the channels on the
    operand planes, plus the 3WAY term stripes x max aux_rows x W1 x D x 2."""
    W1 = W + min(minD, 0) - max(minD + D, 0)
    px, cells = W * H, H * W1 * D
    aux = 0
    if mode == WAY3:
        st = stripes_of(H, nstripes, bs, bs // 2)
        aux = len(st) * max(s[3] for s in st) * W1 * D * 2
    return F * (3 * px * 4 * cn + 3 * px * 8 * cn + cells * 2 * NPATHS[mode] + aux + px * 2 * 3 + px * 4
                + px * 4 * 2)


def engine_bytes(W, H, minD, D, bs, mode, nstripes, cn, F):
    p = _lib.SgbmParams(minD, D, bs, 50, 300, 1, 31, 10, 0, 0, mode, nstripes, 0)
    return _lib.lib().sdr_sgbm_scratch_bytes_ex(ctypes.byref(p), 0, W, H, cn, F)


GRID = [(W, H, 0, D, 5, mode, ns, cn, F)
        for (W, H), D, mode, ns, cn, F in itertools.product(
            ((320, 100), (205, 37)), (64, 128), (SGBM, HH, WAY3, HH4), (1, 4, 7), (1, 3), (1, 2, 8))]
GRID += [(320, 100, -24, 64, 5, mode, 4, 1, 2) for mode in (SGBM, HH, WAY3, HH4)]  # minDisparity < 0


def test_scratch_bytes_follow_the_formula():
    bad = [(c, engine_bytes(*c), scratch_bytes(*c)) for c in GRID if engine_bytes(*c) != scratch_bytes(*c)]
    assert not bad, bad[:5]
    assert all(scratch_bytes(*c) > 0 for c in GRID)


def test_3way_term_counts():
    """The grid reaches stripes with and without rows of their own, and a frame with fewer
    stripes than asked for."""
    assert [s[3] for s in stripes_of(100, 4, 5, 2)] == [0, 2, 2, 2]
    assert len(stripes_of(37, 7, 5, 2)) == 7 and len(stripes_of(100, 1, 5, 2)) == 1
    assert len(stripes_of(100, 30, 3, 1)) == 25


# 320x100, D = 64, blockSize 3.  nstripes = 30: 25 stripes of 4 rows, more top-to-bottom
# directions than a path launch holds beside E and W (22).  nstripes = 20: 20 stripes of 5 rows fit
# the launch, but 19 of them start below row 0 and keep rows of their own, past the 16 extra row
# bands of the cost launch.
@pytest.mark.parametrize("nstripes,nst,naux", [(30, 25, 24), (20, 20, 19)])
def test_stripe_limits_refused_as_compute_refuses(nstripes, nst, naux):
    st = stripes_of(100, nstripes, 3, 1)
    assert (len(st), sum(1 for s in st if s[3])) == (nst, naux)
    assert (nst + 2 > MAX_PATH_DIRS) != (nst + 2 <= MAX_PATH_DIRS and naux > MAX_COST_AUX)
    L = _lib.lib()
    assert engine_bytes(320, 100, 0, 64, 3, WAY3, 4, 1, 1) > 0
    assert engine_bytes(320, 100, 0, 64, 3, WAY3, nstripes, 1, 1) == 0
    assert b"too many 3WAY stripes" in L.sdr_last_error()
    # the other modes ignore nstripes
    assert engine_bytes(320, 100, 0, 64, 3, SGBM, nstripes, 1, 1) > 0
