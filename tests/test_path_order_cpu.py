"""The order of the path-cost records as the plan picks it, without a GPU (sdr_sgbm_records_query
beside sdr_sgbm_plan_query, both at a given compute-unit count): by column unless
SDR_PATH_ORDER=row, but only where the fused pass is the one-column k_south_wta fed by one-chain
k_paths without 3WAY stripes; the strides of either order; and the buffer's slack against what the
fused pass's whole-block loads reach past a frame."""
import os
from contextlib import contextmanager

import pytest

from stereo_depth_ruler_amd import _lib

SGBM, HH, WAY3, HH4 = 0, 1, 2, 3
NREC = {SGBM: 4, HH: 7, WAY3: 2, HH4: 3}
RB, PAD_ROWS = 12, 64          # kSouthRB, kSouthPad
ONE, TC = 1 << 20, 1           # compute units that keep a frame off / send it to the two-column kernels


@contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def query(mode, D, H, W1, F=1, cus=ONE, order="col", rec=None, P2=120, nstripes=4):
    p = _lib.SgbmParams(0, D, 3, 20, P2, 1, 63, 10, 0, 0, mode, nstripes, 0)
    with environment(SDR_PATH_ORDER=order, SDR_PATH_REC=rec):
        return _lib.sgbm_plan(p, W1 + D, H, F, cus=cus), _lib.sgbm_records(p, W1 + D, H, F, cus=cus)


def expect(r, order, nrec, pix, H, W1, D):
    assert (r["order"], r["nrec"], r["pix"]) == (order, nrec, pix)
    assert (r["xs"], r["ys"]) == ((H * pix, pix) if order == "col" else (pix, W1 * pix))
    assert r["frame"] == nrec * H * W1 * D
    assert r["slack"] == PAD_ROWS * W1 * D * nrec


SHAPES = [(H, W1) for H in (1, 11, 12, 13, 25, 37, 720) for W1 in (2, 5, 24, 1152)]


@pytest.mark.parametrize("mode", (SGBM, HH, HH4))
@pytest.mark.parametrize("D", (16, 64, 128, 256, 512))
def test_one_column_route_takes_column_order(mode, D):
    nrec = NREC[mode]
    for H, W1 in SHAPES:
        for rec in (None, "16"):
            plan, r = query(mode, D, H, W1, rec=rec)
            r12 = D == 128 and rec is None
            assert plan["paths"][0] == "k_paths" and plan["south"][0] == "k_south_wta" and not plan["south"][4]
            assert (plan["paths"][3], plan["south"][5], r["r12"]) == (r12, r12, r12)
            pix = nrec * D * (3 if r12 else 4) // 4
            expect(r, "col", nrec, pix, H, W1, D)
            rows = -(-H // RB) * RB
            assert r["reach"] == (W1 - 1) * r["xs"] + (rows - 1) * r["ys"] + pix
            # past the last frame's span: at most RB - 1 records, inside the slack
            assert r["reach"] - r["frame"] <= (RB - 1) * pix <= r["slack"]
            _, rr = query(mode, D, H, W1, rec=rec, order="row")
            expect(rr, "row", nrec, pix, H, W1, D)
            assert rr["reach"] == (rows - 1) * rr["ys"] + W1 * pix
            assert rr["reach"] - rr["frame"] <= (RB - 1) * W1 * pix <= rr["slack"]


def test_column_order_is_the_default():
    """Only SDR_PATH_ORDER=row keeps an eligible call by row."""
    for order in (None, "", "col", "column", "ROW", "1"):
        _, r = query(SGBM, 128, 37, 24, order=order)
        assert r["order"] == "col", order
    assert query(SGBM, 128, 37, 24, order="row")[1]["order"] == "row"


@pytest.mark.parametrize("D", (64, 128))
def test_other_routes_keep_row_order(D):
    H, W1 = 37, 25
    # two columns a workgroup (and, MODE_HH4, two chains a wave); int16 records
    for mode in (SGBM, HH4):
        plan, r = query(mode, D, H, W1, cus=TC)
        assert plan["south"][4] and not r["r12"]
        expect(r, "row", NREC[mode], NREC[mode] * D, H, W1, D)
        # the second column of an odd W1's last pair: one record past the row
        assert r["reach"] == (-(-H // RB) * RB - 1) * r["ys"] + (W1 + 1) * r["pix"]
        assert r["reach"] - r["frame"] <= r["slack"]
    # two chains a wave feeding the one-column fused pass: 2H + W1 = 99 chains against 4 x 20 CUs,
    # W1 = 25 columns against 8 x 20
    plan, r = query(HH4, D, H, W1, cus=20)
    assert plan["paths"][0] == "k_paths_tc" and not plan["south"][4]
    expect(r, "row", 3, 3 * D, H, W1, D)
    # MODE_SGBM_3WAY on the one-column kernel: stripes
    plan, r = query(WAY3, D, H, W1)
    assert not plan["south"][4]
    expect(r, "row", 2, 2 * D, H, W1, D)
    assert r["reach"] - r["frame"] <= r["slack"]
    # a batch that sweeps: E, W and the up record, no fused pass
    plan, r = query(HH, D, 13, 41, F=8)
    assert plan["south"][0] == "sweep"
    expect(r, "row", 3, 3 * D, 13, 41, D)
    assert r["reach"] == 0


def test_tall_frame_keeps_row_order():
    """k_paths re-bases its store resource every 32 steps and carries the steps between in a 32-bit
    offset below 2^31: 32 diagonal steps of (H + 1) * pix * 2 bytes by column."""
    D, W1 = 128, 2
    pix = 7 * D  # MODE_HH, int16 records
    fits = (2 ** 31 - 1 - 2 * pix) // (32 * 2 * pix) - 1
    for H, order in ((fits, "col"), (fits + 1, "row")):
        _, r = query(HH, D, H, W1, rec="16")
        expect(r, order, 7, pix, H, W1, D)
        assert 32 * (r["xs"] + r["ys"]) * 2 + 2 * pix < 2 ** 31


def test_empty_frame_reports_nothing():
    p = _lib.SgbmParams(0, 128, 3, 20, 120, 1, 63, 10, 0, 0, SGBM, 4, 0)
    r = _lib.sgbm_records(p, 100, 20, cus=ONE)  # W1 <= 0
    assert (r["order"], r["pix"], r["frame"], r["reach"]) == ("row", 0, 0, 0)
