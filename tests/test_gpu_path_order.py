"""The path-cost records by column and by row (SDR_PATH_ORDER=col|row when the handle is created;
sdr.h, sdr_sgbm_records): the same maps and -- through sdr_sgbm_debug_stage(4), which keeps its
documented row layout -- the same records, bit for bit, against tests/path_cases.py's staged
reference and against each other.

D = 128 in both record formats (12-bit, and int16 under SDR_PATH_REC=16), MODE_SGBM, MODE_HH4 and
unbatched MODE_HH (the fused pass reads 4, 3 and 7 directions), heights around the fused pass's
12-row blocks (1, 11, 12, 13, 25, 37), 1, 2 and 5 matched columns, one frame and two different ones.
The calls that keep row order whatever the environment says -- the two-column kernel (D = 64 under
the 1-CU knob), MODE_SGBM_3WAY and a batch that sweeps -- say so and compute what they computed.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import path_cases as P
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd.sgbm import DEBUG_PLAN_CUS

D = 128
RB = 12  # kSouthRB: rows of a block of the fused pass
HEIGHTS = (1, 11, 12, 13, 25, 37)
W1S = (1, 2, 5)
MODES = (P.SGBM, P.HH4, P.HH)


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@contextmanager
def environment(**kw):
    """The named variables set (None: unset) for the block, then put back."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def create(c, order, rec16=False):
    with environment(SDR_PATH_ORDER=order, SDR_PATH_REC="16" if rec16 else None):
        return sdr.StereoSGBM.create(*c.args, **c.kwargs)


def run(torch, m, c, F, knob=P.KNOB_ONE):
    """The case's first F frames on handle m -> (plan, records, {stage: array of all frames})."""
    m.set_debug_knob(DEBUG_PLAN_CUS, knob)
    fr = P.frames(c)[:F]
    Ld = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    Rd = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    out = m.compute(Ld, Rd)
    torch.cuda.synchronize()
    plan, recs = m.last_plan(), m.last_records()
    H, W, W1 = c.H, c.W, c.W1
    got = {"final": out.cpu().numpy(), 0: m.debug_stage(0, (F, H, W1, c.D), np.int16),
           1: m.debug_stage(1, (F, H, W), np.int16), 2: m.debug_stage(2, (F, H, W), np.int16),
           5: m.debug_stage(5, (F, H, W), np.uint32),
           4: m.debug_stage(4, (F, H, W1, recs["nrec"], c.D), np.int16)}
    return plan, recs, got


def used(c, recs, rec4):
    """The part of a frame's stage 4 span the records fill (12-bit: its first 3/4), all frames."""
    n = c.H * c.W1 * recs["pix"]
    assert recs["pix"] == recs["nrec"] * c.D * (3 if recs["r12"] else 4) // 4
    return rec4.reshape(rec4.shape[0], -1)[:, :n]


def path_costs(c, recs, got, f):
    """Frame f's stage 4 as path costs [H][W1][R][D]."""
    if not recs["r12"]:
        return got[4][f]
    e = P.decode_rec12(used(c, recs, got[4])[f].view(np.uint32), c.H, c.W1, recs["nrec"], c.D)
    assert 0 <= e.min() and e.max() <= c.P2
    return (got[0][f].astype(np.int64)[:, :, None, :] - e).astype(np.int16)


def check_frame(oracle, c, recs, got, f, ref, what):
    """Frame f of a run: stages 4, 1, 5 and 2 against the staged reference, the final map against
    the oracle (the staged reference ends at the LR-checked map)."""
    L, R = P.frames(c)[f]
    m0 = c.minX1
    what = f"{c.name} {what} frame {f}"
    assert np.array_equal(got[0][f], ref.C), f"{what}: stage 0"
    L4 = path_costs(c, recs, got, f)
    assert L4.shape == ref.recs.shape
    bad = L4 != ref.recs
    assert not bad.any(), f"{what}: stage 4: {bad.sum()} values differ, first at (y, x, q, d) = {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(got[1][f][:, m0:m0 + c.W1], ref.raw[:, m0:m0 + c.W1]), f"{what}: stage 1"
    assert np.array_equal(got[5][f], ref.keys), f"{what}: stage 5"
    assert np.array_equal(got[2][f], ref.lr), f"{what}: stage 2"
    p = oracle.make_params(*c.args, **c.kwargs)
    assert np.array_equal(got["final"][f], oracle.sgbm_compute(L, R, p)), f"{what}: final map"


def same_run(c, recs, a, b, what):
    m0 = c.minX1
    assert np.array_equal(used(c, recs, a[4]), used(c, recs, b[4])), f"{c.name}: stage 4 {what}"
    assert np.array_equal(a[1][:, :, m0:m0 + c.W1], b[1][:, :, m0:m0 + c.W1]), f"{c.name}: stage 1 {what}"
    for k in (0, 5, 2, "final"):
        assert np.array_equal(a[k], b[k]), f"{c.name}: stage {k} {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("W1", W1S)
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("mode", MODES, ids=["sgbm", "hh4", "hh"])
def test_orders_agree(gpu, oracle, mode, H, W1):
    np_ = P.NP_OF[mode]
    # blockSize 1 where one matched column would be narrower than the block's half width
    c = P.Case(f"order-np{np_}-h{H}-w{W1}", mode, D, H, W1, None, None, F=2, bs=1 if W1 == 1 else P.BS,
               seed=7000 + 100 * np_ + 10 * H + W1)
    refs = [P.staged(L, R, c) for L, R in P.frames(c)]
    for rec16 in (False, True):
        runs = {}
        for order in ("col", "row"):
            m = create(c, order, rec16)
            for F in (1, 2):
                plan, recs, got = run(gpu, m, c, F)
                what = f"{order} rec16={rec16} F={F}"
                assert plan["paths"] == ("k_paths", 2, False, not rec16), what
                assert plan["south"] == ("k_south_wta", 2, False, np_, False, not rec16), what
                pix = np_ * D * (4 if rec16 else 3) // 4
                want = (pix * H, pix) if order == "col" else (pix, pix * W1)
                assert (recs["order"], recs["r12"], recs["nrec"], recs["pix"], recs["xs"], recs["ys"]) == \
                       (order, not rec16, np_, pix) + want, what
                assert recs["frame"] == np_ * H * W1 * D, what
                # a last partial block reads whole: up to RB - 1 records past the column's (frame's) end
                rows = -(-H // RB) * RB
                assert recs["reach"] == (W1 - 1) * recs["xs"] + (rows - 1) * recs["ys"] + pix, what
                assert recs["reach"] - recs["frame"] <= recs["slack"], what
                for f in range(F):
                    check_frame(oracle, c, recs, got, f, refs[f], what)
                runs[order, F] = (recs, got)
            m.close()
        for F in (1, 2):
            same_run(c, runs["row", F][0], runs["col", F][1], runs["row", F][1], f"rec16={rec16} F={F}: col against row")


def row_order_case(gpu, oracle, c, knob, sweep=False):
    """A call that keeps its records by row under SDR_PATH_ORDER=col: it says so, and computes what
    the staged reference and a handle created under SDR_PATH_ORDER=row compute."""
    runs = {}
    for order in ("col", "row"):
        m = create(c, order)
        plan, recs, got = run(gpu, m, c, c.F, knob)
        assert (plan["paths"], plan["south"]) == c.plan_key(), order
        pix = recs["nrec"] * c.D
        assert (recs["order"], recs["r12"], recs["pix"], recs["xs"], recs["ys"]) == ("row", False, pix, pix, pix * c.W1), order
        assert recs["reach"] - recs["frame"] <= recs["slack"], order
        check_frame(oracle, c, recs, got, 0, P.staged(*P.frames(c)[0], c, sweep=sweep), order)
        runs[order] = (recs, got)
        m.close()
    same_run(c, runs["row"][0], runs["col"][1], runs["row"][1], "col against row")


@pytest.mark.gpu
def test_two_column_kernel_keeps_row_order(gpu, oracle):
    """D = 64 (PAD, int16 records) under the 1-CU knob: two columns a workgroup."""
    c = P.Case("order-tc-D64", P.SGBM, 64, 37, 25, P._paths(2, True), P._south(2, True, 4, tc=True), seed=7901)
    row_order_case(gpu, oracle, c, P.KNOB_TC)


@pytest.mark.gpu
def test_3way_keeps_row_order(gpu, oracle):
    """Four stripes of a D = 128 frame on the one-column kernel: stripes, so by row."""
    c = P.Case("order-3way", P.WAY3, D, 37, 24, P._paths(2, False), P._south(2, False, 2), nstripes=4, seed=7902)
    row_order_case(gpu, oracle, c, P.KNOB_ONE)


@pytest.mark.gpu
def test_sweep_keeps_row_order(gpu, oracle):
    """Batched MODE_HH: E, W and the up record, by row."""
    c = P.BY_NAME["sweep-D128-w41"]
    row_order_case(gpu, oracle, c, 0, sweep=True)
