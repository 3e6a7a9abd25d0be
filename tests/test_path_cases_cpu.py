"""The path-case table (tests/path_cases.py) without a GPU: the plan query names every case's
kernels and the table covers the whole enumeration, every input meets the conditions that make its
case worth running, the staged numpy reference agrees with the oracle, and wrong references
(mutations) differ from the right one on the cases that exist to catch them.

Which cases catch which mutation (asserted per case in test_reference_and_mutations):
  * last minimum instead of first on ties         -- every band case of H >= 37 (its flat bands)
  * the d +- 1 neighbour dropped at a lane boundary -- every band case of H >= 37, at the case's own DPL
  * the subpixel term applied at best = 0 or D - 1  -- every band case of H >= 37
  * a wrapping sum instead of the saturating one    -- every "binary" case
  * rows r and r + 768 of the output swapped        -- every case of 781 rows
  * the second column of the last odd pair written  -- every two-column case of W1 = 25, H >= 37
  * an overlap row of a 3WAY stripe output          -- the "stripes" cases
"""
import ctypes

import numpy as np
import pytest

import numpy_ref as N
import path_cases as P
from stereo_depth_ruler_amd._lib import SDRError, SgbmLaunches, lib, sgbm_plan

CUS = 256  # an MI355X; any non-zero value keeps the query off the GPU
ALL = P.CASES + P.natural_cases(CUS)
IDS = [c.name for c in ALL]


def plan_of(c, cus=CUS):
    return sgbm_plan(c.params(), c.W, c.H, c.F, cus=c.knob or cus)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_plan_names_the_expected_kernels(c):
    plan = plan_of(c)
    assert (plan["paths"], plan["south"]) == c.plan_key()
    assert plan["cost"] == (("generic", 0, 0, 1) if c.D > 256 else ("k_cost", c.bs, 2 if c.D > 128 else 1, 1))
    assert plan["post"] == "median3_lr" and plan["cus"] == (c.knob or CUS)
    nS = {P.WAY3: len(P.stripes(c.H, c.nstripes))}.get(c.mode, 1)
    if c.south[0] == "sweep":
        # eligible, its tiling unknown off the GPU; the paths launch keeps E and W
        assert plan["sweep_shape"] == ((0, 0), (0, 0))
        assert (plan["paths_chains"], plan["south_chains"]) == (2 * c.H * c.F, 0)
    else:
        assert plan["south_chains"] == nS * c.W1 * c.F
    if c.flip:
        other = sgbm_plan(c.params(), c.W, c.H, c.F, cus=c.flip)
        assert other["south"][4] != plan["south"][4], "the flipped knob reaches the other column form"


def test_table_covers_the_enumeration():
    """9 paths kernels, 33 fused-pass kernels and 4 sweep families, each named by some case."""
    assert {c.paths for c in ALL} == P.ALL_PATHS
    assert {c.south for c in ALL if c.south[0] == "k_south_wta"} == P.ALL_SOUTH
    assert {c.south for c in ALL if c.south[0] == "sweep"} == P.ALL_SWEEPS
    # the table's own rules: window reuse on every DPL 2 form and once per wider (DPL, PAD)
    tall = {c.south for c in ALL if c.H == P.TALL}
    assert {s for s in P.ALL_SOUTH if s[1] == 2} <= tall
    assert {(s[1], s[2]) for s in tall} == {(d, p) for d in (2, 4, 8) for p in (True, False)}
    assert {c.uniq_rule for c in ALL} == {1, 2}
    for fam in ("one", "r12", "tc", "sweep"):
        assert {c.minD for c in ALL if fam in c.name and "minD" in c.tags} == {-5, 3}, fam


def test_natural_thresholds_sit_on_both_sides():
    nat = {c.name: c for c in P.natural_cases(CUS)}
    for D in (16, 128):
        for np_ in (4, 3):
            big, small = nat[f"natural-D{D}-np{np_}-F8"], nat[f"natural-D{D}-np{np_}-F7"]
            assert big.W1 * 8 > 8 * CUS >= small.W1 * 7
            assert plan_of(big)["south"][4] and not plan_of(small)["south"][4]
            # one column at D = 128: 12-bit records, unless the E / W / N launch (MODE_HH4's 2H + W1
            # chains a frame against 4 x CUs) still takes two chains a wave
            assert plan_of(small)["south"][5] == (D == 128 and np_ == 4)
    hh4 = nat["natural-D128-np3-F8"]
    assert plan_of(hh4)["paths"][0] == "k_paths_tc" and plan_of(hh4, cus=4 * CUS)["paths"][0] == "k_paths"


def test_query_refusals_and_sweep_limit():
    c = P.BY_NAME["sweep-D272-chains"]
    assert plan_of(c)["south"][0] == "k_south_wta"  # past D = 256 a batch takes chains
    bad = P.BY_NAME["one-D16-np4"].params()
    bad.numDisparities = 17
    with pytest.raises(SDRError) as e:
        sgbm_plan(bad, 64, 8, cus=CUS)
    assert e.value.code == -2
    empty = sgbm_plan(P.BY_NAME["one-D16-np4"].params(), 10, 8, cus=CUS)  # W1 <= 0: no launch
    assert (empty["paths"], empty["south"], empty["post"]) == (("none",), ("none",), "none")


def test_record_layout_and_null_guards():
    """sdr_sgbm_launches is 26 int32; the handle entries refuse a null handle without a GPU."""
    assert ctypes.sizeof(SgbmLaunches) == 26 * 4
    out = SgbmLaunches()
    assert lib().sdr_sgbm_last_plan(None, ctypes.byref(out)) == -1
    assert lib().sdr_sgbm_plan_query(None, 0, 64, 8, 1, 1, 256, ctypes.byref(out)) == -1
    assert lib().sdr_sgbm_plan_query(ctypes.byref(P.CASES[0].params()), 0, 64, 8, 1, 1, -1, ctypes.byref(out)) == -1
    assert lib().sdr_sgbm_debug_knob(None, 2, 1) == -1


def _input_conditions(c, r):
    acc = r.acc
    if c.kind == "binary":
        assert (r.S.min(-1) >= 32767).any(), "no pixel with every S saturated: another seed"
        return
    if c.H < 37:
        assert acc.mean() >= 0.3
        return
    inv = (c.minD - 1) * 16
    assert acc.mean() >= 0.4 and (~acc).mean() >= 0.1
    assert ((r.raw != inv) & (r.lr == inv)).sum() >= 4, "LR-invalidated pixels"
    won = np.unique(r.best[acc])
    assert set((won // (c.D // 16)).tolist()) == set(range(16)), "accepted winners in all 16 lane groups"
    assert won[0] == 0 and won[-1] == c.D - 1


def _mutations(c, r):
    e = r.eff
    band = c.kind == "band" and c.H >= 37
    if band:
        # last minimum on ties: an accepted pixel whose minimum is attained twice
        last = c.D - 1 - r.S[..., ::-1].argmin(-1)
        assert (r.acc & (last != r.best)).any()
        # the subpixel term at the range's ends: non-zero there unless the inner neighbour ties
        lo = r.acc & (r.best == 0) & (r.S[..., 1] > r.S[..., 0])
        hi = r.acc & (r.best == c.D - 1) & (r.S[..., -2] > r.S[..., -1])
        assert lo.any() and hi.any()
        # a lane boundary of the chain wave (DPL disparities a lane) dropping its neighbour
        Cq = r.C[:48]
        assert np.array_equal(P.chain_E(Cq, e["P1"], e["P2"]), r.recs[:48, :, 0])
        assert not np.array_equal(P.chain_E(Cq, e["P1"], e["P2"], cut=c.paths[1]), r.recs[:48, :, 0])
    if c.kind == "binary":
        # a wrapping sum: recompute S from the records is not possible for the fused direction, so
        # from the volumes' definition -- the unsaturated sum passes 32767 somewhere
        tot = sum(N._path_volume(r.C.astype(np.int64), d[0], d[1], e["P1"], e["P2"]) for d in N.SGM_DIRS[c.mode])
        wrapped = ((tot + 32768) % 65536) - 32768
        assert not np.array_equal(N.wta_map(wrapped, e)[0], N.wta_map(r.S, e)[0])
    if c.H == P.TALL:
        m = c.minX1
        assert not np.array_equal(r.raw[:13, m:m + c.W1], r.raw[768:, m:m + c.W1])
    if c.south[4:5] == (True,) and c.W1 % 2 and c.H >= 37:
        # the odd last pair's second column, column W1: a phantom pixel copying column W1 - 1
        # would fold its key into the right view
        x = c.W1
        ok = r.acc[:, x - 1]
        minS = r.S.min(-1)[:, x - 1]
        x2 = x + c.minX1 - r.best[:, x - 1] - c.minD
        inside = ok & (x2 >= 0) & (x2 < c.W)
        key = (minS << 16) | (0xffff - x)
        rows = np.nonzero(inside)[0]
        assert (key[rows] < r.keys[rows, x2[rows]].astype(np.int64)).any()
    if "stripes" in c.tags:
        # each stripe also writing the overlap row before its first output row, after the stripe above
        L, R = P.frames(c)[0]
        segs = P.stripes(c.H, c.nstripes)
        assert len(segs) == 4 and all(out0 - 1 >= s0 for s0, _, out0 in segs[1:])
        early = P.staged(L, R, c, segs=[(s0, end, max(out0 - 1, 0)) for s0, end, out0 in segs])
        assert any(not np.array_equal(early.raw[out0 - 1], r.raw[out0 - 1]) for _, _, out0 in segs[1:])


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_reference_and_mutations(oracle, c):
    """Per case, on frame 0: the staged reference is the oracle's (cost volume and LR-checked
    map), the input conditions hold, and the mutations the case exists for differ."""
    L, R = P.frames(c)[0]
    r = P.reference(c)
    p = oracle.make_params(*c.args, **c.kwargs)
    assert np.array_equal(r.C, oracle.cost_volume(L, R, p))
    assert np.array_equal(r.lr, oracle.sgbm_compute(L, R, p, stages=0))
    _input_conditions(c, r)
    _mutations(c, r)


def test_band_pair_is_what_it_says():
    D, W1, H = 32, 24, 60
    L, R = P.band_pair(H, W1, D, seed=5)
    d = P.band_shifts(4 + D, D, 6)
    assert d[:4] == [0, D - 1, 1, D - 2] and sorted(d[4:]) == list(range(D))
    for k in (0, 1, 2, 3, 5):  # matched bands: left x = right x - d within the +-3 noise
        y = 3 * k
        a = L[y, D:].astype(int)
        b = R[y, D - d[k]:D - d[k] + a.size].astype(int)
        assert np.abs(a - b).max() <= 3, k
    assert (L[18:21] == 128).all() and np.abs(R[18:21].astype(int) - 128).max() <= 3  # band 6: flat + noise
    assert np.abs(L[12, D:].astype(int) - R[12, D - d[4]:D - d[4] + W1].astype(int)).max() > 3  # band 4: noise
