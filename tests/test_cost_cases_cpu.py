"""The BT cost edge cases (cost_cases.py) without a GPU: every entry reaches what its name says (the
instantiation by sdr_sgbm_plan_query, the classes by the kernels' own conditions restated), the
tables cover every class, the pin agrees with the C oracle, a plain loop and a closed form, and --
so that a passing GPU test means something -- deliberately wrong references that each group of
cases must tell from the pin."""
import ctypes

import numpy as np
import pytest

import cost_cases as C
import numpy_ref as N
from numpy_ref import SGM_3WAY, SGM_HH, SGM_HH4, SGM_SGBM
from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd._lib import SDRError, sgbm_plan
from test_plan_cpu import stripes_of

CUS = 256  # any non-zero value keeps a plan query off the GPU


def params_of(c, mode=None):
    return _lib.SgbmParams(*C.create_args(c, mode), c.ns, 0)


def plan_of(c, mode=None):
    return sgbm_plan(params_of(c, mode), c.W, c.H, c.F, c.cn, cus=CUS)


# ---- the instantiations the ABI reaches ---------------------------------------------------

def test_blocksize_11_with_three_channels_is_refused_everywhere():
    """2*P2 + 3*(min(2*ftzero, 255) + 63)*121 > 32767 at the smallest P2 and every preFilterCap, in
    every mode: k_cost<11, K, 3> cannot be reached, so it is not compiled.  blockSize 9 is."""
    for mode in C.MODES:
        for cap in C.CAPS + (0,):
            for D in (16, 144):
                assert C.p2_max(11, cap, 3) < 2
                p = _lib.SgbmParams(0, D, 11, 1, 2, 1, cap, 10, 0, 0, mode, 4, 0)
                with pytest.raises(SDRError) as e:
                    sgbm_plan(p, D + 40, 30, 1, 3, cus=CUS)
                assert e.value.code == -8 and "int16" in str(e.value)
                if cap <= 63:  # (one channel passes the domain at blockSize 11 from cap 127 on)
                    assert sgbm_plan(p, D + 40, 30, 1, 1, cus=CUS)["cost"] == ("k_cost", 11, 1 if D == 16 else 2, 1)
            p = _lib.SgbmParams(0, 16, 9, 1, 2, 1, 15, 10, 0, 0, mode, 4, 0)
            assert sgbm_plan(p, 56, 30, 1, 3, cus=CUS)["cost"] == ("k_cost", 9, 1, 3)
    # past blockSize 11 the colour block term leaves the domain too: the generic path sees colour
    # only through D > 256
    assert all(C.p2_max(bs, 15, 3) < 2 for bs in (11, 13, 15, 17))


def test_plan_query_reports_no_band():
    out = plan_of(C.COST_CASES[0])
    assert (out["cost_rows"], out["cost_bands"]) == (0, 0)


# ---- every entry reaches what its name says -----------------------------------------------

@pytest.mark.parametrize("c", C.COST_CASES + C.STRIPE_CASES, ids=lambda c: c.id)
def test_entry_reaches_its_instantiation(c):
    assert c.W1 == c.W + min(c.minD, 0) - max(c.minD + c.D, 0) >= c.bs // 2 + 1
    assert c.H <= 80 and c.W <= 660 and c.H * c.W1 * c.D <= 80 * 320 * 16, c.id
    assert 1 <= c.P1 < c.P2 <= C.p2_max(c.bs, c.cap, c.cn)
    for mode in (c.mode, C.other_hh_mode(c.mode)):
        assert plan_of(c, mode)["cost"] == C.kernel_of(c.bs, c.D, c.cn), mode
    name = c.name
    if name.startswith("k_"):
        nr, k, cn = (int(v) for v in name.split("__")[0].split("_")[1:4])
        assert C.kernel_of(c.bs, c.D, c.cn) == ("k_cost", nr, k, cn)
        if "__W1_" in name:
            assert C.w1_class(c) == name.split("__W1_")[1].split("__")[0]
            assert f"__D{c.D}" in name
    if "cn3" in name:
        assert c.cn == 3
    if "P2max" in name:
        assert c.P2 == C.p2_max(c.bs, c.cap, c.cn)
    if name.startswith("generic"):
        assert C.kernel_of(c.bs, c.D, c.cn)[0] == "generic"


def block_split(c):
    """(EDGE, interior) column blocks by k_cost's own condition."""
    b, s = C.bcols_of(c.D), c.bs // 2
    nb = (c.W1 + b - 1) // b
    interior = [bx for bx in range(nb) if bx * b - s >= 0 and bx * b + b + s <= c.W1]
    return [bx for bx in range(nb) if bx not in interior], interior


def test_instantiation_entries_cover_every_kernel_width_and_range_class():
    inst = [c for c in C.COST_CASES if "instantiation" in c.tags]
    assert [C.kernel_of(c.bs, c.D, c.cn) for c in inst] == [("k_cost",) + i for i in C.INSTANTIATIONS]
    assert len(C.INSTANTIATIONS) == 22 and len({c.id for c in C.COST_CASES + C.STRIPE_CASES}) == \
        len(C.COST_CASES + C.STRIPE_CASES)
    assert {c.mode for c in inst} == set(C.MODES)
    for k in (1, 2):
        mine = [c for c in inst if C.kernel_of(c.bs, c.D)[2] == k]
        assert {C.w1_class(c) for c in mine} == set(C.W1_CLASSES), k
        assert {c.D for c in mine} == set(C.D_CLASSES[k]), k
        for cn in (1, 3):
            assert {c.D for c in mine if c.cn == cn} == set(C.D_CLASSES[k]), (k, cn)
        for c in mine:
            edge, interior = block_split(c)
            if C.w1_class(c) == "3bcols+5":
                assert interior and 1 in interior and len(edge) + len(interior) == 4, c.id
            elif c.bs > 1:
                assert not interior, c.id
    # lanes past the last pair alias it: 56 of 64 at D = 16, 32 at D = 64, none at D = 128; in the
    # second word lanes 8..63 at D = 144, none at D = 256
    assert [64 - min(64, D // 2) for D in C.D_CLASSES[1]] == [56, 32, 0]
    assert [128 - D // 2 for D in C.D_CLASSES[2]] == [56, 0]
    # the dynamic LDS of the colour K = 2 launches passes 64 KiB from NR = 3 at D = 256
    lds = [c for c in C.COST_CASES if "lds" in c.tags]
    assert {(c.bs, c.D, c.cn) for c in lds} == {(nr, 256, 3) for nr in (3, 5, 7, 9)}
    for c in lds:
        assert lds_bytes(c.bs, 2, 3, c.D) > 65536, c.id
    assert lds_bytes(3, 2, 3, 256) == 66176 and lds_bytes(1, 2, 3, 256) < 65536
    assert max(lds_bytes(nr, k, cn, 128 * k) for nr, k, cn in C.INSTANTIATIONS) <= 160 * 1024


def lds_bytes(nr, k, cn, D):
    """CostCfg<NR, K, CN>::lds_bytes restated."""
    bcols = 32 if k == 1 else 16
    nlv = 4 * ((bcols + nr - 1 + 3) // 4)
    half = ((nlv + D + 1) // 2 + 7) // 16 * 16 + 8
    return 2 * 6 * cn * half * 8 + 2 * nlv * 16 * cn + 2 * nlv * k * 64 * 4


def test_band_entries_reach_their_class_and_cover_every_class():
    assert {(c.bs, C.kernel_of(c.bs, c.D)[2]) for c in C.BAND_CASES if c.cn == 1} == set(C.BAND_KERNELS)
    assert {(5, 2), (11, 2)} <= set(C.BAND_KERNELS) and {nr for nr, k in C.BAND_KERNELS} == set(C.BLOCK_SIZES)
    seen = {}
    for c in C.BAND_CASES:
        cls = c.tags[1]
        assert c.name.startswith(f"band_{cls}__") and c.ty >= 1 and c.H <= 80
        bands = C.bands_of(c)
        assert [b[:2] for b in bands] == [(y, min(y + c.ty, c.H)) for y in range(0, c.H, c.ty)]
        assert any(cls in b[4] for b in bands), (c.id, bands)
        # (trips, tail) of every band by the formula: n = tlast - tfirst + 1 + 2 SH2 rows, U = 2 NR
        s, U, ylim = c.bs // 2, 2 * c.bs, max(c.H - 1 - c.bs // 2, 0)
        for ty0, ty1, trips, tail, _ in bands:
            yl = max(ty0, min(ty1, max(1, c.H - s))) if C.is_hh(c.mode) else ty1
            if yl <= ty0:
                assert trips is None
                continue
            n = min(yl - 1, ylim) - min(ty0, ylim) + 1 + 2 * s
            assert (trips, tail) == divmod(n, U) and n <= c.ty + 2 * s
        if c.cn == 1:
            seen.setdefault((c.bs, C.kernel_of(c.bs, c.D)[2]), set()).add(cls)
        # the launcher's own rule gives a small frame 4-row bands: no full trip from NR = 5 on
        if c.bs >= 5:
            assert all(b[2] in (0, None) for b in C.bands_of(c, ty=4)), c.id
    for (nr, k), classes in seen.items():
        assert classes == set(C.BAND_CLASSES_BS1 if nr == 1 else C.BAND_CLASSES), (nr, k)
    # at least three full trips for NR = 5..11 on frames under 100 rows
    for nr in (5, 7, 9, 11):
        assert any(b[2] >= 3 for c in C.BAND_CASES if c.bs == nr for b in C.bands_of(c))
    # blockSize 1 has neither frozen nor P2 rows
    c1 = [c for c in C.BAND_CASES if c.bs == 1]
    for c in c1:
        for mode in C.MODES:
            assert not any(b[4] & {"straddles_ylim", "frozen", "hh_straddles_yl", "hh_p2_only"}
                           for b in C.bands_of(c, mode)), c.id


def test_edge_entries_cover_every_class():
    cases = C.COST_CASES
    for bs in (7, 11):
        hs = [c for c in cases if "height" in c.tags and c.bs == bs]
        assert [c.H for c in hs] == [C.h_of(k, bs) for k in C.H_CLASSES] and [c.tags[1] for c in hs] == list(C.H_CLASSES)
    mind = [c for c in cases if "minD" in c.tags]
    assert {c.minD for c in mind} >= {3, -20} and any(c.minD + c.D < 0 for c in mind)
    assert {C.kernel_of(c.bs, c.D)[2] for c in mind if c.minD == -20} == {1, 2}
    # the staging clamp acts: some staged right column falls left of 0 and some right of W - 1
    for c in mind:
        xr_lo = max(c.minD + c.D, 0) - c.bs // 2 - c.minD - (c.D - 1)
        xr_hi = max(c.minD + c.D, 0) + c.W1 - 1 + c.bs // 2 - c.minD
        assert xr_lo < 0 or xr_hi > c.W - 1, c.id
    assert any(max(c.minD + c.D, 0) + c.W1 - 1 + c.bs // 2 - c.minD > c.W - 1 for c in mind)
    caps = [c for c in cases if "cap" in c.tags]
    assert [c.cap for c in caps] == list(C.CAPS) and {c.cn for c in caps} == {1, 3}
    for c in caps:
        assert c.kind == "binary" and c.P2 == C.p2_max(c.bs, c.cap, c.cn)
        assert 2 * c.P2 + c.cn * (min(2 * C.ftzero_of(c.cap), 255) + 63) * c.bs ** 2 <= 32767 < \
            2 * (c.P2 + 1) + c.cn * (min(2 * C.ftzero_of(c.cap), 255) + 63) * c.bs ** 2
        with pytest.raises(SDRError):
            p = params_of(c)
            p.P2 += 1
            sgbm_plan(p, c.W, c.H, 1, c.cn, cus=CUS)
    assert [C.ftzero_of(cap) & 0xff for cap in C.CAPS] == [15, 63, 127, 129, 255, 233]
    kinds = [c for c in cases if "kind" in c.tags]
    assert {(c.kind, c.cn) for c in kinds} >= {(k, cn) for k in C.KINDS for cn in (1, 3)}
    batches = [c for c in cases if "batch" in c.tags and "generic" not in c.tags]
    assert {(C.kernel_of(c.bs, c.D)[2], c.cn, c.F) for c in batches} == {(k, cn, 3) for k in (1, 2) for cn in (1, 3)}


def test_generic_entries_cover_every_class():
    g = [c for c in C.COST_CASES if "generic" in c.tags]
    assert {c.bs for c in g if c.bs > 11} == {13, 15, 17}
    assert all(c.cn == 1 and c.cap == 15 for c in g if c.bs > 11)
    for cn in (1, 3):
        assert {c.D for c in g if c.D > 256 and c.cn == cn} == {272, 320, 512}, cn
    assert {c.W1 for c in g} >= {63, 64, 65, 129} and {c.H for c in g} >= {31, 32, 33, 65}
    assert C.HSUM_STRIP == 64 and C.VSUM_CHUNK == 32
    assert {(c.W1 + 63) // 64 for c in g} >= {1, 2, 3} and {(c.H + 31) // 32 for c in g} >= {1, 2, 3}
    c = C.COST_BY_ID["generic_bs13__hh_yl_on_chunk"]
    assert C.is_hh(c.mode) and (c.H - c.bs // 2) % C.VSUM_CHUNK == 0 and c.H > c.H - c.bs // 2 >= 1
    c = C.COST_BY_ID["generic_bs15__D48_24pairs"]
    assert c.D // 2 == 24 and 256 % (c.D // 2) != 0
    assert any(c.F == 3 for c in g) and any(C.kernel_of(c.bs, c.D)[0] == "generic" for c in C.STRIPE_CASES)
    assert any(c.minD < 0 for c in g)


def test_stripe_table_covers_what_it_claims():
    cases = C.STRIPE_CASES
    assert {c.ns for c in cases} == {1, 3, 4, 8} and {c.cn for c in cases} == {1, 3}
    short = full = 0
    for c in cases:
        st = stripes_of(c.H, c.ns, c.bs, c.bs // 2)
        short += sum(1 for s0, end, out0, aux in st if aux and aux == end - s0 and aux != c.bs // 2)
        full += sum(1 for s0, end, out0, aux in st if aux == c.bs // 2 and aux != end - s0)
    assert short >= 8 and full >= 8
    for bs in (7, 9, 11):
        assert any(aux and aux == end - s0 for c in cases if c.bs == bs
                   for s0, end, out0, aux in stripes_of(c.H, c.ns, c.bs, c.bs // 2)), bs
    kern = {C.kernel_of(c.bs, c.D, c.cn) for c in cases}
    assert {(k[0], k[2], k[3]) for k in kern} >= {("k_cost", 1, 1), ("k_cost", 2, 1), ("k_cost", 1, 3),
                                                  ("k_cost", 2, 3), ("generic", 0, 1)}
    assert any(c.bs == 1 for c in cases)


def test_prefilter_table_covers_what_it_claims():
    shapes = C.PREFILTER_SHAPES
    assert len({s[0] for s in shapes}) == len(shapes)
    for cn in (1, 3):
        assert {s[2] for s in shapes if s[3] == cn} == C.PREFILTER_WIDTHS[cn]
        assert {s[1] for s in shapes if s[3] == cn} >= {1, 2, 3, 8}
    assert {s[1] for s in shapes} == C.PREFILTER_HEIGHTS and {s[5] for s in shapes} == set(C.CAPS)
    reached = set()
    for name, H, W, cn, layout, cap in shapes:
        F, stride, fstride, offL, offR, nbytes = C.transform_layout(H, W * cn, layout)
        assert stride >= W * cn and fstride >= H * stride and offR >= offL + F * fstride
        p = _lib.SgbmParams(0, 16, 1, 1, 2, 1, cap, 12, 0, 0, 0, 4, 0)
        assert sgbm_plan(p, W, H, F, cn, cus=CUS)["cost"] == ("k_cost", 1, 1, cn), name
        dword = [C.takes_dword_path(W, cn, stride, fstride, off & 3) for off in (offL, offR)]
        assert dword[0] == dword[1], name
        why = "dword" if dword[0] else "odd" if (W * cn) & 3 else "stride" if stride & 3 else \
            "base" if offL & 3 else "fstride"
        if why == "base":
            assert {offL & 3, offR & 3} == {1, 3}
        reached.add((why, cn, F > 1))
        assert name.startswith({"dword": ("dword", "batch_260"), "odd": ("odd", "batch_17"), "stride": "stride",
                                "base": "base1", "fstride": "batch"}[why]), (name, why)
        assert ("cn3" in name) == (cn == 3)
    assert reached >= {(w, cn, False) for w in ("dword", "odd", "stride", "base") for cn in (1, 3)} | \
        {("fstride", 1, True), ("fstride", 3, True), ("dword", 1, True), ("odd", 1, True)}
    # the row loop's trips at 256 columns a trip, and both row strides
    assert {1 + (s[2] - 1) // 256 for s in shapes} >= {1, 2, 4}
    assert {s[4][1] for s in shapes if isinstance(s[4], tuple) and s[4][0] == "stride"} == {1, 7}


# ---- the references agree -----------------------------------------------------------------

@pytest.mark.parametrize("c", C.COST_CASES, ids=lambda c: c.id)
def test_pin_equals_the_oracle(oracle, c):
    for f, (L, R) in enumerate(C.cost_pairs(c)):
        assert L.shape[:2] == (c.H, c.W) and (L.ndim == 3) == (c.cn == 3)
        for mode in (c.mode, C.other_hh_mode(c.mode)):
            ref = oracle.cost_volume(L, R, oracle.make_params(*C.create_args(c, mode)))
            pin = C.pin_of(c, f, mode)
            assert pin.shape == (c.H, c.W1, c.D) and np.array_equal(pin, ref), (f, mode)
            assert np.array_equal(pin, volume(c, mode, f=f)), (f, mode)  # the restatement the mutants turn
            assert pin.min() >= c.P2 >= 0


@pytest.mark.parametrize("H,W,cn", [(1, 3, 1), (1, 4, 3), (2, 5, 1), (3, 6, 3), (4, 9, 1), (3, 2, 1)])
def test_operand_planes_equal_the_loop(H, W, cn):
    rng = np.random.default_rng(10 * H + W)
    for cap in C.CAPS:
        ft = C.ftzero_of(cap)
        shape = (H, W) if cn == 1 else (H, W, cn)
        for img in (rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 2, shape).astype(np.uint8) * 255):
            p = C.operand_planes(img, ft)
            assert np.array_equal(p, C.operand_planes_loop(img, ft))
            assert p.min() >= 0 and p.max() <= 255 and (p[:, 1] <= p[:, 0]).all() and (p[:, 0] <= p[:, 2]).all()
            s8, s9 = C.stage8_pin(img, ft), C.stage9_pin(img, ft)
            assert s8.shape == (H, W, 3 * cn) and s8.dtype == np.uint32 and s9.shape == (3 * cn, H, W)
            assert np.array_equal(s9, C.stage9_loop(img, ft))
            # stage 8 holds the same six values a pixel as stage 9's q(x)
            for w in range(3 * cn):
                assert np.array_equal(s8[:, :, w] & 0xffff, (s9[w] & np.uint64(0xffff)).astype(np.uint32))
                assert np.array_equal(s8[:, :, w] >> 16, ((s9[w] >> np.uint64(32)) & np.uint64(0xffff)).astype(np.uint32))


def test_const_closed_form_holds_on_the_pin():
    consts = [c for c in C.COST_CASES if c.kind == "const"]
    assert {c.cn for c in consts} == {1, 3} and any(C.is_hh(c.mode) for c in consts)
    for c in consts:
        L, R = C.cost_pairs(c)[0]
        levels = C.const_levels(L, R)
        assert len(levels) == c.cn and all(a != b for a, b in levels)
        for mode in C.MODES:
            value, mask, frozen = C.const_closed_form(levels, c.H, c.W, c.minD, c.D, c.bs, c.P2, mode)
            pin = C.pin_of(c, 0, mode)
            assert mask.any() and (pin[mask] == value).all(), (c.id, mode)
            assert frozen.any() == C.is_hh(mode) and (pin[frozen] == c.P2).all()
            assert 3 * mask.sum() > mask.size // 2, c.id
    c = C.COST_BY_ID["const__bs11_hh"]
    assert any((abs(a - b) >> 2) > 0 for a, b in C.const_levels(*C.cost_pairs(c)[0]))


# ---- the cases discriminate ---------------------------------------------------------------
# A restatement of the pin with one knob per mistake.  With every knob at rest it equals the pin
# (test_pin_equals_the_oracle); with one turned, at least one case of the group that exists for that
# mistake must differ -- a group that cannot tell the wrong formula from the right one proves
# nothing on the GPU either.

def planes(ch, ft, nowrap):
    I = ch.astype(np.int64)
    H, W = I.shape
    up, dn = np.vstack([I[:1], I[:-1]]), np.vstack([I[1:], I[-1:]])
    m = (1 << 30) - 1 if nowrap else 0xff
    sob, raw = np.full((H, W), ft & m, np.int64), np.full((H, W), ft & m, np.int64)
    g = 2 * (I[:, 2:] - I[:, :-2]) + (up[:, 2:] - up[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
    sob[:, 1:-1] = (np.clip(g, -ft, ft) + ft) & m
    raw[:, 1:-1] = I[:, 1:-1]
    return sob, raw


def env(ch, rnd, zero_env):
    a, b = ch.copy(), ch.copy()
    a[:, :-1] = (ch[:, :-1] + ch[:, 1:] + rnd) // 2
    b[:, 1:] = (ch[:, 1:] + ch[:, :-1] + rnd) // 2
    if zero_env:  # the neighbour past the image read as 0
        a[:, -1] = (ch[:, -1] + rnd) // 2
        b[:, 0] = (ch[:, 0] + rnd) // 2
    return np.minimum(np.minimum(a, b), ch), np.maximum(np.maximum(a, b), ch)


def pixel_costs(L, R, minD, D, ft, cols, rnd=0, zero_env=False, nowrap=False, shift_after=False):
    """[H][len(cols)][D]: the pixel cost at matched-range columns cols (any integers: the image
    column minX1 + col and the right column are clamped to the image)."""
    H, W = L.shape[:2]
    minX1 = max(minD + D, 0)
    xl = np.clip(minX1 + cols, 0, W - 1)
    Ls = [L] if L.ndim == 2 else [L[:, :, i] for i in range(3)]
    Rs = [R] if R.ndim == 2 else [R[:, :, i] for i in range(3)]
    sob = np.zeros((H, len(cols), D), np.int64)
    raw = np.zeros((H, len(cols), D), np.int64)
    for lc, rc in zip(Ls, Rs):
        for k, (u, v) in enumerate(zip(planes(lc, ft, nowrap), planes(rc, ft, nowrap))):
            u0, u1 = env(u, rnd, zero_env)
            v0, v1 = env(v, rnd, zero_env)
            for di in range(D):
                xr = np.clip(minX1 + cols - (minD + di), 0, W - 1)
                c0 = np.maximum(0, np.maximum(u[:, xl] - v1[:, xr], v0[:, xr] - u[:, xl]))
                c1 = np.maximum(0, np.maximum(v[:, xr] - u1[:, xl], u0[:, xl] - v[:, xr]))
                cost = np.minimum(c0, c1)
                if k == 0:
                    sob[:, :, di] += cost
                else:
                    raw[:, :, di] += cost if shift_after else cost >> 2
    return sob + (raw >> 2 if shift_after else raw)


def horizontal(c, f=0, ximg=False, **kw):
    """hs [H][W1][D].  ximg: the box's columns clamp to the image instead of the matched columns."""
    L, R = (C.stripe_pair(c) if "stripes" in c.tags else C.cost_pairs(c)[f])
    s = c.bs // 2
    cols = np.arange(-s, c.W1 + s) if ximg else np.clip(np.arange(-s, c.W1 + s), 0, c.W1 - 1)
    pix = pixel_costs(L, R, c.minD, c.D, C.ftzero_of(c.cap), cols, **kw)
    return sum(pix[:, k:k + c.W1] for k in range(2 * s + 1))


def box(hs, s0, end, SH2, hh, freeze=True, hh_off=0, lo=None):
    """numpy_ref._box_rows.  freeze: the window stops at H-1-SH2; hh_off: added to the first row that
    keeps P2 under MODE_HH; lo: the row the window's top clamps at (the pin: s0)."""
    H = hs.shape[0]
    lo = s0 if lo is None else lo
    out = np.zeros((end - s0,) + hs.shape[1:], np.int64)
    ylim = max(H - 1 - SH2, s0) if freeze else H - 1
    for y in range(s0, end):
        if hh and y > 0 and y + SH2 >= H + hh_off:
            continue
        t = min(y, ylim)
        out[y - s0] = hs[np.clip(np.arange(t - SH2, t + SH2 + 1), lo, H - 1)].sum(0)
    return out


def volume(c, mode, f=0, bkw={}, **hkw):
    return c.P2 + box(horizontal(c, f, **hkw), 0, c.H, c.bs // 2, C.is_hh(mode), **bkw)


def differing(cases, modes=None, **kw):
    out = []
    for c in cases:
        for m in (modes or (c.mode,)):
            if not np.array_equal(volume(c, m), volume(c, m, **kw)):
                out.append(c.id)
                break
    return out


def tagged(tag, pred=lambda c: True):
    return [c for c in C.COST_CASES if tag in c.tags and pred(c)]


LIVELY = ("noise", "binary", "ties")  # kinds whose rows and columns differ


def test_x_clamped_to_the_image_shows_in_every_width_class():
    for k in (1, 2):
        for cls in C.W1_CLASSES:
            group = tagged("instantiation", lambda c: C.kernel_of(c.bs, c.D)[2] == k and C.w1_class(c) == cls
                           and c.bs > 1)
            assert group and differing(group, ximg=True) == [c.id for c in group], (k, cls)
    group = tagged("minD")
    assert differing(group, ximg=True) == [c.id for c in group]


def test_no_vertical_freeze_shows_on_the_height_and_band_entries():
    for bs in (7, 11):
        for cls in C.H_CLASSES:
            group = tagged("height", lambda c: c.bs == bs and c.tags[1] == cls)
            # a row past ylim exists from H = 2 on
            want = [c.id for c in group] if group[0].H >= 2 else []
            assert differing(group, (SGM_SGBM,), bkw=dict(freeze=False)) == want, (bs, cls)
    for cls in ("straddles_ylim", "frozen"):
        group = tagged("band", lambda c: c.tags[1] == cls)
        assert len(group) == 7 and differing(group, bkw=dict(freeze=False)) == [c.id for c in group], cls


def test_hh_rule_off_by_one_row_shows():
    for off in (-1, 1):
        for cls in ("hh_straddles_yl", "hh_p2_only"):
            group = tagged("band", lambda c: c.tags[1] == cls)
            assert len(group) == 7 and differing(group, bkw=dict(hh_off=off)) == [c.id for c in group], (off, cls)
        for bs in (7, 11):
            # the rule's first P2 row, H - SH2, moves up to a row >= 1 from H = SH2 + 2 on, and down
            # from H = SH2 + 1 on
            group = tagged("height", lambda c: c.bs == bs and c.H >= bs // 2 + (2 if off < 0 else 1))
            assert len(group) == (2 if off < 0 else 3)
            assert differing(group, (SGM_HH, SGM_HH4), bkw=dict(hh_off=off)) == [c.id for c in group], (off, bs)


def test_shift_after_the_channel_sum_shows_on_colour_only():
    colour = [c for c in C.COST_CASES if c.cn == 3 and c.kind in LIVELY and "generic" not in c.tags]
    assert len(colour) >= 20 and differing(colour, shift_after=True) == [c.id for c in colour]
    gray = tagged("kind", lambda c: c.cn == 1)
    assert differing(gray, shift_after=True) == []


def test_rounding_average_shows():
    group = [c for c in tagged("instantiation") + tagged("kind") if c.kind in LIVELY]
    assert len(group) >= 26 and differing(group, rnd=1) == [c.id for c in group]


def test_unclamped_envelope_shows_where_a_border_column_is_matched():
    # minD >= 0: the left image's last column is matched in every row; minD < 0: only the last
    # matched column at d = minD reads the right image's last column
    group = [c for c in tagged("instantiation") + tagged("minD") if c.kind in LIVELY and c.minD >= 0]
    assert len(group) >= 20 and any(c.minD > 0 for c in group)
    assert differing(group, zero_env=True) == [c.id for c in group]
    assert differing(tagged("minD", lambda c: c.minD < 0), zero_env=True)


def test_unwrapped_ftzero_shows_from_cap_128_on():
    group = tagged("cap")
    assert differing(group, nowrap=True) == [c.id for c in group if c.cap >= 128]
    assert [c.cap for c in group if c.cap >= 128] == [128, 255, 1000]


def test_stripe_window_clamped_at_row_0_shows_on_the_stripe_rows():
    clamp0, with_rows = set(), 0
    for c in C.STRIPE_CASES:
        L, R = C.stripe_pair(c)
        rows, (nstr, amax) = C.stripe_rows_ref(L, R, c)
        st = stripes_of(c.H, c.ns, c.bs, c.bs // 2)
        assert nstr == len(st) and amax == max(s[3] for s in st)
        if not rows:
            continue
        with_rows += 1
        hs = horizontal(c)
        assert np.array_equal(hs, C.horizontal_sums(L, R, c.minD, c.D, c.bs, C.ftzero_of(c.cap)))
        for s, ref in rows:
            s0, end, out0, aux = st[s]
            assert ref.shape == (aux, c.W1, c.D)
            assert np.array_equal(ref, c.P2 + box(hs, s0, s0 + aux, c.bs // 2, False))
            assert np.array_equal(ref, (c.P2 + N._box_rows(hs, s0, end, c.bs // 2, False))[:aux])
            if not np.array_equal(ref, c.P2 + box(hs, s0, s0 + aux, c.bs // 2, False, lo=0)):
                clamp0.add(c.id)
    assert with_rows >= 13 and len(clamp0) == with_rows


# ---- refusals -----------------------------------------------------------------------------

def test_knob_and_stages_reject_a_null_handle():
    L = _lib.lib()
    buf = np.zeros(16, np.uint64)
    assert L.sdr_sgbm_debug_knob(None, 3, 4) == -1
    for stage in (8, 9):
        assert L.sdr_sgbm_debug_stage(None, stage, buf.ctypes.data, buf.nbytes) == -1
    from stereo_depth_ruler_amd import sgbm
    assert (sgbm.DEBUG_SWEEP_SPIN, sgbm.DEBUG_PLAN_CUS, sgbm.DEBUG_COST_ROWS) == (1, 2, 3)
    assert ctypes.sizeof(_lib.SgbmLaunches) == 26 * 4
    assert _lib.SgbmLaunches.cost_rows.offset == 24 * 4 and _lib.SgbmLaunches.cost_bands.offset == 25 * 4
