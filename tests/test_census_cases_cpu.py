"""The census edge cases (census_cases.py) without a GPU: the pin against an independent loop where
both clamps act at once, the ramps' closed form, the tables against what they claim to reach, and
-- so that a passing GPU test means something -- deliberately wrong references that each group of
cases must tell from the pin."""
import ctypes

import numpy as np
import pytest

import census_cases as C
import census_ref as CR
from numpy_ref import SGM_3WAY, SGM_HH, SGM_HH4, SGM_SGBM, _box_rows
from stereo_depth_ruler_amd import _lib
from test_plan_cpu import stripes_of

CENSUS = 1


# ---- the pin ------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 3), (3, 8), (6, 9), (7, 10), (8, 13)])
def test_pin_equals_the_loop_on_images_smaller_than_the_window(H, W):
    rng = np.random.default_rng(100 * H + W)
    for _ in range(4):
        img = (rng.integers(0, 4, (H, W)) * 85).astype(np.uint8)
        assert np.array_equal(CR.census_9x7(img), C.census_loop(img))


def test_ramps_known_answer():
    """20 x 120, D 32, blockSize 11 at the domain's largest P2: C = 19408 on matched columns 0..81
    of 88 (column 87 at d = 0 reads the right image's last column, which has no darker neighbour),
    and nothing in the volume is larger."""
    c = C.COST_BY_ID["ramps__bs11_P2max"]
    assert (c.H, c.W, c.D, c.bs, c.P2, c.W1) == (20, 120, 32, 11, 12632, 88)
    L, R = C.pair("ramps", c.H, c.W)
    vol = CR.census_cost_volume(L, R, 0, c.D, c.bs, c.P2, SGM_SGBM)
    value, mask = C.ramps_closed_form(c.H, c.W, 0, c.D, c.bs, c.P2, SGM_SGBM)
    assert value == 19408 and vol.max() == 19408
    assert (vol[:, :82] == 19408).all() and (vol[:, 82:, 0] < 19408).all()
    assert mask.any() and (vol[mask] == value).all()
    assert 2 * mask.sum() > mask.size  # the closed form covers most of the volume


@pytest.mark.parametrize("cid", ["ramps__bs11_P2max", "ramps__k2_hh"])
def test_ramps_closed_form_in_every_mode(cid):
    c = C.COST_BY_ID[cid]
    L, R = C.pair("ramps", c.H, c.W)
    for mode in C.MODES:
        value, mask = C.ramps_closed_form(c.H, c.W, c.minD, c.D, c.bs, c.P2, mode)
        vol = CR.census_cost_volume(L, R, c.minD, c.D, c.bs, c.P2, mode)
        assert mask.any() and (vol[mask] == value).all(), mode


# ---- the tables reach what they claim -----------------------------------------------------

def plan_bytes(c, mode=None, nstripes=4, F=None):
    p = _lib.SgbmParams(c.minD, c.D, c.bs, c.P1, c.P2, 1, 0, 12, 0, 0, c.mode if mode is None else mode,
                        nstripes, 0)
    return _lib.lib().sdr_sgbm_scratch_bytes_ex(ctypes.byref(p), CENSUS, c.W, c.H, 1, c.F if F is None else F)


def test_cost_table_covers_what_it_claims():
    cases = C.COST_CASES
    assert len({c.id for c in cases}) == len(cases)
    assert {C.kernel_of(c.bs, c.D) for c in cases} == {(bs, k) for bs in C.BLOCK_SIZES for k in (1, 2)}
    assert {c.mode for c in cases} == set(C.MODES)
    for k, ds in ((1, {16, 48, 128}), (2, {144, 256})):
        mine = [c for c in cases if C.kernel_of(c.bs, c.D)[1] == k]
        assert {C.w1_class(c) for c in mine} >= set(C.W1_CLASSES), k
        assert {c.D for c in mine} >= ds, k
        # an interior column block exists at 3*BCOLS + 5 and nowhere narrower than a block + its halo
        for c in mine:
            b, s = C.bcols_of(c.D), c.bs // 2
            interior = [bx for bx in range((c.W1 + b - 1) // b) if bx * b - s >= 0 and bx * b + b + s <= c.W1]
            if C.w1_class(c) == "3bcols+5":
                assert 1 in interior and (c.W1 + b - 1) // b == 4, c.id  # and a 5-column last block
            elif C.w1_class(c) is not None and c.bs > 1:
                assert not interior, c.id
    for bs in (7, 11):
        assert {C.h_class(c) for c in cases if c.bs == bs} >= set(C.H_CLASSES), bs
    assert {c.minD for c in cases} >= {0, 3, -20}
    assert any(c.minD + c.D < 0 for c in cases)
    assert any(c.F == 3 for c in cases)
    assert {c.kind for c in cases} >= {"ties", "noise", "flat", "binary", "periodic", "steps", "ramps"}
    for bs in C.BLOCK_SIZES:  # the domain's largest P2 computes at every block size's bound or below it
        assert 2 * C.p2_census_max(bs) + 62 * bs * bs <= 32767 < 2 * (C.p2_census_max(bs) + 1) + 62 * bs * bs
    assert {c.bs for c in cases if c.P2 == C.p2_census_max(c.bs)} == set(C.BLOCK_SIZES)
    for c in cases:
        assert c.H <= 40 and c.W <= 420, c.id
        assert c.W1 == c.W + min(c.minD, 0) - max(c.minD + c.D, 0) >= c.bs // 2 + 1, c.id
        assert c.kind != "ramps" or c.W <= 256, c.id


@pytest.mark.parametrize("c", C.COST_CASES, ids=lambda c: c.id)
def test_cost_case_passes_the_plan_and_the_pin(c):
    for mode in C.MODES:
        assert plan_bytes(c, mode) > 0, (mode, _lib.lib().sdr_last_error())
    L, R = C.cost_pairs(c)[0]
    assert L.shape == (c.H, c.W)
    out = C.sgm_of(L, R, C.create_args(c))  # sgm_census asserts the int16 domain of C and of every L_r
    assert out.shape == (c.H, c.W)
    assert CR.census_cost_volume(L, R, c.minD, c.D, c.bs, c.P2, c.mode).shape == (c.H, c.W1, c.D)


def test_domain_edge_is_the_plans_edge():
    for bs in C.BLOCK_SIZES:
        p = _lib.SgbmParams(0, 16, bs, 1, C.p2_census_max(bs) + 1, 1, 0, 12, 0, 0, 0, 4, 0)
        assert _lib.lib().sdr_sgbm_scratch_bytes_ex(ctypes.byref(p), CENSUS, 64, 20, 1, 1) == 0
        assert b"int16" in _lib.lib().sdr_last_error()


def test_transform_table_covers_what_it_claims():
    shapes = C.TRANSFORM_SHAPES
    assert len({s[0] for s in shapes}) == len(shapes)
    assert {s[2] for s in shapes} == C.TRANSFORM_WIDTHS and {s[1] for s in shapes} == C.TRANSFORM_HEIGHTS
    reached = set()
    for name, H, W, layout in shapes:
        F, stride, fstride, offL, offR, nbytes = C.transform_layout(H, W, layout)
        assert stride >= W and fstride >= H * stride and offR >= offL + F * fstride and nbytes >= offR + F * fstride
        p = _lib.SgbmParams(0, 16, 1, 2, 12, 1, 0, 12, 0, 0, 0, 4, 0)
        assert _lib.lib().sdr_sgbm_scratch_bytes_ex(ctypes.byref(p), CENSUS, W, H, 1, F) > 0, name
        dword = [C.takes_dword_path(W, stride, fstride, off & 3) for off in (offL, offR)]
        assert dword[0] == dword[1], name
        why = "dword" if dword[0] else "odd" if W & 3 else "stride" if stride & 3 else \
            "base" if offL & 3 else "fstride"
        if why == "base":
            assert offL & 3 and offR & 3 and (offL & 3) != (offR & 3)
        reached.add((why, F))
        assert name.startswith({"dword": "dword", "odd": ("odd", "batch_17"), "stride": "stride", "base": "base1",
                                "fstride": "batch"}[why]), (name, why)
    assert reached >= {("dword", 1), ("odd", 1), ("stride", 1), ("base", 1), ("fstride", 3), ("odd", 3)}
    # the row loop's trips at 256 columns a trip
    dense_dword = {W for n, H, W, l in shapes if l == "dense" and W % 4 == 0}
    assert any(W <= 256 for W in dense_dword) and any(256 < W <= 512 for W in dense_dword) and 1024 in dense_dword
    assert {1 + (s[2] - 1) // 256 for s in shapes} >= {1, 2, 3, 4}
    assert {l[1] for n, H, W, l in shapes if isinstance(l, tuple) and l[0] == "stride"} == {1, 7}


def test_stripe_table_covers_what_it_claims():
    cases = C.STRIPE_CASES
    assert len({c.id for c in cases}) == len(cases)
    assert {c.ns for c in cases} == {1, 3, 4, 8}
    assert {(c.H, c.ns, c.bs) for c in C.SHORT_STRIPE_CASES} == \
        {(H, ns, bs) for H in (14, 15, 17, 18, 21, 26) for ns in (4, 8) for bs in (7, 9, 11)}
    short = full = 0
    for c in cases:
        assert plan_bytes(c, nstripes=c.ns) > 0, c.id
        st = stripes_of(c.H, c.ns, c.bs, c.bs // 2)
        short += sum(1 for s0, end, out0, aux in st if aux and aux == end - s0 and aux != c.bs // 2)
        full += sum(1 for s0, end, out0, aux in st if aux == c.bs // 2 and aux != end - s0)
    assert short >= 20 and full >= 10
    # every one of the adversarial test's block sizes has a stripe whose every row is its own
    for bs in (7, 9, 11):
        assert any(aux and aux == end - s0 for c in C.SHORT_STRIPE_CASES if c.bs == bs
                   for s0, end, out0, aux in stripes_of(c.H, c.ns, c.bs, c.bs // 2)), bs
    assert {C.kernel_of(c.bs, c.D)[1] for c in cases} == {1, 2}


@pytest.mark.parametrize("c", C.STRIPE_CASES, ids=lambda c: c.id)
def test_stripe_case_passes_the_pin(c):
    L, R = C.pair(c.kind, c.H, c.W, c.D, seed=c.H)
    C.sgm_of(L, R, C.create_args(c), nstripes=c.ns)
    rows, (nstr, amax) = C.stripe_rows_ref(L, R, 0, c.D, c.bs, c.P2, c.ns)
    st = stripes_of(c.H, c.ns, c.bs, c.bs // 2)
    assert nstr == len(st) and amax == max(s[3] for s in st)
    # the stripe's rows in the pin's own per-stripe volume are these rows
    hs = C.horizontal_sums(L, R, 0, c.D, c.bs)
    for s, ref in rows:
        s0, end, out0, aux = st[s]
        assert ref.shape == (aux, c.W1, c.D) and aux <= amax
        assert np.array_equal(ref, (c.P2 + _box_rows(hs, s0, end, c.bs // 2, False))[:aux])


def test_random_cases_lie_inside_the_domain():
    cases = C.random_cases(480, seed=1)
    assert [vars(a) for a in C.random_cases(48, seed=1)] == [vars(a) for a in cases[:48]]  # seeded, a prefix
    for c in cases:
        assert c.mode in C.MODES and c.bs in C.BLOCK_SIZES and c.D % 16 == 0 and 16 <= c.D <= 256
        assert -40 <= c.minD <= 8 and 4 <= c.H <= 36 and c.bs // 2 + 1 <= c.W1 <= 120
        assert 1 <= c.P1 < c.P2 <= C.p2_census_max(c.bs)
        assert c.kind in C.KINDS and (c.kind != "ramps" or c.W <= 256)
        p = _lib.SgbmParams(*C.random_args(c), c.nstripes, c.uniq_rule)
        assert _lib.lib().sdr_sgbm_scratch_bytes_ex(ctypes.byref(p), CENSUS, c.W, c.H, 1, 1) > 0, vars(c)
    first = cases[:48]
    assert {c.mode for c in first} == set(C.MODES) and {c.bs for c in first} == set(C.BLOCK_SIZES)
    assert {c.nstripes for c in first} == {1, 2, 3, 4, 8} and {c.uniq_rule for c in first} == {0, 1, 2}
    assert {c.uniq for c in first} == {0, 1, 10, 15, 50} and {c.d12 for c in first} == {1, 2, 1000000}
    assert any(c.P2 == C.p2_census_max(c.bs) for c in first) and any(c.speckle[0] for c in first)
    assert any(c.D > 128 for c in first) and any(c.minD + c.D < 0 for c in first)
    assert {c.kind for c in first} == set(C.KINDS)


# ---- the cases discriminate ---------------------------------------------------------------
# A restatement of the pin with one knob per mistake.  With every knob at rest it equals the pin;
# with one turned, at least one case of the group that exists for that mistake must differ -- a
# group that cannot tell the wrong formula from the right one proves nothing on the GPU either.

def transform(img, le=False):
    I = np.asarray(img)
    H, W = I.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.uint64)
    for k, (dy, dx) in enumerate(CR.CENSUS_OFFSETS):
        nb = I[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
        out |= ((nb <= I) if le else (nb < I)).astype(np.uint64) << np.uint64(k)
    return out


def horizontal(L, R, minD, D, bs, le=False, rshift=0, xhi=0):
    """hs [H][W1][D].  le: '<=' in the transform; rshift: the right descriptor of x - d - rshift;
    xhi: the horizontal window clamps at W1 - 1 + xhi (the column past the last one computed from
    clamped images, as the kernel computes its halo)."""
    H, W = L.shape
    maxD = minD + D
    minX1, W1 = max(maxD, 0), W + min(minD, 0) - max(maxD, 0)
    TL, TR = transform(L, le), transform(R, le)
    cols = np.arange(W1 + xhi)
    xl = minX1 + np.minimum(cols, W1 - 1)
    pix = np.zeros((H, W1 + xhi, D), np.int64)
    for di, d in enumerate(range(minD, maxD)):
        pix[:, :, di] = CR.popcount64(TL[:, xl] ^ TR[:, np.clip(minX1 + cols - d - rshift, 0, W - 1)])
    s = bs // 2
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1 + xhi)
    return pix[:, xi, :].sum(2)


def box(hs, s0, end, SH2, hh_bottom, lo=None, dylim=0):
    """numpy_ref._box_rows.  lo: the row the window's top clamps at (the pin: s0); dylim: added to
    the row the running window freezes at, H-1-SH2."""
    H = hs.shape[0]
    lo = s0 if lo is None else lo
    out = np.zeros((end - s0,) + hs.shape[1:], np.int64)
    ylim = max(H - 1 - SH2 + dylim, s0)
    for y in range(s0, end):
        if hh_bottom and y > 0 and y + SH2 >= H:
            continue
        t = min(y, ylim)
        out[y - s0] = hs[np.clip(np.arange(t - SH2, t + SH2 + 1), lo, H - 1)].sum(0)
    return out


def volume(c, mode, hkw={}, bkw={}, hh=None):
    L, R = C.cost_pairs(c)[0]
    hh = mode in (SGM_HH, SGM_HH4) if hh is None else hh
    return c.P2 + box(horizontal(L, R, c.minD, c.D, c.bs, **hkw), 0, c.H, c.bs // 2, hh, **bkw)


def differing(cases, modes, **kw):
    return [c.id for c in cases if any(not np.array_equal(volume(c, m), volume(c, m, **kw)) for m in modes)]


def test_restatement_equals_the_pin():
    for c in C.COST_CASES:
        L, R = C.cost_pairs(c)[0]
        for mode in (SGM_SGBM, SGM_HH):
            assert np.array_equal(volume(c, mode), CR.census_cost_volume(L, R, c.minD, c.D, c.bs, c.P2, mode)), c.id
    for _, H, W, _ in C.TRANSFORM_SHAPES[:6]:
        img = C.pair("ties", H, W, seed=3)[0]
        assert np.array_equal(transform(img), CR.census_9x7(img))


def test_le_instead_of_lt_shows_on_ties_and_noise_only():
    for _, H, W, _ in C.TRANSFORM_SHAPES:
        for kind in ("ties", "noise", "binary"):
            img = C.pair(kind, H, W, seed=H + W)[0]
            assert not np.array_equal(transform(img, le=True), CR.census_9x7(img)), (kind, H, W)
    # in the cost volume a flat pair cannot show it (both descriptors change alike); every ties
    # and noise case does
    by_kind = {k: [c for c in C.COST_CASES if c.kind == k] for k in ("flat", "ties", "noise")}
    assert by_kind["flat"] and len(by_kind["ties"]) >= 8 and len(by_kind["noise"]) >= 12
    assert differing(by_kind["flat"], (SGM_SGBM,), hkw=dict(le=True)) == []
    for kind in ("ties", "noise"):
        assert differing(by_kind[kind], (SGM_SGBM,), hkw=dict(le=True)) == [c.id for c in by_kind[kind]]


def test_right_descriptor_off_by_one_shows():
    # (the ramps cannot show it away from the borders: that is what their closed form is for)
    cases = [c for c in C.COST_CASES if c.kind not in ("flat", "ramps")]
    assert differing(cases, (SGM_SGBM,), hkw=dict(rshift=1)) == [c.id for c in cases]


def test_horizontal_clamp_one_past_shows_in_every_width_class():
    for k in (1, 2):
        for cls in C.W1_CLASSES:
            group = [c for c in C.COST_CASES if C.kernel_of(c.bs, c.D)[1] == k and C.w1_class(c) == cls
                     and c.bs > 1 and c.kind != "flat"]
            assert group and differing(group, (SGM_SGBM,), hkw=dict(xhi=1)) == [c.id for c in group], (k, cls)


def test_ylim_off_by_one_and_dropped_hh_bottom_show_in_every_height_class():
    for bs in (7, 11):
        for cls in C.H_CLASSES:
            group = [c for c in C.COST_CASES if c.bs == bs and C.h_class(c) == cls]
            assert group
            s, H = bs // 2, group[0].H
            # ylim - 1 changes a row when a row lies at or past ylim >= 1; MODE_HH's bottom rows
            # exist from two rows on
            want = [c.id for c in group]
            assert differing(group, (SGM_SGBM, SGM_3WAY), bkw=dict(dylim=-1)) == (want if H >= s + 2 else []), (bs, cls)
            assert differing(group, (SGM_HH, SGM_HH4), hh=False) == (want if H >= 2 else []), (bs, cls)
    # (flat, ramps, periodic and steps repeat one row: no vertical mistake shows on them)
    tall = [c for c in C.COST_CASES if c.H >= c.bs // 2 + 2 and c.kind in ("noise", "ties", "binary", "textured")]
    assert len(tall) >= 20 and differing(tall, (SGM_SGBM,), bkw=dict(dylim=-1)) == [c.id for c in tall]
    tall = [c for c in tall if c.bs > 1]  # blockSize 1: no row lies past H-1-SH2
    assert differing(tall, (SGM_SGBM,), bkw=dict(dylim=1)) == [c.id for c in tall]


def test_stripe_window_clamped_at_row_0_and_ylim_show_on_the_stripe_rows():
    clamp0, ylim = [], []
    with_rows = 0
    for c in C.STRIPE_CASES:
        L, R = C.pair(c.kind, c.H, c.W, c.D, seed=c.H)
        rows, _ = C.stripe_rows_ref(L, R, 0, c.D, c.bs, c.P2, c.ns)
        if not rows:
            continue
        with_rows += 1
        st = stripes_of(c.H, c.ns, c.bs, c.bs // 2)
        hs = C.horizontal_sums(L, R, 0, c.D, c.bs)
        for s, ref in rows:
            s0, end, out0, aux = st[s]
            assert np.array_equal(ref, c.P2 + box(hs, s0, s0 + aux, c.bs // 2, False))
            if not np.array_equal(ref, c.P2 + box(hs, s0, s0 + aux, c.bs // 2, False, lo=0)):
                clamp0.append(c.id)
            if not np.array_equal(ref, c.P2 + box(hs, s0, s0 + aux, c.bs // 2, False, dylim=-1)):
                ylim.append(c.id)
    # every case with rows of its own tells the clamp
    assert with_rows >= 40 and len(set(clamp0)) == with_rows
    assert ylim


# ---- the row bands ------------------------------------------------------------------------

def test_band_cases_reach_their_trips_and_tails():
    """Every band class at NR 5, 7 and 11 and both K: the entry's band height (set through
    SDR_DEBUG_COST_ROWS on the GPU) puts a band in the class it is named for, by the kernel's own
    row count n = tlast - tfirst + 1 + 2 SH2 and its unroll U = 2 NR."""
    assert {(c.bs, C.kernel_of(c.bs, c.D)[1]) for c in C.BAND_CASES} == set(C.BAND_KERNELS)
    assert {nr for nr, k in C.BAND_KERNELS} >= {5, 7, 11} and {k for nr, k in C.BAND_KERNELS} == {1, 2}
    for nr, k in C.BAND_KERNELS:
        assert [c.cls for c in C.BAND_CASES if (c.bs, C.kernel_of(c.bs, c.D)[1]) == (nr, k)] == list(C.BAND_CLASSES)
    for c in C.BAND_CASES:
        assert c.H <= 80 and plan_bytes(c) > 0 and plan_bytes(c, SGM_HH) > 0, c.id
        s, U, ylim = c.bs // 2, 2 * c.bs, max(c.H - 1 - c.bs // 2, 0)
        bands = C.bands_of(c)
        assert [b[:2] for b in bands] == [(y, min(y + c.ty, c.H)) for y in range(0, c.H, c.ty)]
        assert any(c.cls in b[4] for b in bands), (c.id, bands)
        for ty0, ty1, trips, tail, _ in bands:
            yl = max(ty0, min(ty1, max(1, c.H - s))) if C.is_hh(c.mode) else ty1
            if yl <= ty0:
                assert trips is None
                continue
            assert (trips, tail) == divmod(min(yl - 1, ylim) - min(ty0, ylim) + 1 + 2 * s, U)
        # under the launcher's own 4-row bands no block completes a trip
        assert all(b[2] in (0, None) for b in C.bands_of(c, ty=4)), c.id
    for nr in (5, 7, 11):
        assert any(b[2] >= 3 for c in C.BAND_CASES if c.bs == nr for b in C.bands_of(c))
