"""The emit edge cases (emit_cases.py) without a GPU: each case has the property it is named for,
shown with the oracle and numpy, so that a pass of test_gpu_cloud_edges.py and
test_gpu_display_edges.py means the engine was taken to that edge -- the sort's pass counts, the
sizes, the anisotropy, cell indices past 2^24, order-sensitive sums, PCL's 2^31 decision, the first
float of every output level, all 65 536 operand pairs of each addWeighted and the compare values of
the depth statistics."""
import numpy as np
import pytest

import emit_cases as E
from test_oracle_cloud import wrapped_extent_product

F32 = np.float32


def eq(a, b):
    return a.shape == b.shape and np.array_equal(E.u32(a), E.u32(b))


# ---- voxel grid -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", E.VOXEL_IDS)
def test_numpy_restatement_equals_oracle(oracle, cid):
    pts, leaf = E.voxel_case(cid)
    ref, passthrough = E.voxel_reference(oracle, cid)
    got, pt = E.np_voxel(pts, leaf)
    assert pt == passthrough and eq(got, ref)


def test_lattice_is_what_it_claims():
    pts, _ = E.voxel_case("band-16x16x1")
    fin = np.isfinite(pts[:, :3]).all(1)
    assert not fin[0] and not fin[-1] and 0.08 < 1 - fin.mean() < 0.12
    bad = pts[~fin, :3]
    for c in range(3):  # NaN, +inf and -inf, each in x, in y and in z
        assert np.isnan(bad[:, c]).any() and (bad[:, c] == np.inf).any() and (bad[:, c] == -np.inf).any()
    assert len(np.unique(pts.view(np.uint32)[:, 3] >> 24)) == 256  # alpha too: all 32 bits random
    P = E.voxel_params(pts, E.LEAF)
    first, second = pts[np.flatnonzero(fin)[:2], :3]
    assert np.array_equal(np.floor(first * P.inv), P.fmin)
    assert np.array_equal(np.floor(second * P.inv) - P.fmin, [15, 15, 0])


@pytest.mark.parametrize("dims,nbits", list(zip(E.BAND_DIMS, E.BAND_BITS)), ids=lambda v: str(v))
def test_band_cases_sit_on_the_pass_count_edges(oracle, dims, nbits):
    cid = "band-%dx%dx%d" % dims
    pts, leaf = E.voxel_case(cid)
    P = E.voxel_params(pts, leaf)
    assert tuple(P.div) == dims and P.past == dims[0] * dims[1] * dims[2]
    assert P.past.bit_length() == nbits
    assert len(pts) == 4097 and leaf == E.LEAF
    # voxel 0 holds points from both ends of the cloud with non-finite ones in between: a marker
    # that sorted to digit 0 would cut its run
    cell = np.floor(pts[:, :3] * P.inv) - P.fmin
    zero = np.flatnonzero(P.fin & (cell == 0).all(1))
    assert len(zero) >= 3 and (~P.fin[zero[0]:zero[1]]).any() and (~P.fin[zero[-2]:zero[-1]]).any()
    ref, passthrough = E.voxel_reference(oracle, cid)
    assert not passthrough and 0 < len(ref) <= P.fin.sum()


def test_band_products():
    assert [E.voxel_params(*E.voxel_case("band-%dx%dx%d" % d)).past for d in E.BAND_DIMS] == \
        [255, 256, 65535, 65536, 16776450, 2**24, 2146435072]
    passes = [(b + 7) // 8 for b in E.BAND_BITS]
    assert passes == [1, 2, 2, 3, 3, 4, 4]


def test_size_cases(oracle):
    assert E.SIZES == [1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193]
    for n in E.SIZES:
        pts, _ = E.voxel_case(f"size-{n}")
        fin = np.isfinite(pts[:, :3]).all(1)
        assert len(pts) == n and fin.any()
        if n >= 8:
            assert not fin[0] and not fin[-1]
        ref, passthrough = E.voxel_reference(oracle, f"size-{n}")
        assert not passthrough and 1 <= len(ref) <= 105
    pts, _ = E.voxel_case("one-finite")
    assert len(pts) == 300 and np.isfinite(pts[:, :3]).all(1).sum() == 1
    assert len(E.voxel_reference(oracle, "one-finite")[0]) == 1
    pts, _ = E.voxel_case("none-finite")
    assert len(pts) == 300 and not np.isfinite(pts[:, :3]).all(1).any()
    assert len(E.voxel_reference(oracle, "none-finite")[0]) == 0


def test_anisotropy_shows(oracle):
    """No two permutations of the leaf give the same output, and none equals an isotropic leaf: an
    engine that used one axis' leaf for all three cannot pass."""
    assert len(E.PERMS) == 6
    ids = ["aniso-%g-%g-%g" % l for l in E.PERMS + E.ISO]
    base = E.voxel_case(ids[0])[0]
    outs = []
    for cid in ids:
        assert np.array_equal(E.u32(E.voxel_case(cid)[0]), E.u32(base))  # the same cloud
        outs.append(E.voxel_reference(oracle, cid)[0])
    for i in range(len(outs)):
        for j in range(i):
            assert not eq(outs[i], outs[j]), (ids[i], ids[j])


@pytest.mark.parametrize("cid,axis", [("minb+x", 0), ("minb-y", 1)])
def test_cell_indices_past_2_24(oracle, cid, axis):
    """floor(min * inv) lies past 2^24, where floats are 2 apart: the 5 cells of that axis fall into
    3 (75 voxels for 125 cells), so floorf(p * inv) is taken where it is coarser than the grid.

    min_b itself is the cast of that float, so (float)min_b == min_b for EVERY input; here both
    operands of PCL's float subtraction lie in one binade and their difference is exact, so the
    subtraction done in integers after the cast gives the same output (asserted).  What tells the
    two apart is an axis of more than 2^24 cells: test_float_subtraction_of_min_b_shows."""
    pts, leaf = E.voxel_case(cid)
    P = E.voxel_params(pts, leaf)
    assert abs(P.fmin[axis]) > 2**24 and abs(int(P.minb[axis])) > 2**24
    assert float(F32(P.minb[axis])) == P.minb[axis]
    assert ((P.mx - P.mn) * P.inv).max() < 16
    ref, passthrough = E.voxel_reference(oracle, cid)
    assert not passthrough and len(ref) == 75
    assert eq(E.np_voxel(pts, leaf, int_minb=True)[0], ref)
    other = E.lattice((5, 5, 5), 1000, leaf, (0.3, 0.1, -0.2), seed=9)
    assert len(oracle.voxel_grid(other, leaf)[0]) == 125  # the same lattice near the origin


@pytest.mark.parametrize("cid,near", [("minb-wide+3", 3), ("minb-wide-5", -5)])
def test_float_subtraction_of_min_b_shows(oracle, cid, near):
    """More than 2^24 cells along x from an odd min_b: floorf(x * inv) - (float)min_b is not a float
    for the far cells, the float subtraction rounds it (ties to even) and merges cells; done in
    integers after the cast, all eight cells stay apart.  The extents keep PCL's casts defined."""
    pts, leaf = E.voxel_case(cid)
    P = E.voxel_params(pts, leaf)
    assert int(P.minb[0]) == near and near % 2 == 1 and P.div[0] > 2**24 and tuple(P.div[1:]) == (1, 1)
    assert 0 < P.prod <= 2**31 - 1 and P.past.bit_length() == 26
    far = np.asarray(E.WIDE_FAR, F32)
    exact = far.astype(np.int64) - near
    assert (F32(1) * far - F32(near)).astype(np.int64).tolist() != exact.tolist()
    ref, passthrough = E.voxel_reference(oracle, cid)
    ints, _ = E.np_voxel(pts, leaf, int_minb=True)
    assert not passthrough and len(ints) == 8 > len(ref) >= 4
    assert not eq(ints[:len(ref)], ref)


def test_long_runs_are_order_sensitive(oracle):
    pts, leaf = E.voxel_case("long-one")
    assert len(pts) == E.LONG_N > 65793
    ref, _ = E.voxel_reference(oracle, "long-one")
    assert len(ref) == 1
    c = pts.view(np.uint32)[:, 3]
    for shift in (0, 8, 16, 24):
        assert int(((c >> shift) & 255).sum()) > 2**24
    rev, _ = oracle.voxel_grid(pts[::-1], leaf)
    assert not eq(rev, ref)
    assert E.u32(rev)[0, 3] != E.u32(ref)[0, 3] or not np.array_equal(rev[0, :3], ref[0, :3])
    pts, leaf = E.voxel_case("long-mixed")
    ref, _ = E.voxel_reference(oracle, "long-mixed")
    assert len(pts) == 25000 and len(ref) == 5001
    assert not eq(oracle.voxel_grid(pts[::-1], leaf)[0], ref)


def test_passthrough_edge(oracle):
    below, leaf = E.voxel_case("edge-below")
    past, _ = E.voxel_case("edge-past")
    assert (E.u32(below) != E.u32(past)).sum() == 1  # one coordinate of one point
    assert wrapped_extent_product(below, 1.0) == 46341 * 46340 == 2**31 - 1 - 41707
    assert wrapped_extent_product(past, 1.0) == 46341 * 46341 >= 2**31
    assert E.voxel_params(below, leaf).prod == 46341 * 46340
    assert not E.voxel_reference(oracle, "edge-below")[1]
    out, passthrough = E.voxel_reference(oracle, "edge-past")
    assert passthrough and eq(out, past)


def test_ties_and_duplicates(oracle):
    pts, leaf = E.voxel_case("ties")
    assert leaf == (0.5, 0.5, 0.5) and np.array_equal(pts[:, :3] * 2, np.round(pts[:, :3] * 2))
    z = E.u32(pts)[:, :3]
    assert (z == 0x80000000).any() and (z == 0).any() and (pts[:, :3] < 0).any()
    pts, _ = E.voxel_case("identical")
    assert len(pts) == 1000 and (E.u32(pts) == E.u32(pts)[0]).all()
    assert len(E.voxel_reference(oracle, "identical")[0]) == 1


def test_cloud_frames():
    assert (8192 * 256 + 1, 1, 1) in E.CLOUD_SHAPES
    xyz, bgr = E.cloud_frames(37, 5, 3)
    assert not (bgr == E.SENT).any() and 0.03 < (~np.isfinite(xyz).all(-1)).mean() < 0.1


# ---- display: thresholds ------------------------------------------------------------------------------

@pytest.mark.parametrize("nd", E.NUM_DISP)
def test_gamma_thresholds(oracle, nd):
    """Level v first appears exactly at t[v]: the three floats before it are below v, t[v] and the
    three after it at v or above, for all 255 levels."""
    t = E.gamma_thresholds(oracle, nd)
    assert E.bisect_calls(("g", nd)) <= 31 and (np.diff(t) > 0).all()
    frame = E.gamma_frame(oracle, nd)
    assert frame.shape[1] == E.WIDE > 256
    out = oracle.show_disparity_map(frame, nd).reshape(-1)
    lv = out[:255 * 7].reshape(255, 7).astype(int)
    v = np.arange(1, 256)[:, None]
    assert (lv[:, :3] < v).all() and (lv[:, 3:] >= v).all() and (lv[:, 3] == v[:, 0]).all()
    sp = out[255 * 7:255 * 7 + 9]
    # 0, -0, denormal, nd, 2 nd, +inf (cvRound's integer indefinite saturates to 0), -inf, NaN, -1
    assert sp.tolist() == [0, 0, 0, 255, 255, 0, 0, 0, 0]


def test_depth_thresholds(oracle):
    zr = np.array(E.ZR0)
    frame = E.depth_frame(oracle)
    out = oracle.show_depth_map(frame, zr, E.IDENT)
    assert zr.tolist() == [950.0, 2700.0] == list(E.range_after(E.ZR0))
    assert frame.shape[1] == E.WIDE and E.bisect_calls(("z",) + E.ZR0) <= 31
    lv = out[..., 0].reshape(-1)[2:2 + 255 * 7].reshape(255, 7).astype(int)
    v = np.arange(1, 256)[:, None]
    assert (lv[:, :3] < v).all() and (lv[:, 3:] >= v).all() and (lv[:, 3] == v[:, 0]).all()
    t = E.depth_thresholds(oracle)
    assert Z_in(t[1:]) and E.depth_levels(oracle, t[:1], E.ZR0)[0] == 0


def Z_in(t):
    return bool(((t > E.Z_LO) & (t < E.Z_HI)).all())


# ---- display: addWeighted -----------------------------------------------------------------------------

def f32_ties(alpha, beta, fused=True):
    """The operand pairs (a, b) whose float sum a * alpha + b * beta is an exact .5, as a mask
    [a, b], and the sums: fused as the oracle and the engine evaluate it, fma(a, alpha, b * beta),
    or with both products rounded."""
    a, b = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij")
    t = (b.astype(F32) * F32(beta)).astype(np.float64)
    s = a * np.float64(F32(alpha)) if fused else (a.astype(F32) * F32(alpha)).astype(np.float64)
    r = (s + t).astype(F32).astype(np.float64)  # the sum of the two is exact in double (33 bits)
    return r - np.floor(r) == 0.5, r


def test_add_weighted_ties_exist(oracle):
    """Exact .5 ties, where round-half-to-even decides: 6289 pairs for 0.7 / 0.3 and 630 for
    0.63 / 0.37 in the fused form (6260 and 633 with both products rounded); the oracle rounds each
    of them to the even neighbour."""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for alpha, beta, fused, plain in ((0.7, 0.3, 6289, 6260), (0.63, 1.0 - F32(0.63), 630, 633)):
        m, r = f32_ties(alpha, beta)
        assert int(m.sum()) == fused and int(f32_ties(alpha, beta, False)[0].sum()) == plain
        got = oracle.add_weighted(a.astype(np.uint8), float(F32(alpha)), b.astype(np.uint8), float(F32(beta)))
        even = 2 * np.floor(r / 2 + 0.25)
        assert np.array_equal(got[m], even[m]) and np.array_equal(got[~m], np.round(r[~m]))


def all_pairs(p, q):
    return len(np.unique(p.astype(np.int64).reshape(-1) * 256 + q.reshape(-1))) == 65536


def test_overlay_holds_every_pair(oracle):
    vis, left = E.overlay_pairs()
    lc = oracle.resize_area_half_bgr(left)
    hc = oracle.apply_colormap(vis, E.IDENT)
    yy, xx = np.mgrid[0:256, 0:256]
    for c in range(3):
        assert np.array_equal(lc[..., c], yy) and np.array_equal(hc[..., c], xx)
        assert all_pairs(lc[..., c], hc[..., c])


def test_ema_frames_hold_every_pair(oracle):
    yy, xx = np.mgrid[0:256, 0:256]
    d = E.ema_disp_frames(oracle)
    assert np.array_equal(oracle.show_disparity_map(d[0], 80), yy)
    assert np.array_equal(oracle.show_disparity_map(d[1], 80), xx)
    assert all_pairs(oracle.show_disparity_map(d[0], 80), oracle.show_disparity_map(d[1], 80))
    z = E.ema_depth_frames(oracle)
    zr = np.array(E.ZR0)
    first = oracle.show_depth_map(z[0], zr, E.IDENT)
    second = oracle.show_depth_map(z[1], zr, E.IDENT)  # no EMA: its own levels, second range state
    assert zr.tolist() == list(E.range_after(E.range_after(E.ZR0)))
    for c in range(3):
        assert np.array_equal(first[:256, :, c], yy) and np.array_equal(second[:256, :, c], xx)


# ---- display: compare values ---------------------------------------------------------------------------

def test_compare_frames(oracle):
    x = E.zcmp_frames()
    assert len(x) == 130 > 64 and len(E.ZVALS) == 13
    assert {p[1] for p in E.ZPOS} >= {0, 63, 255, 256} and E.ZPOS[-1] == (1, E.WIDE - 1)
    below, at, above = E.ZVALS[:3]
    assert below < at == 10000 < above and E.ZVALS[4] == 12000
    assert E.ZVALS[8] > 0 and E.ZVALS[8] < np.finfo(F32).tiny == E.ZVALS[9]
    for f in range(130):
        v, p, alone = E.ZVALS[f // 10], E.ZPOS[(f // 2) % 5], f % 2
        z = x[f, ..., 2]
        valid = z[(z > 0) & (z < 10000)]
        want = ([] if alone else [5000.0]) + ([float(v)] if 0 < v < 10000 else [])
        assert sorted(valid.tolist()) == sorted(want)
        zr = np.array(E.ZR0)
        oracle.depth_range_update(x[f], zr)
        lo, hi = (min(want), max(want)) if len(want) == 2 else (1000.0, 2000.0)
        assert zr.tolist() == [0.9 * 1000 + 0.1 * lo, 0.9 * 2000 + 0.1 * hi]
        inside = int(0 <= v <= 12000) + int(not alone)
        for col0 in (0, 80):
            n = inside - int(p[1] < col0 and 0 <= v <= 12000)
            assert oracle.depth_coverage(x[f], col0) == n / 600 * 100
    # what tells z < 10000 from z <= 10000, and z <= 12000 from z < 12000
    zr_at, zr_below = np.array(E.ZR0), np.array(E.ZR0)
    oracle.depth_range_update(x[10], zr_at)
    oracle.depth_range_update(x[0], zr_below)
    assert zr_at[1] != zr_below[1]


def test_many_frames_and_clamps(oracle):
    x = E.many_frames()
    assert x.shape == (70, 3, 90, 3)
    z = x[..., 2]
    nvalid = ((z > 0) & (z < 10000)).reshape(70, -1).sum(1)
    assert nvalid[5] == 0 and nvalid[40] == 0 and nvalid[20] == 1 and (nvalid > 1).sum() == 67
    cov = [oracle.depth_coverage(x[f], 80) for f in range(70)]
    assert cov[64:] != cov[:6] and len(set(cov[64:])) > 1  # reading the first chunk of 64 again shows
    for (state, (lo, hi)) in E.CLAMP_STATES:
        zr = np.array(state)
        oracle.depth_range_update(E.clamp_frame(lo, hi), zr)
        free = (0.9 * state[1] + 0.1 * hi)
        assert zr[1] == zr[0] + 1.0 and zr[1] != free  # the zmin + 1 clamp decided the maximum
    assert oracle.depth_coverage(E.coverage_frame(65, 2), 65) == 0  # col0 >= W: no column left
