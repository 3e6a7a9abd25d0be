"""GPU: the census kernels (csrc/sdr_census.hip: k_census, k_cost_census<NR, K>) at every
instantiation and input edge, bit-exact against the numpy pin (tests/census_ref.py).  The cases and
what each reaches are tests/census_cases.py; tests/test_census_cases_cpu.py shows, on the pin alone,
that they reach it and that they tell a wrong formula from the right one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import census_cases as C  # noqa: E402
import census_ref as CR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from conftest import hyp_examples  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.sgbm import set_handle_stream  # noqa: E402
from test_gpu_path_records import path_rec_env  # noqa: E402

CENSUS = sdr.COST_CENSUS


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


# ---- the transform ------------------------------------------------------------------------

def compute_in_layout(m, Ls, Rs, layout):
    """The matcher's device entry on frames laid out as census_cases.transform_layout says, in a
    buffer of random bytes (so padding that is read shows); returns the maps [F][H][W]."""
    F, H, W = Ls.shape
    F_, stride, fstride, offL, offR, nbytes = C.transform_layout(H, W, layout)
    assert F == F_
    buf = np.random.default_rng(H * W).integers(0, 256, nbytes + 8, dtype=np.uint8)
    for off, imgs in ((offL, Ls), (offR, Rs)):
        np.lib.stride_tricks.as_strided(buf[off:], (F, H, W), (fstride, stride, 1))[...] = imgs
    flat = torch.from_numpy(buf).to(dev())
    out = torch.empty((F, H, W), dtype=torch.int16, device=dev())
    set_handle_stream(m._h, 0)
    check(lib().sdr_sgbm_compute_device(m._h, flat.data_ptr() + offL, flat.data_ptr() + offR, W, H, stride, fstride,
                                        F, out.data_ptr(), W, W * H))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name,H,W,layout", C.TRANSFORM_SHAPES, ids=[s[0] for s in C.TRANSFORM_SHAPES])
def test_transform_equals_the_pin(name, H, W, layout):
    """Stage 7, the descriptors of both roles of every frame, at D = 16, blockSize 1 (no size of
    the table is refused: the plan's only height limit is the 2 GiB one)."""
    F = C.transform_layout(H, W, layout)[0]
    m = sdr.StereoSGBM.create(0, 16, 1, 2, 12, 1, 0, 12, 0, 0, 0, cost=CENSUS)
    for kind in C.TRANSFORM_KINDS:
        frames = [C.pair(kind, H, W, 16, seed=31 * f + W) for f in range(F)]
        Ls, Rs = np.stack([p[0] for p in frames]), np.stack([p[1] for p in frames])
        compute_in_layout(m, Ls, Rs, layout)
        T = m.debug_stage(7, (F, 2, H, W), np.uint64)
        for f in range(F):
            assert np.array_equal(T[f, 0], CR.census_9x7(Ls[f])), (kind, f, "left")
            assert np.array_equal(T[f, 1], CR.census_9x7(Rs[f])), (kind, f, "right")
    m.close()


# ---- the cost volume ----------------------------------------------------------------------

def compute_frames(m, pairs):
    """One frame through the host entry, several as a device batch."""
    if len(pairs) == 1:
        return m.compute(*pairs[0])[None]
    Ld = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev())
    Rd = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev())
    out = m.compute(Ld, Rd)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("c", C.COST_CASES, ids=lambda c: c.id)
def test_cost_volume_equals_the_pin_in_every_mode(c):
    """Stage 0 of every frame under all four modes (3WAY's is the frame-level volume).  Before each
    compute the handle runs the swapped pair, so a cell the kernel does not write holds another
    volume's value and not the one expected."""
    pairs = C.cost_pairs(c)
    swapped = [(R, L) for L, R in pairs]
    m = sdr.StereoSGBM.create(*C.create_args(c), cost=CENSUS)
    ref = {}
    for mode in C.MODES:
        m.setMode(mode)
        compute_frames(m, swapped)
        compute_frames(m, pairs)
        vol = m.debug_stage(0, (c.F, c.H, c.W1, c.D), np.int16)
        hh = mode in (C.SGM_HH, C.SGM_HH4)
        for f, (L, R) in enumerate(pairs):
            if (hh, f) not in ref:
                ref[hh, f] = CR.census_cost_volume(L, R, c.minD, c.D, c.bs, c.P2, mode)
            bad = vol[f] != ref[hh, f]
            assert not bad.any(), f"mode {mode} frame {f}: {bad.sum()} cells differ, first {np.argwhere(bad)[0]}"
            if c.kind == "ramps":  # the closed form does not depend on the pin
                value, mask = C.ramps_closed_form(c.H, c.W, c.minD, c.D, c.bs, c.P2, mode)
                assert mask.any() and (vol[f][mask] == value).all(), mode
    m.close()


# ---- MODE_SGBM_3WAY's stripe-start rows ---------------------------------------------------

@pytest.mark.parametrize("c", C.STRIPE_CASES, ids=lambda c: c.id)
def test_stripe_start_rows_and_maps(c):
    """Stage 6's defined rows (band s, rows [0, aux_rows)), the final map and the LR-checked one."""
    L, R = C.pair(c.kind, c.H, c.W, c.D, seed=c.H)
    args = C.create_args(c)
    m = sdr.StereoSGBM.create(*args, nstripes=c.ns, cost=CENSUS)
    m.compute(R, L)
    got = m.compute(L, R)
    rows, (nstr, amax) = C.stripe_rows_ref(L, R, 0, c.D, c.bs, c.P2, c.ns)
    if amax:
        aux = m.debug_stage(6, (nstr, amax, c.W1, c.D), np.int16)
        for s, ref in rows:
            bad = aux[s, :len(ref)] != ref
            assert not bad.any(), f"stripe {s}: {bad.sum()} cells differ, first {np.argwhere(bad)[0]}"
    else:
        assert not rows
    ref = C.sgm_of(L, R, args, nstripes=c.ns)
    assert np.array_equal(got, ref), f"{(got != ref).sum()} px differ"
    assert np.array_equal(m.debug_stage(2, (c.H, c.W), np.int16), C.sgm_of(L, R, args, stages=0, nstripes=c.ns))
    m.close()


# ---- end to end ---------------------------------------------------------------------------
NCHUNKS = 6
RANDOM = C.random_cases(hyp_examples(48), seed=2026)


@pytest.mark.parametrize("chunk", range(NCHUNKS))
def test_random_cases_bit_exact(chunk):
    """The seeded survey over the census domain (48 cases, times SDR_HYP_SCALE), in chunks: the
    final map and the LR-checked map, nstripes and uniq_rule on both sides."""
    for c in RANDOM[chunk::NCHUNKS]:
        L, R = C.pair(c.kind, c.H, c.W, c.D, seed=c.seed)
        args = C.random_args(c)
        m = sdr.StereoSGBM.create(*args, nstripes=c.nstripes, uniq_rule=c.uniq_rule, cost=CENSUS)
        got = m.compute(L, R)
        ref = C.sgm_of(L, R, args, nstripes=c.nstripes, uniq_rule=c.uniq_rule)
        assert np.array_equal(got, ref), f"{vars(c)}: {(got != ref).sum()} px differ"
        raw = m.debug_stage(2, (c.H, c.W), np.int16)
        assert np.array_equal(raw, C.sgm_of(L, R, args, stages=0, nstripes=c.nstripes, uniq_rule=c.uniq_rule)), vars(c)
        m.close()


def test_both_record_formats_on_ties():
    """D 128, MODE_SGBM, P2 = 4095: the 12-bit path-cost records and the int16 ones (a matcher
    created under SDR_PATH_REC=16) give the pin's maps on a census volume of ties."""
    H, D = 24, 128
    W = D + 70
    L, R = C.pair("ties", H, W, D, seed=5)
    args = (0, D, 5, 50, 4095, 1, 0, 12, 0, 0, 0)
    ref, ref_lr = C.sgm_of(L, R, args), C.sgm_of(L, R, args, stages=0)
    recs = []
    for rec16 in (False, True):
        with path_rec_env("16" if rec16 else None):
            m = sdr.StereoSGBM.create(*args, cost=CENSUS)
        got = m.compute(L, R)
        assert np.array_equal(got, ref), f"rec16={rec16}: {(got != ref).sum()} px differ"
        assert np.array_equal(m.debug_stage(2, (H, W), np.int16), ref_lr), f"rec16={rec16}"
        recs.append(m.debug_stage(4, (H * (W - D) * 4 * (D * 3 // 4),), np.int16))
        m.close()
    assert not np.array_equal(recs[0], recs[1])  # the two matchers did write different formats


def test_paired_class_path_roles_and_volume():
    """StereoDisparity(Q, cost=COST_CENSUS) runs both matchers as one batch of two frames on the
    left matcher's handle; frame 1 takes the images swapped (k_census's swap = f >= split, the cost
    kernel's frame_geom): its descriptors are [T(R), T(L)] and its volume the right matcher's."""
    Lf, Rf, _ = S.make_pair(48, 360, 160, seed=77)
    bl, br = np.repeat(Lf[:, :, None], 3, 2), np.repeat(Rf[:, :, None], 3, 2)
    sd = sdr.StereoDisparity(S.REFERENCE_Q, cost=CENSUS)
    sd.computeDisparity(bl, br)
    sl = sdr.resize_area_half(sdr.cvt_bgr2gray(torch.from_numpy(bl).to(dev()))).cpu().numpy()
    sr = sdr.resize_area_half(sdr.cvt_bgr2gray(torch.from_numpy(br).to(dev()))).cpu().numpy()
    h, w = sl.shape
    W1 = w - 80
    T = sd.matcher.debug_stage(7, (2, 2, h, w), np.uint64)
    TL, TR = CR.census_9x7(sl), CR.census_9x7(sr)
    assert not np.array_equal(TL, TR)
    assert np.array_equal(T[0, 0], TL) and np.array_equal(T[0, 1], TR)
    assert np.array_equal(T[1, 0], TR) and np.array_equal(T[1, 1], TL)
    vol = sd.matcher.debug_stage(0, (2, h, W1, 80), np.int16)
    assert np.array_equal(vol[0], CR.census_cost_volume(sl, sr, 0, 80, 5, 2400, C.SGM_3WAY))
    assert np.array_equal(vol[1], CR.census_cost_volume(sr, sl, -79, 80, 5, 2400, C.SGM_3WAY))


# ---- the row bands ------------------------------------------------------------------------

@pytest.mark.parametrize("nr,k", C.BAND_KERNELS, ids=[f"k_{nr}_{k}" for nr, k in C.BAND_KERNELS])
def test_cost_volume_under_every_band_class(nr, k):
    """k_cost_census<NR, K> with the band height of every class of census_cases.BAND_CLASSES, set
    through SDR_DEBUG_COST_ROWS: the volume equals the pin and the one the launcher's own band
    height computes, and sdr_sgbm_last_plan reports the bands that ran."""
    for c in [c for c in C.BAND_CASES if (c.bs, C.kernel_of(c.bs, c.D)[1]) == (nr, k)]:
        pairs = C.cost_pairs(c)
        swapped = [(R, L) for L, R in pairs]
        m = sdr.StereoSGBM.create(*C.create_args(c), cost=CENSUS)
        for mode in (c.mode, C.SGM_3WAY if C.is_hh(c.mode) else C.SGM_HH):
            m.setMode(mode)
            vols = []
            for ty in (c.ty, 0):
                m.set_debug_knob(sdr.sgbm.DEBUG_COST_ROWS, ty)
                compute_frames(m, swapped)
                compute_frames(m, pairs)
                plan = m.last_plan()
                rows = plan["cost_rows"]
                assert plan["cost"] == ("census", nr, k, 1) and (rows == ty if ty else rows >= 4), (c.id, plan)
                assert plan["cost_bands"] == (c.H + rows - 1) // rows, (c.id, plan)
                vols.append(m.debug_stage(0, (1, c.H, c.W1, c.D), np.int16)[0])
            ref = CR.census_cost_volume(*pairs[0], c.minD, c.D, c.bs, c.P2, mode)
            bad = vols[0] != ref
            assert not bad.any(), f"{c.id} mode {mode}: {bad.sum()} cells differ, first {np.argwhere(bad)[0]}"
            assert np.array_equal(vols[0], vols[1]), (c.id, mode)
        m.close()
