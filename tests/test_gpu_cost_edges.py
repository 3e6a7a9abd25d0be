"""GPU: the BT prefilter and cost kernels (csrc/sdr_cost.hip: k_prefilter; sdr_cost_kernel.hpp:
k_cost<NR, K, CN>; sdr_cost_generic.hip) at every instantiation, row band and input edge, bit-exact
against the numpy pin (tests/numpy_ref.py through tests/cost_cases.py).  The cases and what each
reaches are tests/cost_cases.py; tests/test_cost_cases_cpu.py shows, on the pin alone, that they
reach it and that they tell a wrong formula from the right one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cost_cases as C  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import check, lib  # noqa: E402
from stereo_depth_ruler_amd.sgbm import DEBUG_COST_ROWS, SDRError, set_handle_stream  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev():
    return torch.device("cuda", 0)


def compute_frames(m, pairs):
    """One frame through the host entry, several as a device batch (gray or colour)."""
    if len(pairs) == 1:
        return m.compute(*pairs[0])[None]
    Ld = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev())
    Rd = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev())
    out = m.compute(Ld, Rd)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_equal(got, ref, what):
    bad = got != ref
    assert not bad.any(), f"{what}: {bad.sum()} cells differ, first {np.argwhere(bad)[0]}"


# ---- the cost volume ----------------------------------------------------------------------

@pytest.mark.parametrize("c", C.COST_CASES, ids=lambda c: c.id)
def test_cost_volume_equals_the_pin(c):
    """Stage 0 of every frame under the entry's mode and a mode of the other hh_bottom class, with
    the entry's band height set through SDR_DEBUG_COST_ROWS.  Before each compute the handle runs
    the swapped pair, so a cell the kernel does not write holds another volume's value and not the
    one expected.  sdr_sgbm_last_plan names the kernel and the bands that ran."""
    pairs = C.cost_pairs(c)
    swapped = [(R, L) for L, R in pairs]
    m = sdr.StereoSGBM.create(*C.create_args(c))
    kernel = C.kernel_of(c.bs, c.D, c.cn)
    for mode in (c.mode, C.other_hh_mode(c.mode)):
        m.setMode(mode)
        m.set_debug_knob(DEBUG_COST_ROWS, c.ty)
        compute_frames(m, swapped)
        compute_frames(m, pairs)
        plan = m.last_plan()
        assert plan["cost"] == kernel, mode
        if kernel[0] == "generic":
            assert (plan["cost_rows"], plan["cost_bands"]) == (0, 0)
        else:
            rows = plan["cost_rows"]
            assert rows == c.ty if c.ty else rows >= 4, plan
            assert plan["cost_bands"] == (c.H + rows - 1) // rows
        vol = m.debug_stage(0, (c.F, c.H, c.W1, c.D), np.int16)
        for f, (L, R) in enumerate(pairs):
            assert_equal(vol[f], C.pin_of(c, f, mode), f"mode {mode} frame {f}")
            if c.kind == "const":  # the closed form does not depend on the pin
                value, mask, frozen = C.const_closed_form(C.const_levels(L, R), c.H, c.W, c.minD, c.D, c.bs, c.P2, mode)
                assert mask.any() and (vol[f][mask] == value).all() and (vol[f][frozen] == c.P2).all(), mode
        if c.ty:
            # the launcher's own band height computes the same volume
            m.set_debug_knob(DEBUG_COST_ROWS, 0)
            compute_frames(m, swapped)
            compute_frames(m, pairs)
            own = m.last_plan()
            assert own["cost"] == kernel and own["cost_rows"] >= 4 and \
                own["cost_bands"] == (c.H + own["cost_rows"] - 1) // own["cost_rows"]
            assert_equal(m.debug_stage(0, (c.F, c.H, c.W1, c.D), np.int16), vol, f"mode {mode}: knob 0 against {c.ty}")
    m.close()


# ---- MODE_SGBM_3WAY's stripe-start rows ---------------------------------------------------

@pytest.mark.parametrize("c", C.STRIPE_CASES, ids=lambda c: c.id)
def test_stripe_start_rows_and_maps(oracle, c):
    """Stage 6's defined rows (band s, rows [0, aux_rows)), the final map and the LR-checked one."""
    L, R = C.stripe_pair(c)
    args = C.create_args(c)
    m = sdr.StereoSGBM.create(*args, nstripes=c.ns)
    m.compute(R, L)
    got = m.compute(L, R)
    assert m.last_plan()["cost"] == C.kernel_of(c.bs, c.D, c.cn)
    rows, (nstr, amax) = C.stripe_rows_ref(L, R, c)
    if amax:
        aux = m.debug_stage(6, (nstr, amax, c.W1, c.D), np.int16)
        for s, ref in rows:
            assert_equal(aux[s, :len(ref)], ref, f"stripe {s}")
    else:
        assert not rows
    assert_equal(m.debug_stage(0, (c.H, c.W1, c.D), np.int16), C.pin_volume(L, R, c.minD, c.D, c.bs, c.P2, c.cap, c.mode),
                 "stage 0")
    p = oracle.make_params(*args, nstripes=c.ns)
    assert_equal(got, oracle.sgbm_compute(L, R, p), "final map")
    assert_equal(m.debug_stage(2, (c.H, c.W), np.int16), oracle.sgbm_compute(L, R, p, stages=0), "LR-checked map")
    m.close()


# ---- the prefilter ------------------------------------------------------------------------

def compute_in_layout(m, Ls, Rs, cn, layout):
    """The matcher's device entry on frames laid out as census_cases.transform_layout says (in bytes
    of a row of W * cn), in a buffer of random bytes, so padding that is read shows."""
    F, H, W = Ls.shape[:3]
    F_, stride, fstride, offL, offR, nbytes = C.transform_layout(H, W * cn, layout)
    assert F == F_
    buf = np.random.default_rng(H * W).integers(0, 256, nbytes + 8, dtype=np.uint8)
    for off, imgs in ((offL, Ls), (offR, Rs)):
        np.lib.stride_tricks.as_strided(buf[off:], (F, H, W * cn), (fstride, stride, 1))[...] = imgs.reshape(F, H, W * cn)
    flat = torch.from_numpy(buf).to(dev())
    out = torch.empty((F, H, W), dtype=torch.int16, device=dev())
    set_handle_stream(m._h, 0)
    check(lib().sdr_sgbm_compute_device_cn(m._h, flat.data_ptr() + offL, flat.data_ptr() + offR, W, H, cn, stride,
                                           fstride, F, out.data_ptr(), W, W * H))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,H,W,cn,layout,cap", C.PREFILTER_SHAPES, ids=[s[0] for s in C.PREFILTER_SHAPES])
def test_prefilter_operands_equal_the_pin(name, H, W, cn, layout, cap):
    """Stages 8 and 9, the operands of both roles of every frame, at D = 16, blockSize 1."""
    F = C.transform_layout(H, W * cn, layout)[0]
    ft = C.ftzero_of(cap)
    m = sdr.StereoSGBM.create(0, 16, 1, 1, 2, 1, cap, 12, 0, 0, 0)
    for kind in C.PREFILTER_KINDS:
        Ls, Rs = C.prefilter_frames(kind, H, W, cn, F)
        compute_in_layout(m, Ls, Rs, cn, layout)
        assert m.last_plan()["cost"] == ("k_cost", 1, 1, cn)
        s8 = m.debug_stage(8, (F, H, W, 3 * cn), np.uint32)
        s9 = m.debug_stage(9, (F, 3 * cn, H, W), np.uint64)
        for f in range(F):
            assert_equal(s8[f], C.stage8_pin(Ls[f], ft), f"{kind} frame {f} stage 8")
            assert_equal(s9[f], C.stage9_pin(Rs[f], ft), f"{kind} frame {f} stage 9")
    m.close()


def test_paired_class_path_roles_operands_and_volume():
    """StereoDisparity(Q) runs both matchers as one batch of two frames on the left matcher's
    handle; frame 1 takes the images swapped (k_prefilter's swap = f >= split, the cost kernel's
    frame_geom): its left pack is the right image's, its pair planes the left image's, and its
    volume the right matcher's."""
    Lf, Rf, _ = S.make_pair(48, 360, 160, seed=77)
    bl, br = np.repeat(Lf[:, :, None], 3, 2), np.repeat(Rf[:, :, None], 3, 2)
    sd = sdr.StereoDisparity(S.REFERENCE_Q)
    sd.computeDisparity(bl, br)
    sl = sdr.resize_area_half(sdr.cvt_bgr2gray(torch.from_numpy(bl).to(dev()))).cpu().numpy()
    sr = sdr.resize_area_half(sdr.cvt_bgr2gray(torch.from_numpy(br).to(dev()))).cpu().numpy()
    h, w = sl.shape
    W1 = w - 80
    assert sd.matcher.last_plan()["cost"] == ("k_cost", 5, 1, 1)
    s8 = sd.matcher.debug_stage(8, (2, h, w, 3), np.uint32)
    s9 = sd.matcher.debug_stage(9, (2, 3, h, w), np.uint64)
    assert not np.array_equal(C.stage8_pin(sl, 63), C.stage8_pin(sr, 63))
    assert_equal(s8[0], C.stage8_pin(sl, 63), "frame 0 stage 8")
    assert_equal(s8[1], C.stage8_pin(sr, 63), "frame 1 stage 8")
    assert_equal(s9[0], C.stage9_pin(sr, 63), "frame 0 stage 9")
    assert_equal(s9[1], C.stage9_pin(sl, 63), "frame 1 stage 9")
    vol = sd.matcher.debug_stage(0, (2, h, W1, 80), np.int16)
    assert_equal(vol[0], C.pin_volume(sl, sr, 0, 80, 5, 2400, 63, C.SGM_3WAY), "frame 0 stage 0")
    assert_equal(vol[1], C.pin_volume(sr, sl, -79, 80, 5, 2400, 63, C.SGM_3WAY), "frame 1 stage 0")


# ---- refusals -----------------------------------------------------------------------------

def test_stages_8_and_9_are_an_error_after_a_census_compute():
    L, R = C.pair("noise", 12, 40, 16, seed=1)
    m = sdr.StereoSGBM.create(0, 16, 3, 18, 108, 1, 15, 12, 0, 0, 0, cost=sdr.COST_CENSUS)
    m.compute(L, R)
    for stage, shape, dt in ((8, (12, 40, 3), np.uint32), (9, (3, 12, 40), np.uint64)):
        with pytest.raises(SDRError) as e:
            m.debug_stage(stage, shape, dt)
        assert e.value.code == -1 and "census" in str(e.value)
    m.setCostType(sdr.COST_BT)
    m.compute(L, R)
    assert_equal(m.debug_stage(8, (12, 40, 3), np.uint32), C.stage8_pin(L, 15), "stage 8")
    assert_equal(m.debug_stage(9, (3, 12, 40), np.uint64), C.stage9_pin(R, 15), "stage 9")
    with pytest.raises(SDRError):  # more than the last compute's planes hold
        m.debug_stage(8, (13, 40, 3), np.uint32)
    with pytest.raises(SDRError):
        m.debug_stage(7, (2, 12, 40), np.uint64)  # and the descriptors are gone
    m.close()
