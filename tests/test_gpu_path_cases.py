"""Every k_paths / k_paths_tc / k_south_wta instantiation and every k_sweep16 family, stage by
stage and bit for bit (tests/path_cases.py; the table and its references are pinned without a GPU
by test_path_cases_cpu.py).

Per case: set SDR_DEBUG_PLAN_CUS, compute, assert that sdr_sgbm_last_plan names the kernels the
case exists for, then compare stage 0 (cost volume) with the oracle, stage 4 (every direction's
path costs, int16 or decoded 12-bit e = C - L) with the numpy volumes, stage 1 (WTA map, matched
columns) and stage 5 (right-view keys) with the numpy WTA, and stage 2 and the final map with the
oracle.  Where a shape has both column forms the same handle runs it again with the knob flipped:
stage 1, stage 5 and the final map must not move.
"""
import numpy as np
import pytest

import path_cases as P
import stereo_depth_ruler_amd as sdr
from stereo_depth_ruler_amd._lib import sgbm_plan
from stereo_depth_ruler_amd.sgbm import DEBUG_PLAN_CUS

NATURAL_NAMES = [c.name for c in P.natural_cases(256)]  # the names do not depend on the CU count


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def run(torch, m, c, knob):
    """One compute of the case's frames under the knob -> (plan, {stage: array of all frames})."""
    m.set_debug_knob(DEBUG_PLAN_CUS, knob)
    fr = P.frames(c)
    Ld = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    Rd = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    out = m.compute(Ld, Rd)
    torch.cuda.synchronize()
    plan = m.last_plan()
    F, H, W, W1, D = c.F, c.H, c.W, c.W1, c.D
    nrec = 3 if plan["south"][0] == "sweep" else P.NP_OF[c.mode]
    got = {"final": out.cpu().numpy(), 0: m.debug_stage(0, (F, H, W1, D), np.int16),
           1: m.debug_stage(1, (F, H, W), np.int16), 2: m.debug_stage(2, (F, H, W), np.int16),
           5: m.debug_stage(5, (F, H, W), np.uint32),
           4: m.debug_stage(4, (F, H, W1, nrec, D), np.int16)}  # frames nrec*H*W1*D*2 bytes apart
    return plan, got


def path_costs(c, plan, rec, f, C):
    """Frame f's stage 4 as path costs [H][W1][R][D]: the int16 records themselves, or C - e of the
    12-bit ones (which fill the first 3/4 of the frame's span)."""
    if not plan["paths"][3]:
        return rec[f]
    nrec = rec.shape[3]
    n = c.H * c.W1 * nrec * c.D * 3 // 4  # int16 elements
    e = P.decode_rec12(rec[f].reshape(-1)[:n].view(np.uint32), c.H, c.W1, nrec, c.D)
    assert 0 <= e.min() and e.max() <= c.P2
    return (C.astype(np.int64)[:, :, None, :] - e).astype(np.int16)


def check_frame(oracle, c, plan, got, f, staged=True):
    """Frame f against the oracle and (staged) every stage of the numpy reference."""
    L, R = P.frames(c)[f]
    p = oracle.make_params(*c.args, **c.kwargs)
    m0 = c.minX1
    assert np.array_equal(got[0][f], oracle.cost_volume(L, R, p)), f"{c.name} frame {f}: stage 0"
    if staged:
        r = P.reference(c, f)
        L4 = path_costs(c, plan, got[4], f, got[0][f])
        for q in range(r.recs.shape[2]):
            bad = L4[:, :, q] != r.recs[:, :, q]
            assert not bad.any(), (f"{c.name} frame {f}: stage 4 record {q}: {bad.sum()} values differ, first at "
                                   f"(y, x, d) = {tuple(np.argwhere(bad)[0])}")
        bad = got[1][f][:, m0:m0 + c.W1] != r.raw[:, m0:m0 + c.W1]
        assert not bad.any(), f"{c.name} frame {f}: stage 1: {bad.sum()} px, first at {tuple(np.argwhere(bad)[0])}"
        bad = got[5][f] != r.keys
        assert not bad.any(), f"{c.name} frame {f}: stage 5: {bad.sum()} keys, first at {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(got[2][f], oracle.sgbm_compute(L, R, p, stages=0)), f"{c.name} frame {f}: stage 2"
    assert np.array_equal(got["final"][f], oracle.sgbm_compute(L, R, p)), f"{c.name} frame {f}: final map"


def same_maps(c, a, b, what):
    m0 = c.minX1
    assert np.array_equal(a[1][:, :, m0:m0 + c.W1], b[1][:, :, m0:m0 + c.W1]), f"{c.name}: stage 1 {what}"
    assert np.array_equal(a[5], b[5]), f"{c.name}: stage 5 {what}"
    assert np.array_equal(a["final"], b["final"]), f"{c.name}: final map {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("c", P.CASES, ids=[c.name for c in P.CASES])
def test_path_case(gpu, oracle, c):
    m = sdr.StereoSGBM.create(*c.args, **c.kwargs)
    plan, got = run(gpu, m, c, c.knob)
    assert (plan["paths"], plan["south"]) == c.plan_key()
    if c.tiles:
        (sd, td), (su, tu) = plan["sweep_shape"]
        assert (td, tu) == c.tiles and sd >= 1 and su >= 1
    check_frame(oracle, c, plan, got, 0)
    for f in range(1, c.F):
        check_frame(oracle, c, plan, got, f, staged=False)
    if c.flip:
        plan2, got2 = run(gpu, m, c, c.flip)
        assert plan2["south"][4] != plan["south"][4], "the flipped knob runs the other column form"
        same_maps(c, got, got2, "under the flipped knob")
    m.close()


@pytest.mark.gpu
def test_knob_never_reaches_the_sweep(gpu, oracle):
    """SDR_DEBUG_PLAN_CUS moves the chain-count thresholds alone: under it a batch sweeps with the
    tiling the device's own compute units give, and computes the same maps."""
    c = P.BY_NAME["sweep-D16-w41"]
    m = sdr.StereoSGBM.create(*c.args, **c.kwargs)
    plan, got = run(gpu, m, c, 0)
    for knob in (P.KNOB_TC, P.KNOB_ONE):
        plan2, got2 = run(gpu, m, c, knob)
        assert plan2["south"] == plan["south"] and plan2["sweep_shape"] == plan["sweep_shape"]
        assert plan2["cus"] == knob
        same_maps(c, got, got2, f"under knob {knob}")
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NATURAL_NAMES)
def test_natural_dispatch(gpu, oracle, name):
    """No knob: a batch whose column chains pass 8 x CUs takes the two-column kernels by itself,
    one frame fewer does not.  Every frame equals its own single-frame run; frames 0, a middle one
    and the last equal the oracle, frame 0 at every stage."""
    cus = sgbm_plan(P.BY_NAME["one-D16-np4"].params(), 64, 8)["cus"]
    c = {n.name: n for n in P.natural_cases(cus)}[name]
    assert c.south[4] == (c.F == 8)
    m = sdr.StereoSGBM.create(*c.args, **c.kwargs)
    plan, got = run(gpu, m, c, 0)
    assert (plan["paths"], plan["south"], plan["cus"]) == (c.paths, c.south, cus)
    check_frame(oracle, c, plan, got, 0)
    for f in (c.F // 2, c.F - 1):
        check_frame(oracle, c, plan, got, f, staged=False)
    one = P.Case(c.name, c.mode, c.D, c.H, c.W1, c.paths, c.south, F=1)
    fr = P.frames(c)
    for f in range(c.F):
        Ld, Rd = (gpu.from_numpy(a[None]).cuda() for a in fr[f])
        out = m.compute(Ld, Rd)
        gpu.cuda.synchronize()
        assert not m.last_plan()["south"][4], "a single frame of these shapes stays on one column"
        single = {"final": out.cpu().numpy(), 1: m.debug_stage(1, (1, c.H, c.W), np.int16),
                  5: m.debug_stage(5, (1, c.H, c.W), np.uint32)}
        same_maps(one, {k: v[f:f + 1] for k, v in got.items()}, single, f"of frame {f} against its own run")
    m.close()
