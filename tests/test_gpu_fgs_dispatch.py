"""Every dispatch branch of the sequential FGS solver (SDR_FGS_THOMAS, the default), bit for bit
against the oracle (oracle/wls_oracle.c fgs_line): no tolerance anywhere.

The dispatch plan (sdr_fgs_seq.hip fgs_plan) picks k_fgs_lr<L> from the line length (L = 16 only
with SDR_FGS_LR_MAXL=16, 8 up to 768 samples, 4 up to 1536, 2 up to 3072, k_fgs_th beyond), gives
each coefficient job its own L (16 / 8 / 4) or sends all of them to k_fgs_th when one line is past
1536 samples, and picks k_fgs_th<TWO, LPB> by how many line-frames the chip holds.  Each
instantiation has its own LDS layout, chunk length, DMA piece sizes and tiny-quotient redo, so
each is run here as rows and as columns, through fastGlobalSmootherFilter (the pack-kernel entry,
a stack of 2) and through DisparityWLSFilter.filter (the in_transposed entry), at (lambda, sigma) =
(8000, 1.1) and (50, 5.0), on inputs that reach both division forms (tests/fgs_cases.py).

Every case FIRST asserts, through sdr_fgs_plan_query (the launchers' own code), that it reaches the
instantiation it is named for: a later change of the thresholds fails here instead of silently
moving the coverage.  The smallest shapes reaching each instantiation are in fgs_cases.py's case
lists; test_fgs_dispatch_cpu.py checks the plans and the inputs without a GPU.

The knob-selected instantiations (k_fgs_lr<16>; k_fgs_th<true, LPB> on short lines) run in one
fresh child process each (the knobs are read once): tests/fgs_dispatch_child.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fgs_cases as C  # noqa: E402
from stereo_depth_ruler_amd._lib import fgs_plan  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ids(cases):
    return [C.case_id(c) for c in cases]


def _run(oracle, case):
    errs = C.run_case(oracle, case)
    assert not errs, errs


@pytest.mark.parametrize("case", C.LR4, ids=_ids(C.LR4))
def test_lr4(oracle, case):
    """k_fgs_lr<4> and k_fgs_lrjob on 4 lines: 769 .. 1536 samples (1280- and 1920-wide WLS)."""
    _run(oracle, case)


@pytest.mark.parametrize("case", C.LR2, ids=_ids(C.LR2))
def test_lr2(oracle, case):
    """k_fgs_lr<2> passes with k_fgs_th jobs: 1537 .. 3072 samples (half-4K WLS)."""
    _run(oracle, case)


@pytest.mark.parametrize("case", C.TH_PAST, ids=_ids(C.TH_PAST))
def test_th_past_lr(oracle, case):
    """3073 samples, one past k_fgs_lr<2>: k_fgs_th<true, 16> passes, k_fgs_th jobs."""
    _run(oracle, case)


@pytest.mark.parametrize("case", C.LR8, ids=_ids(C.LR8))
def test_lr8_edges(oracle, case):
    """k_fgs_lr<8> and k_fgs_lrjob on 8 lines at their ends: 385, 767, 768 samples."""
    _run(oracle, case)


@pytest.mark.parametrize("case", C.STACK3, ids=_ids(C.STACK3))
def test_stack_of_three(oracle, case):
    """One pair (k_fgs_lr<4>) and a single image (k_fgs_th<false, 16>) in one call."""
    single = fgs_plan(case["w"], case["h"], 1, 1)
    assert single["row_pass"] == single["col_pass"] == ("th", 16), single
    _run(oracle, case)


@pytest.mark.parametrize("case", C.MIXED, ids=_ids(C.MIXED))
def test_mixed_job_launches(oracle, case):
    """k_fgs_lrjob with the row jobs and the column jobs on 16, 8 or 4 lines each, all nine
    pairings in one launch; and the launches a 1600-sample row sends to k_fgs_th."""
    _run(oracle, case)


@pytest.mark.parametrize("case", C.SINGLE, ids=_ids(C.SINGLE))
def test_single_image_th_lines(oracle, case):
    """k_fgs_th<false, 32> and <false, 64>: 4200 and 8300 lines of one image (the query asks the
    device for its compute units: 256 on the MI355X)."""
    _run(oracle, case)


@pytest.mark.parametrize("H,W", [(9, 1116), (1100, 25)])
def test_device_batch_equals_frames(oracle, H, W):
    """sdr_wls_filter_device on F = 3 frames (blockIdx.y = frame in k_fgs_lr<4> and k_fgs_lrjob)
    equals the frames filtered one at a time, and the oracle."""
    rw = W - 16
    plan = fgs_plan(rw, H, 3, 2)
    axis = "row" if rw > H else "col"
    assert plan[f"{axis}_pass"] == ("lr", 4) and plan[f"{axis}_job"] == ("lrjob", 4), plan
    ins = [C.wls_inputs(oracle, H, rw, 8000.0, 1.1, plan, seed=s) for s in (1, 2, 3)]
    q = ins[0][3]
    for g, _, _, _ in ins:
        assert not C.check_inputs(oracle, g[:, 16:], 8000.0, 1.1, plan)
    dev = torch.device("cuda", 0)
    g = torch.from_numpy(np.stack([i[0] for i in ins])).to(dev)
    dl = torch.from_numpy(np.stack([i[1] for i in ins])).to(dev)
    dr = torch.from_numpy(np.stack([i[2] for i in ins])).to(dev)
    f = C.make_filter(q, W, H)
    out = f.filter(dl, g, dr)
    conf = f.getConfidenceMap()
    torch.cuda.synchronize()
    out, conf = out.cpu().numpy(), conf.cpu().numpy()
    for i, (gi, a, b, _) in enumerate(ins):
        one = f.filter(a, gi, b)
        assert np.array_equal(out[i], one), i
        assert np.array_equal(C.bits(conf[i]), C.bits(f.getConfidenceMap())), i
        ref, ref_conf = oracle.wls_filter(a, b, gi, q, return_conf=True)
        assert np.array_equal(out[i], ref), i
        assert np.array_equal(C.bits(conf[i]), C.bits(ref_conf)), i


@pytest.mark.parametrize("group", sorted(C.KNOB_CASES))
def test_knob_group(group):
    """SDR_FGS_LR_MAXL=16 (k_fgs_lr<16>, also under a (360, 576) WLS map's 16-line column passes)
    and SDR_FGS_LR=0 SDR_FGS_LRJOB=0 (k_fgs_th<true, 16 | 32 | 64> passes and jobs on short
    lines): one fresh child process a group, one at a time; the child asserts the plans."""
    env = dict(os.environ, **C.KNOB_ENV[group])
    r = subprocess.run([sys.executable, os.path.join(HERE, "fgs_dispatch_child.py"), group], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    assert verdict["ran"] == len(C.KNOB_CASES[group]) and not verdict["failed"], verdict
