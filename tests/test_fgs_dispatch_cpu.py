"""sdr_fgs_plan_query without a GPU: the sequential FGS solver's dispatch on both sides of every
threshold (the launchers run the same functions), and the condition on the inputs of
test_gpu_fgs_dispatch.py for every shape it lists, from the oracle's weight table alone."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import fgs_cases as C
from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd._lib import FGS_PCR, fgs_plan

HERE = os.path.dirname(os.path.abspath(__file__))
CUS = 256


def plan(w, h, **kw):
    kw.setdefault("cus", CUS)
    return fgs_plan(w, h, **kw)


def test_plan_struct_layout():
    assert ctypes.sizeof(_lib.FgsLaunch) == 8 and ctypes.sizeof(_lib.FgsPlan) == 40


@pytest.mark.parametrize("n,below,above", [
    # (n, the row pass / row job at n, at n + 1)
    (384, (("lr", 8), ("lrjob", 16)), (("lr", 8), ("lrjob", 8))),   # the passes' default cap is 8
    (768, (("lr", 8), ("lrjob", 8)), (("lr", 4), ("lrjob", 4))),
    # (past 1536 every job of the launch runs on k_fgs_th: 3 x (1 + ceil(n / lines)) workgroups
    # within 256 CUs at 32 lines for n = 1537, at 64 for n = 3072)
    (1536, (("lr", 4), ("lrjob", 4)), (("lr", 2), ("th", 32))),
    (3072, (("lr", 2), ("th", 64)), (("th", 16), ("th", 64))),
])
def test_line_length_thresholds(n, below, above):
    """Two right-hand sides, 5 lines of n and of n + 1 samples, as rows and as columns."""
    for k, want in ((n, below), (n + 1, above)):
        p = plan(k, 5)
        assert (p["row_pass"], p["row_job"]) == want, (k, p)
        assert p["col_pass"] == ("lr", 8)
        q = plan(5, k)
        assert (q["col_pass"], q["col_job"]) == want, (k, q)
        assert q["row_pass"] == ("lr", 8)


def test_job_fallback_is_all_or_nothing():
    """One job past 1536 samples sends every job of the launch to k_fgs_th: the 5-sample columns'
    job runs on k_fgs_lrjob next to 1536-sample rows and on k_fgs_th next to 1537-sample ones."""
    assert plan(1536, 5)["col_job"] == ("lrjob", 16)
    p = plan(1537, 5)
    assert p["row_job"][0] == p["col_job"][0] == "th" and p["row_job"] == p["col_job"]
    p = plan(5, 1537)
    assert p["row_job"][0] == p["col_job"][0] == "th"
    # each job of a k_fgs_lrjob launch has its own lines
    assert (plan(900, 20)["row_job"], plan(900, 20)["col_job"]) == (("lrjob", 4), ("lrjob", 16))
    assert (plan(24, 400)["row_job"], plan(24, 400)["col_job"]) == (("lrjob", 16), ("lrjob", 8))


def test_single_image_takes_th_passes():
    p = plan(300, 20, nimg=1)
    assert p["row_pass"] == p["col_pass"] == ("th", 16)
    assert (p["row_job"], p["col_job"]) == (("lrjob", 16), ("lrjob", 16))  # the jobs do not depend on it


@pytest.mark.parametrize("lf,lines", [(4096, 16), (4097, 32), (8192, 32), (8193, 64)])
def test_th_lines_by_line_frames(lf, lines):
    """k_fgs_th's lines a workgroup: 16 while the workgroups fit the chip's 256 CUs at once
    (line-frames <= 16 * 256), then 32 (<= 32 * 256), then 64: one frame, and the same line-frames
    as frames of fewer lines."""
    assert plan(5, lf, nimg=1)["row_pass"] == ("th", lines)
    assert plan(lf, 5, nimg=1)["col_pass"] == ("th", lines)
    assert plan(3073, lf)["row_pass"] == ("th", lines)  # two right-hand sides past k_fgs_lr
    if lf % 2 == 0:
        assert plan(5, lf // 2, nframes=2, nimg=1)["row_pass"] == ("th", lines)
    else:
        assert plan(5, (lf + 1) // 2, nframes=2, nimg=1)["row_pass"] == ("th", lines)
    # half as many CUs: half as many line-frames
    assert plan(5, lf // 2 if lf % 2 == 0 else lf // 2 + 1, nimg=1, cus=CUS // 2)["row_pass"] == ("th", lines)


def test_th_job_lines_count_every_job():
    """The jobs of a launch share its workgroups: 2 * num_iter jobs (8 at most) of `nl` lines."""
    # 6 jobs, 3 of 5 lines and 3 of 1600: 3 * (1 + 100) workgroups of 16 lines > 256, of 32: 153
    assert plan(5, 1600)["col_job"] == ("th", 32)
    assert plan(5, 1600, num_iter=1)["col_job"] == ("th", 16)  # 2 jobs: 101 workgroups


def test_pcr_plan_and_refusals():
    p = plan(560, 360, solver=FGS_PCR)
    assert (p["row_pass"], p["col_pass"]) == (("pcr", 1), ("pcr", 2))
    assert p["row_job"] == p["col_job"] == ("none", 0)
    with pytest.raises(_lib.SDRError):
        plan(4097, 5, solver=FGS_PCR)
    for bad in (dict(w=0, h=5), dict(w=5, h=5, nimg=3), dict(w=5, h=5, num_iter=0), dict(w=5, h=5, solver=7)):
        with pytest.raises(_lib.SDRError):
            plan(**bad)
    assert _lib.lib().sdr_fgs_plan_query(5, 5, 1, 2, 3, 1, CUS, None) == -1


def test_generator_meets_input_condition(oracle):
    """Every shape test_gpu_fgs_dispatch.py runs in its own process: the plan it is named for (on a
    256-CU device) and, at (8000, 1.1), a group with a tiny non-zero weight and a clean group in
    every chunk of every line."""
    bad = {C.case_id(c): e for c in C.PARENT_CASES
           if (e := C.run_case(oracle, c, cus=CUS, inputs_only=True))}
    assert not bad, bad


@pytest.mark.parametrize("group", sorted(C.KNOB_CASES))
def test_knob_groups_meet_input_condition(oracle, group):
    """The same for the knob groups, each in a child process with its knobs set (the query reads
    them like the launchers do)."""
    env = dict(os.environ, **C.KNOB_ENV[group])
    r = subprocess.run([sys.executable, os.path.join(HERE, "fgs_dispatch_child.py"), group,
                        "--inputs-only", "--cus", str(CUS)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    assert verdict["ran"] == len(C.KNOB_CASES[group]) and not verdict["failed"], verdict
