"""Runs one knob group of the FGS dispatch cases (fgs_cases.KNOB_CASES) against the oracle and
prints a JSON verdict on the last line of its output: {"group", "ran", "failed": {case: [what]}}.

The engine reads SDR_FGS_LR, SDR_FGS_LRJOB and SDR_FGS_LR_MAXL once, so a knob needs a process of
its own: test_gpu_fgs_dispatch.py and test_fgs_dispatch_cpu.py start this script with the group's
environment (fgs_cases.KNOB_ENV) and assert on the verdict.

    python tests/fgs_dispatch_child.py GROUP [--inputs-only --cus N]

--inputs-only stops every case after the plan and input assertions (no GPU), with the plan of a
device of N compute units.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]


def main(argv):
    import fgs_cases as C
    from oracle import oracle as O

    group = argv[0]
    inputs_only = "--inputs-only" in argv
    cus = int(argv[argv.index("--cus") + 1]) if "--cus" in argv else 0
    for k, v in C.KNOB_ENV[group].items():
        assert os.environ.get(k) == v, f"{k} must be {v} for group {group}"
    O.build()
    failed = {}
    cases = C.KNOB_CASES[group]
    for c in cases:
        errs = C.run_case(O, c, cus=cus, inputs_only=inputs_only)
        if errs:
            failed[C.case_id(c)] = errs
    print(json.dumps({"group": group, "ran": len(cases), "failed": failed}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
