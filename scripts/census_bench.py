"""Census vs Birchfield-Tomasi matching cost, A/B in ONE process: a BT handle and a census handle
on the same resident inputs, rounds alternating between them (as scripts/kbench.py alternates
builds).  Per round and handle: the whole-call device time (device events around `iters` calls,
per-kernel timing off) and the per-kind kernel times (enable_timing(2)).  Prints one JSON object;
the comparison's margin is the round-to-round spread of BT's own k_cost time in this run.

    python scripts/census_bench.py --config c2 [--rounds 7 --iters 30] > profiles/census_bench_c2.json

Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402

CONFIGS = {  # W, H, D, mode, blockSize
    "c2": (1280, 720, 128, sdr.MODE_SGBM, 5),
    "c0": (640, 360, 80, sdr.MODE_SGBM_3WAY, 5),
}
KINDS = {"prefilter": sdr.sgbm.KERNEL_PREFILTER, "k_cost": sdr.sgbm.KERNEL_COST,
         "k_paths": sdr.sgbm.KERNEL_PATHS, "k_south_wta": sdr.sgbm.KERNEL_WTA_LR}


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "rounds": [round(float(x), 2) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("census_bench.py needs a GPU")
    W, H, D, mode, bs = CONFIGS[a.config]
    L, R, _ = S.make_pair(H, W, D, seed=100)
    dev = torch.device("cuda", 0)
    dl, dr = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    # BT with the reference's penalties; census with penalties scaled to its block cost (<= 62*bs^2)
    handles = {
        "bt": sdr.StereoSGBM.create(0, D, bs, 600, 2400, 1, 63, 12, 200, 2, mode),
        "census": sdr.StereoSGBM.create(0, D, bs, 2 * bs * bs, 12 * bs * bs, 1, 63, 12, 200, 2, mode,
                                        cost=sdr.COST_CENSUS),
    }
    out = torch.empty((1, H, W), dtype=torch.int16, device=dev)
    res = {n: {k: [] for k in list(KINDS) + ["frame"]} for n in handles}
    for _ in range(a.rounds):
        for name, m in handles.items():
            for _ in range(3):
                m.compute(dl, dr, out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                m.compute(dl, dr, out)
            e1.record()
            torch.cuda.synchronize()
            res[name]["frame"].append(e0.elapsed_time(e1) * 1000 / a.iters)
            m.enable_timing(2)
            for _ in range(a.iters):
                m.compute(dl, dr, out)
            torch.cuda.synchronize()
            for k, kind in KINDS.items():
                t, n = m.kernel_time(kind)
                res[name][k].append(t * 1000 / max(n, 1))
            m.enable_timing(0)
    valid = {}
    for name, m in handles.items():
        d = m.compute(dl, dr).cpu().numpy()
        valid[name] = float((d != -16).mean())
    W1 = W - D
    cells = H * W1 * D
    bt_cost = res["bt"]["k_cost"]
    report = {
        "config": a.config, "W": W, "H": H, "D": D, "mode": mode, "blockSize": bs, "iters": a.iters,
        "rounds": a.rounds, "unit": "us", "device": torch.cuda.get_device_name(0),
        "cells": cells,
        # bytes a cell of C: both kernels write 2 B; the operands they read per pixel and eye
        "bytes_per_cell_written": 2,
        "operand_bytes_per_pixel": {"bt": {"left": 12, "right": 24}, "census": {"left": 8, "right": 8}},
        "bt": {k: stats(v) for k, v in res["bt"].items()},
        "census": {k: stats(v) for k, v in res["census"].items()},
        "valid_fraction": valid,
        "bt_k_cost_spread_us": float(max(bt_cost) - min(bt_cost)),
        "ratio_census_over_bt": {k: float(np.median(res["census"][k]) / np.median(res["bt"][k]))
                                 for k in ("prefilter", "k_cost", "frame")},
    }
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
