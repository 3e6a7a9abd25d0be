#!/usr/bin/env python3
"""What finding a frame's dominant planes costs on a 640x360 float disparity frame holding three
surfaces (floor, box, wall; noise, 5 % outliers, 20 % holes).

In one process, alternating round-robin so that drift hits every candidate alike:
  (a) the only way before the device search: copy the disparity frame (921.6 kB) to the host and
      run a vectorised numpy search with the same M and the same number of rounds (the restatement
      tests/plane_search_ref.py, which is vectorised over pixels and hypotheses; it takes 0.1-3 s
      a call, so it gets --host-reps repetitions only);
  (b) Ruler.find_planes_device + copying out the records and the count, at M = 64 / 256 / 1024 and
      max_planes 1 and 4, with and without the 230 kB label map copied out;
  (c) Ruler.fit_plane_device on the same region in the same run (iterations 3: 5 sweeps + 1 record
      launch): the yardstick for the launch overhead a sweep.
Each repetition is a host clock from the call to the end of the copy-out (which synchronises); (a)
is timed in the same run and is never the code under test.

--kernels-only runs (b) at max_planes 4 alone, for a rocprofv3 --kernel-trace --stats run of its
own; --kernel-stats merges that run's kernel_stats.csv into the JSON as the score kernel's own time
and its evaluations a second.

usage: scripts/plane_search_bench.py [--reps 200] [--out profiles/plane_search_bench_c4.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import plane_search_ref as SR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402

H, W = 360, 640
MIN_INLIERS = 1000


def stats(us):
    a = np.sort(np.asarray(us, np.float64))
    return {"median_us": round(float(np.median(a)), 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]), 2),
            "p90_us": round(float(a[int(0.9 * (len(a) - 1))]), 2), "min_us": round(float(a[0]), 2), "n": len(a)}


def kernel_stats(path, result):
    """The search's kernels from a rocprofv3 --stats run of --kernels-only (its calls are M = 64,
    256, 1024 at max_planes 4, `reps` times each)."""
    f = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)[0]
    rows = {}
    for r in csv.DictReader(open(f)):
        name = r["Name"]
        for k in ("k_search_draw", "k_search_score", "k_search_pick", "k_search_finish", "k_search_claim",
                  "k_search_init", "k_plane_sweep"):
            if k in name:
                e = rows.setdefault(k, {"calls": 0, "total_ns": 0})
                e["calls"] += int(r["Calls"])
                e["total_ns"] += int(float(r["TotalDurationNs"]))
    for e in rows.values():
        e["avg_us"] = round(e["total_ns"] / max(e["calls"], 1) / 1e3, 3)
    result["kernel_stats"] = rows
    sc = rows.get("k_search_score")
    if sc:  # a repetition of --kernels-only is one search at each M, 4 score launches each
        reps = sc["calls"] / (4 * len(result["score_evaluations"]))
        evals = sum(result["score_evaluations"].values()) * reps
        result["score_kernel"] = {"evaluations": int(evals), "total_ns": sc["total_ns"],
                                  "giga_evaluations_per_s": round(evals / sc["total_ns"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --stats run of --kernels-only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_search_bench_c4.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, _, _ = SR.three_surface_scene(H, W)
    disp = torch.from_numpy(d).to(dev)
    ruler = sdr.Ruler(S.REFERENCE_Q)
    reg = (0, 0, 0, W - 1, H - 1)
    reg_d = torch.from_numpy(np.array([reg], np.int32)).to(dev)
    cands, host = {}, {}
    found = {}
    for M in (64, 256, 1024):
        for NP in (1, 4):
            kw = dict(max_planes=NP, hypotheses=M, min_inliers=MIN_INLIERS)

            def host_search(kw=kw):  # (a)
                m = disp.cpu().numpy()
                return SR.find_planes(m, reg, S.REFERENCE_Q, **kw)[1]

            def search(kw=kw):  # (b)
                rec, count, _, _ = ruler.find_planes_device(disp, reg_d, **kw)
                return rec.cpu(), count.cpu()

            def search_labels(kw=kw):
                rec, count, _, lab = ruler.find_planes_device(disp, reg_d, labels=True, **kw)
                return rec.cpu(), count.cpu(), lab.cpu()

            if a.kernels_only:
                if NP == 4:
                    cands[f"b_find_planes_M{M}_planes{NP}"] = search
                continue
            host[f"a_frame_to_host_numpy_search_M{M}_planes{NP}"] = host_search
            cands[f"b_find_planes_M{M}_planes{NP}"] = search
            cands[f"b_find_planes_labels_out_M{M}_planes{NP}"] = search_labels
            found[f"M{M}_planes{NP}"] = int(search()[1][0])
    if not a.kernels_only:
        cands["c_fit_plane_640x360_iterations3"] = lambda: ruler.fit_plane_device(disp, reg_d, iterations=3).cpu()
    times = {k: [] for k in list(cands) + list(host)}
    for rep in range(a.warmup + a.reps):
        for name, fn in cands.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e6
            if rep >= a.warmup:
                times[name].append(dt)
        if a.warmup <= rep < a.warmup + a.host_reps:
            for name, fn in host.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e6)
    if a.kernels_only:
        print(json.dumps({k: stats(v) for k, v in times.items()}))
        return
    px = int((d[0] > -1.0).sum())
    result = {"map": [H, W], "disparity_frame_bytes": H * W * 4, "valid_pixels": px, "reps": a.reps,
              "host_reps": a.host_reps, "min_inliers": MIN_INLIERS, "planes_found": found,
              "method": "host clock around call + copy-out (synchronises), candidates alternated round-robin",
              "device": torch.cuda.get_device_name(0),
              "candidates": {k: stats(v) for k, v in times.items()}}
    # the score kernel's work at max_planes 4: free pixels x hypotheses that are not void, a round
    result["score_evaluations"] = {}
    for M in (64, 256, 1024):
        trace = []
        SR.find_planes(d, reg, S.REFERENCE_Q, max_planes=4, hypotheses=M, min_inliers=MIN_INLIERS, trace=trace)
        result["score_evaluations"][f"M{M}"] = int(sum(len(t["u"]) * int((~t["table"]["void"]).sum()) for t in trace))
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
