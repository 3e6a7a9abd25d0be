#!/usr/bin/env python3
"""What one measurement costs at the class path's map size (640x360, six frames resident).

In one process, alternating round-robin so that drift hits every candidate alike:
  (a) the only way before the ruler: copy one frame's XYZ map to the host (2.76 MB) and index it;
  (b) Ruler.measure_device + copying out the records, for K in {1, 64, 1024} x radius in {0, 2} x
      profile off / on (the record's profile fields; no per-sample rows are requested).
Each repetition is a host clock from the call to the end of the copy-out (which synchronises).
Then the LiveLoop frame with and without one LiveLoop.measure per frame, as a same-run A/B: frames
issued round-robin on six streams, timed in blocks that alternate between the loops.  The segment
is a host tuple, as a mouse click produces it, and a device tensor uploaded once, both measured.

usage: scripts/ruler_bench.py [--reps 200] [--out profiles/ruler_bench_c4.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.config import StereoConfiguration  # noqa: E402
from stereo_depth_ruler_amd.pipeline import LiveLoop  # noqa: E402
from stereo_depth_ruler_amd.rectify import StereoRectifier  # noqa: E402


def stats(us):
    a = np.sort(np.asarray(us, np.float64))
    return {"median_us": round(float(np.median(a)), 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]), 2),
            "p90_us": round(float(a[int(0.9 * (len(a) - 1))]), 2), "min_us": round(float(a[0]), 2), "n": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=48, help="frames per block of the LiveLoop A/B")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per variant of the LiveLoop A/B")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ruler_bench_c4.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    F, H, W = 6, 360, 640
    rng = np.random.default_rng(0)
    # a noisy wall with holes, as SGBM / WLS output looks to the ruler
    d = 40.0 + rng.normal(0, 0.25, (F, H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    d[rng.random((F, H, W)) < 0.15] = -1.0
    disp = torch.from_numpy(d).to(dev)
    conf = torch.from_numpy(rng.uniform(0, 255, (F, H, W)).astype(np.float32)).to(dev)
    xyz = sdr.reprojectImageTo3D(disp, S.REFERENCE_Q, False)
    torch.cuda.synchronize()

    def segments(K):
        return np.stack([rng.integers(0, F, K), rng.integers(0, W, K), rng.integers(0, H, K),
                         rng.integers(0, W, K), rng.integers(0, H, K)], axis=1).astype(np.int32)

    cands = {}

    def copy_lookup():  # (a)
        m = xyz[2].cpu().numpy()
        return float(np.linalg.norm(m[117, 434] - m[189, 440]))

    cands["a_xyz_frame_to_host_lookup"] = copy_lookup
    for K in (1, 64, 1024):
        segs_h = segments(K)
        segs_d = torch.from_numpy(segs_h).to(dev)
        for r in (0, 2):
            for prof in (False, True):
                ruler = sdr.Ruler(S.REFERENCE_Q, radius=r, min_count=1 if r == 0 else 3, profile=prof)

                def run(ruler=ruler, segs_d=segs_d):
                    # profile_cap 0: the record's profile fields without the per-sample rows
                    rec, _ = ruler.measure_device(disp, segs_d, conf=conf, profile_cap=0)
                    return rec.cpu()

                cands[f"b_measure_K{K}_r{r}_profile{int(prof)}"] = run
    times = {k: [] for k in cands}
    for it in range(a.warmup + a.reps):
        for name, fn in cands.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e6
            if it >= a.warmup:
                times[name].append(dt)
    result = {"map": [F, H, W], "xyz_frame_bytes": H * W * 12, "reps": a.reps,
              "method": "host clock around call + copy-out (synchronises), candidates alternated round-robin",
              "device": torch.cuda.get_device_name(0),
              "candidates": {k: stats(v) for k, v in times.items()}}

    # ---- LiveLoop frame time with / without one enqueued measure ----
    cfg = StereoConfiguration()
    assert cfg.loadFromFile(os.path.join(ROOT, "tests", "golden", "stereo.yaml"))
    Wf, Hf = cfg.imageSize
    rect = StereoRectifier(cfg)
    ns = 6
    frames = [torch.from_numpy(S.sbs_bgr_color_frame(Hf, Wf, 80, seed=100 + i)[None]).to(dev) for i in range(ns)]
    streams = [torch.cuda.Stream(dev) for _ in range(ns)]
    plain = [LiveLoop(rect, cfg.Q, 1) for _ in range(ns)]
    ruled = [LiveLoop(rect, cfg.Q, 1, ruler=dict(radius=2, min_count=3, profile=True)) for _ in range(ns)]
    seg_host = [(0, 217, 58, 220, 94)]
    seg_dev = torch.from_numpy(np.array(seg_host, np.int32)).to(dev)

    def block(pipes, seg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            k = i % ns
            with torch.cuda.stream(streams[k]):
                pipes[k].enqueue(frames[k], streams[k])
                if seg is not None:
                    pipes[k].measure(seg, streams[k], profile_cap=37)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.frames

    for _ in range(2):
        block(plain, None)
        block(ruled, seg_host)
        block(ruled, seg_dev)
    ab = {"plain": [], "ruler_conf_only": [], "ruler_measure_host_segment": [], "ruler_measure_device_segment": []}
    for _ in range(a.blocks):
        ab["plain"].append(block(plain, None))
        ab["ruler_conf_only"].append(block(ruled, None))
        ab["ruler_measure_host_segment"].append(block(ruled, seg_host))
        ab["ruler_measure_device_segment"].append(block(ruled, seg_dev))
    result["live_loop_frame"] = {
        "frame": [Hf, 2 * Wf, 3], "streams": ns, "frames_per_block": a.frames,
        "method": "host clock over a block of frames issued round-robin on six streams, ended by a "
                  "synchronise; blocks alternate plain / ruler=... without measure / with one "
                  "LiveLoop.measure a frame (radius 2, min_count 3, profile on with its 37 rows, one 37-sample "
                  "segment given as a host tuple or as a device tensor)",
        **{k: stats(v) for k, v in ab.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
