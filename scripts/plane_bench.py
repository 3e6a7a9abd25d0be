#!/usr/bin/env python3
"""What a plane fit costs at the class path's map size (640x360, six frames resident).

In one process, alternating round-robin so that drift hits every candidate alike:
  (a) the only way before the device fit: copy one float disparity frame (921.6 kB) to the host
      and run np.linalg.lstsq on the valid pixels of the region (one plain least-squares fit: no
      refits, so it is the baseline of iterations 0 and a lower bound for a host robust fit);
  (b) Ruler.fit_plane_device + copying out the 128-byte record, for the same regions, iterations 0
      and 3;
  (c) a fit plus 64 point queries chained on one stream (the records tensor feeds
      plane_distance_device; one copy-out of 64 x 32 bytes at the end).
Regions: 32x32, 160x120 and the whole frame.  Each repetition is a host clock from the call to the
end of the copy-out (which synchronises); (a) is timed in the same run and is never the code under
test.

usage: scripts/plane_bench.py [--reps 200] [--out profiles/plane_bench_c4.json]
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


def stats(us):
    a = np.sort(np.asarray(us, np.float64))
    return {"median_us": round(float(np.median(a)), 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]), 2),
            "p90_us": round(float(a[int(0.9 * (len(a) - 1))]), 2), "min_us": round(float(a[0]), 2), "n": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_bench_c4.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    F, H, W = 6, 360, 640
    rng = np.random.default_rng(0)
    # a tilted surface with noise, holes and outliers, as SGBM / WLS output looks to the fit
    ys, xs = np.mgrid[0:H, 0:W]
    d = 30.0 + 0.02 * xs - 0.035 * ys + rng.normal(0, 0.25, (F, H, W))
    d = (np.round(d * 16) / 16).astype(np.float32)
    u = rng.random((F, H, W))
    d[u < 0.30] = -1.0
    out = (u >= 0.30) & (u < 0.45)
    d[out] = rng.uniform(1, 80, int(out.sum())).astype(np.float32)
    disp = torch.from_numpy(d).to(dev)
    ruler = sdr.Ruler(S.REFERENCE_Q, radius=1, min_count=2)
    regions = {"32x32": (2, 300, 160, 331, 191), "160x120": (2, 240, 120, 399, 239), "640x360": (2, 0, 0, W - 1, H - 1)}
    cands = {}
    for name, (f, x0, y0, x1, y1) in regions.items():
        def host_fit(f=f, x0=x0, y0=y0, x1=x1, y1=y1):  # (a)
            m = disp[f].cpu().numpy()[y0:y1 + 1, x0:x1 + 1]
            vy, vx = np.nonzero(m > -1.0)
            A = np.stack([vx, vy, np.ones_like(vx)], axis=1).astype(np.float64)
            return np.linalg.lstsq(A, m[vy, vx].astype(np.float64), rcond=None)[0]

        cands[f"a_frame_to_host_lstsq_{name}"] = host_fit
        reg_d = torch.from_numpy(np.array([[f, x0, y0, x1, y1]], np.int32)).to(dev)
        pts = np.stack([np.full(64, f), rng.integers(x0, x1 + 1, 64), rng.integers(y0, y1 + 1, 64),
                        np.zeros(64, np.int64)], axis=1).astype(np.int32)
        pts_d = torch.from_numpy(pts).to(dev)
        for it in (0, 3):
            def fit(reg_d=reg_d, it=it):  # (b)
                return ruler.fit_plane_device(disp, reg_d, iterations=it).cpu()

            def fit_query(reg_d=reg_d, pts_d=pts_d, it=it):  # (c)
                planes = ruler.fit_plane_device(disp, reg_d, iterations=it)
                return ruler.plane_distance_device(disp, planes, pts_d).cpu()

            cands[f"b_fit_plane_{name}_iterations{it}"] = fit
            cands[f"c_fit_plus_64_queries_{name}_iterations{it}"] = fit_query
    times = {k: [] for k in cands}
    for rep in range(a.warmup + a.reps):
        for name, fn in cands.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e6
            if rep >= a.warmup:
                times[name].append(dt)
    result = {"map": [F, H, W], "disparity_frame_bytes": H * W * 4, "reps": a.reps,
              "method": "host clock around call + copy-out (synchronises), candidates alternated round-robin",
              "device": torch.cuda.get_device_name(0),
              "candidates": {k: stats(v) for k, v in times.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
