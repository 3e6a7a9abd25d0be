#!/usr/bin/env python3
"""What the relief of a region costs on a 640x360 float disparity frame holding three surfaces
(floor, box, wall; noise, 5 % outliers, 20 % holes), against the floor plane the search finds.

In one process, in blocks; inside a block the candidates alternate round-robin so that drift hits
every one alike.  A candidate's figure is the median over the blocks of the block's median, its
spread the lowest and highest block median:
  (a) Ruler.relief_device with 3 quantiles and its 128-byte record copied out: a 32x32 region, a
      320x240 region, the whole frame, the whole frame under the box's label;
  (b) the device route that existed before: Ruler.plane_distance_device with one query a region
      pixel (the queries already on the device), the finite distances sorted with torch.sort, the
      three order statistics copied out (the same three values as (a)'s, checked here);
  (c) the host route: the disparity frame (921.6 kB) copied out and the numpy restatement
      (tests/relief_ref.py) run on it (--host-reps repetitions a block only).
Each repetition is a host clock from the call to the end of the copy-out (which synchronises).
Then a C4 LiveLoop frame (2560x720 side-by-side stream, six streams) with and without one
whole-frame relief enqueued behind each frame, in alternating blocks of frames.

--kernels-only runs the whole-frame relief alone, for a rocprofv3 --kernel-trace --stats run of its
own; --kernel-stats DIR merges that run's kernel_stats.csv into the JSON that --out names (the
relief's kernels: calls and mean us a launch) and measures nothing.

usage: scripts/relief_bench.py [--blocks 7] [--reps 40] [--out profiles/relief_bench_c4.json]
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
import relief_ref as LR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.config import StereoConfiguration  # noqa: E402
from stereo_depth_ruler_amd.pipeline import LiveLoop  # noqa: E402
from stereo_depth_ruler_amd.rectify import StereoRectifier  # noqa: E402
from stereo_depth_ruler_amd.ruler import PLANE_DTYPE, RELIEF_DTYPE, as_relief_queries  # noqa: E402

H, W = 360, 640
QUANT = (50, 500, 950)


def over_blocks(block_medians):
    a = np.asarray(block_medians, np.float64)
    return {"median_us": round(float(np.median(a)), 2), "lowest_block_us": round(float(a.min()), 2),
            "highest_block_us": round(float(a.max()), 2), "blocks": len(a)}


def kernel_stats(path, out):
    """The relief's kernels from a rocprofv3 --stats run of --kernels-only, into the JSON at `out`."""
    f = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)[0]
    rows = {}
    for r in csv.DictReader(open(f)):
        for k in ("k_relief_sweep", "k_relief_pick1", "k_relief_pick2", "k_relief_finish"):
            if k in r["Name"]:
                for n in "123":  # the sweep's pass, from the mangled or the demangled name
                    if k == "k_relief_sweep" and (f"Li{n}E" in r["Name"] or f", {n}>" in r["Name"]):
                        k = f"k_relief_sweep_pass{n}"
                e = rows.setdefault(k, {"calls": 0, "total_ns": 0})
                e["calls"] += int(r["Calls"])
                e["total_ns"] += int(float(r["TotalDurationNs"]))
    for e in rows.values():
        e["avg_us"] = round(e["total_ns"] / max(e["calls"], 1) / 1e3, 3)
    with open(out) as fh:
        result = json.load(fh)
    result["kernel_stats"] = {"method": "rocprofv3 --kernel-trace --stats in a run of its own: the whole-frame relief "
                                        "(3 quantiles, no label) alone", **rows}
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["kernel_stats"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --stats run of --kernels-only")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=120, help="LiveLoop frames a block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relief_bench_c4.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out)
        return
    dev = torch.device("cuda", 0)
    Q = S.REFERENCE_Q
    d, truth, _ = SR.three_surface_scene(H, W)
    disp = torch.from_numpy(d).to(dev)
    ruler = sdr.Ruler(Q)
    planes_t, count, _, lab_t = ruler.find_planes_device(disp, None, max_planes=4, hypotheses=256, min_inliers=1000,
                                                         labels=True)
    planes = planes_t.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    lab = lab_t.cpu().numpy()
    n_found = int(count.cpu()[0])
    idx = [int(np.argmax([((lab == i) & (truth == s)).sum() for i in range(n_found)])) for s in range(3)]
    floor, box = idx[0], idx[1]

    regions = {"32x32": (0, 300, 160, 331, 191, floor, -1), "320x240": (0, 160, 60, 479, 299, floor, -1),
               "frame": (0, 0, 0, W - 1, H - 1, floor, -1), "frame_label": (0, 0, 0, W - 1, H - 1, floor, box)}
    cands, host, agree = {}, {}, {}
    for name, reg in regions.items():
        if a.kernels_only and name != "frame":
            continue
        q_d = torch.from_numpy(as_relief_queries([reg])).to(dev)

        def relief(q_d=q_d):  # (a)
            return ruler.relief_device(disp, planes_t, q_d, labels=lab_t, quantiles=QUANT).cpu()

        cands[f"a_relief_{name}"] = relief
        rec = relief().numpy().reshape(-1).view(RELIEF_DTYPE)[0]
        if name == "frame_label" or a.kernels_only:
            continue  # the per-pixel route has no mask
        xs, xe, ys, ye = reg[1], reg[3], reg[2], reg[4]
        yy, xx = np.mgrid[ys:ye + 1, xs:xe + 1]
        pts = np.stack([np.zeros(xx.size, np.int32), xx.reshape(-1), yy.reshape(-1), np.full(xx.size, floor)], axis=1)
        pts_d = torch.from_numpy(np.ascontiguousarray(pts, np.int32)).to(dev)
        perm = torch.tensor(QUANT, device=dev, dtype=torch.int64)

        def per_pixel(pts_d=pts_d):  # (b)
            out = ruler.plane_distance_device(disp, planes_t, pts_d)
            dist = out.view(torch.float64).reshape(-1, 4)[:, 2]
            s, _ = torch.sort(dist[torch.isfinite(dist)])
            return s[((s.numel() - 1) * perm) // 1000].cpu()

        cands[f"b_plane_distance_per_pixel_sort_{name}"] = per_pixel
        agree[name] = bool(np.array_equal(per_pixel().numpy().astype(np.float32), rec["q"][:3]))

        def on_host(reg=reg):  # (c)
            return LR.relief(disp.cpu().numpy(), planes, [reg], Q, quantiles=QUANT)

        host[f"c_frame_to_host_numpy_{name}"] = on_host

    if a.kernels_only:
        for _ in range(a.warmup + a.blocks * a.reps):
            cands["a_relief_frame"]()
        torch.cuda.synchronize()
        return
    blocks = {k: [] for k in list(cands) + list(host)}
    for _ in range(a.warmup):
        for fn in cands.values():
            fn()
    for _ in range(a.blocks):
        times = {k: [] for k in blocks}
        for rep in range(a.reps):
            for name, fn in list(cands.items()) + (list(host.items()) if rep < a.host_reps else []):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e6)
        for k, v in times.items():
            blocks[k].append(float(np.median(v)))
    result = {"map": [H, W], "disparity_frame_bytes": H * W * 4, "quantiles": list(QUANT), "reps_per_block": a.reps,
              "host_reps_per_block": a.host_reps, "planes_found": n_found, "floor_plane": floor, "box_label": box,
              "regions": {k: list(v) for k, v in regions.items()},
              "method": "host clock around call + copy-out (synchronises); candidates alternated round-robin inside "
                        "a block; median over blocks of the block medians, with the lowest and highest block",
              "device": torch.cuda.get_device_name(0),
              "per_pixel_route_gives_the_same_quantiles": agree,
              "candidates": {k: over_blocks(v) for k, v in blocks.items()}}

    # ---- a C4 LiveLoop frame with / without one whole-frame relief behind it ----
    cfg = StereoConfiguration()
    assert cfg.loadFromFile(os.path.join(ROOT, "tests", "golden", "stereo.yaml"))
    Wf, Hf = cfg.imageSize
    rect = StereoRectifier(cfg)
    ns = 6
    frames = [torch.from_numpy(S.sbs_bgr_color_frame(Hf, Wf, 80, seed=100 + i)[None]).to(dev) for i in range(ns)]
    streams = [torch.cuda.Stream(dev) for _ in range(ns)]
    loops = [LiveLoop(rect, cfg.Q, 1, ruler=dict()) for _ in range(ns)]
    w2, h2 = loops[0].w2, loops[0].h2
    with torch.cuda.stream(streams[0]):
        loops[0].enqueue(frames[0], streams[0])
        plane_d = loops[0].fit_plane([(0, 0, h2 // 2, w2 - 1, h2 - 1)], streams[0])
    streams[0].synchronize()
    reg_d = torch.from_numpy(as_relief_queries([(0, 0, 0, w2 - 1, h2 - 1, 0, -1)])).to(dev)

    def block(with_relief):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            k = i % ns
            with torch.cuda.stream(streams[k]):
                loops[k].enqueue(frames[k], streams[k])
                if with_relief:
                    loops[k].relief(plane_d, reg_d, streams[k], quantiles=QUANT)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.frames

    for _ in range(2):
        block(False)
        block(True)
    ab = {"frame_only": [], "frame_and_relief": []}
    for _ in range(a.blocks):
        ab["frame_only"].append(block(False))
        ab["frame_and_relief"].append(block(True))
    result["live_loop_frame"] = {
        "frame": [Hf, 2 * Wf, 3], "map": [h2, w2], "streams": ns, "frames_per_block": a.frames,
        "plane_flags": int(plane_d.cpu().numpy().reshape(-1).view(PLANE_DTYPE)["flags"][0]),
        "method": "host clock over a block of frames issued round-robin on six streams, ended by a synchronise; "
                  "blocks alternate without / with one whole-frame LiveLoop.relief (3 quantiles, plane and query on "
                  "the device) a frame; us a frame",
        **{k: over_blocks(v) for k, v in ab.items()}}
    for lp in loops:
        lp.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
