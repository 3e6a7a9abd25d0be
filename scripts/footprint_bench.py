#!/usr/bin/env python3
"""What the footprint of a region costs on a 640x360 float disparity frame holding three surfaces
(floor, box, wall; noise, 5 % outliers, 20 % holes), in the floor plane the search finds.

In one process, in blocks; inside a block the candidates alternate round-robin so that drift hits
every one alike.  A candidate's figure is the median over the blocks of the block's median, its
spread the lowest and highest block median:
  (a) Ruler.footprint_device (cell 16 mm, grid 512, support 4, heights -100 .. 600 mm: without the
      band one far outlier moves the grid's origin away from every other member) and its 256-byte
      record copied out: a 32x32 region, the whole frame, the whole frame under the box's label;
  (b) Ruler.relief_device (3 quantiles) on the same queries, its 128-byte record copied out: the
      nearest device yardstick;
  (c) the only route before: the disparity frame (921.6 kB) and the label map (230.4 kB) copied out
      and the numpy restatement (tests/footprint_ref.py) run on them (--host-reps repetitions a
      block only; its record is checked against (a)'s on every bit).
Each repetition is a host clock from the call to the end of the copy-out (which synchronises).
Then a C4 LiveLoop frame (2560x720 side-by-side stream, six streams) with and without one
whole-frame footprint enqueued behind each frame, in alternating blocks of frames.

usage: scripts/footprint_bench.py [--blocks 7] [--reps 40] [--out profiles/footprint_bench_c4.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import footprint_ref as FR  # noqa: E402
import plane_search_ref as SR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.config import StereoConfiguration  # noqa: E402
from stereo_depth_ruler_amd.pipeline import LiveLoop  # noqa: E402
from stereo_depth_ruler_amd.rectify import StereoRectifier  # noqa: E402
from stereo_depth_ruler_amd.ruler import FOOTPRINT_DTYPE, PLANE_DTYPE, as_relief_queries  # noqa: E402

H, W = 360, 640
FOOT = dict(cell=16.0, grid=512, support=4, h_range=(-100.0, 600.0))
QUANT = (50, 500, 950)


def over_blocks(block_medians):
    a = np.asarray(block_medians, np.float64)
    return {"median_us": round(float(np.median(a)), 2), "lowest_block_us": round(float(a.min()), 2),
            "highest_block_us": round(float(a.max()), 2), "blocks": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=120, help="LiveLoop frames a block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "footprint_bench_c4.json"))
    a = ap.parse_args()
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

    regions = {"32x32": (0, 300, 160, 331, 191, floor, -1), "frame": (0, 0, 0, W - 1, H - 1, floor, -1),
               "frame_label": (0, 0, 0, W - 1, H - 1, floor, box)}
    cands, host, agree, recs = {}, {}, {}, {}
    for name, reg in regions.items():
        q_d = torch.from_numpy(as_relief_queries([reg])).to(dev)

        def footprint(q_d=q_d):  # (a)
            return ruler.footprint_device(disp, planes_t, q_d, labels=lab_t, **FOOT).cpu()

        def relief(q_d=q_d):  # (b)
            return ruler.relief_device(disp, planes_t, q_d, labels=lab_t, quantiles=QUANT).cpu()

        def on_host(reg=reg):  # (c)
            return FR.footprint(disp.cpu().numpy(), planes, [reg], Q, labels=lab_t.cpu().numpy(), **FOOT)

        cands[f"a_footprint_{name}"] = footprint
        cands[f"b_relief_{name}"] = relief
        host[f"c_frame_and_labels_to_host_numpy_{name}"] = on_host
        rec = footprint().numpy().reshape(-1).view(FOOTPRINT_DTYPE)
        agree[name] = rec.tobytes() == on_host().tobytes()
        recs[name] = {"flags": int(rec["flags"][0]), "side_mm": [round(float(v), 2) for v in rec["side"][0]],
                      "angle_deg": int(rec["angle_deg"][0]), "n": int(rec["n"][0]), "n_cells": int(rec["n_cells"][0]),
                      "n_outside": int(rec["n_outside"][0]), "fill": round(float(rec["fill"][0]), 3)}

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
    result = {"map": [H, W], "disparity_frame_bytes": H * W * 4, "label_map_bytes": H * W, "footprint": FOOT,
              "relief_quantiles": list(QUANT), "reps_per_block": a.reps, "host_reps_per_block": a.host_reps,
              "planes_found": n_found, "floor_plane": floor, "box_label": box,
              "regions": {k: list(v) for k, v in regions.items()}, "records": recs,
              "method": "host clock around call + copy-out (synchronises); candidates alternated round-robin inside "
                        "a block; median over blocks of the block medians, with the lowest and highest block",
              "device": torch.cuda.get_device_name(0),
              "host_restatement_gives_the_same_record": agree,
              "candidates": {k: over_blocks(v) for k, v in blocks.items()}}

    # ---- a C4 LiveLoop frame with / without one whole-frame footprint behind it ----
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

    def block(with_footprint):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            k = i % ns
            with torch.cuda.stream(streams[k]):
                loops[k].enqueue(frames[k], streams[k])
                if with_footprint:
                    loops[k].footprint(plane_d, reg_d, streams[k], **FOOT)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.frames

    for _ in range(2):
        block(False)
        block(True)
    ab = {"frame_only": [], "frame_and_footprint": []}
    for _ in range(a.blocks):
        ab["frame_only"].append(block(False))
        ab["frame_and_footprint"].append(block(True))
    result["live_loop_frame"] = {
        "frame": [Hf, 2 * Wf, 3], "map": [h2, w2], "streams": ns, "frames_per_block": a.frames,
        "plane_flags": int(plane_d.cpu().numpy().reshape(-1).view(PLANE_DTYPE)["flags"][0]),
        "method": "host clock over a block of frames issued round-robin on six streams, ended by a synchronise; "
                  "blocks alternate without / with one whole-frame LiveLoop.footprint (plane and query on the "
                  "device) a frame; us a frame",
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
