#!/usr/bin/env python3
"""What the objects of a region cost on a 640x360 float disparity frame holding a box top and a
hemisphere on a tilted floor (noise, 5 % outliers, 20 % holes), above the floor plane the search
finds.

In one process, in blocks; inside a block the candidates alternate round-robin so that drift hits
every one alike.  A candidate's figure is the median over the blocks of the block's median, its
spread the lowest and highest block median:
  (a) Ruler.find_objects_device (heights 10 .. 1000 mm, max_diff 1 px, connectivity 8, min_pixels 64,
      max_objects 16) with its records (16 x 64 + 64 bytes) copied out: the whole frame and a 32x32
      region, each without a label map and with the 230.4 kB label map copied out too;
  (b) sdr_filter_speckles_device on the same frame as int16 (maxSpeckleSize 64, maxDiff 16 = 1 px), a
      copy-in on the device included: the nearest existing labelling, and its baseline;
  (c) Ruler.find_planes_device at its default, its records copied out;
  (d) the only route before: the disparity frame (921.6 kB) copied out and the numpy restatement
      (tests/objects_ref.py) run on it (--host-reps repetitions a block only; its records and labels
      are checked against (a)'s on every bit).
Each repetition is a host clock from the call to the end of the copy-out (which synchronises).
Then a C4 LiveLoop frame (2560x720 side-by-side stream, six streams) with and without one
whole-frame find_objects enqueued behind each frame, in alternating blocks of frames.

usage: scripts/objects_bench.py [--blocks 7] [--reps 40] [--out profiles/objects_bench_c4.json]
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
import objects_ref as OR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.config import StereoConfiguration  # noqa: E402
from stereo_depth_ruler_amd.pipeline import LiveLoop  # noqa: E402
from stereo_depth_ruler_amd.rectify import StereoRectifier  # noqa: E402
from stereo_depth_ruler_amd.ruler import OBJECT_DTYPE, OBJECT_SCAN_DTYPE, PLANE_DTYPE, as_relief_queries  # noqa: E402

H, W = 360, 640
OBJ = dict(h_range=(10.0, 1000.0), max_diff=1.0, connectivity=8, min_pixels=64, max_objects=16)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench_c4.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    Qw = FR.scene_q(S.REFERENCE_Q)
    d, truth, _ = OR.two_object_scene(Qw, H=H, W=W)
    disp = torch.from_numpy(d).to(dev)
    disp16 = torch.from_numpy(np.round(d[0] * 16).astype(np.int16)).to(dev)
    work16 = torch.empty_like(disp16)
    ruler = sdr.Ruler(Qw)
    planes_t, count, _, lab_t = ruler.find_planes_device(disp, None, max_planes=3, hypotheses=256, min_inliers=1000,
                                                         labels=True)
    planes = planes_t.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    lab = lab_t.cpu().numpy()
    n_found = int(count.cpu()[0])
    floor = int(np.argmax([((lab == i) & (truth == 0)).sum() for i in range(n_found)]))

    regions = {"frame": (0, 0, 0, W - 1, H - 1, floor, -1), "32x32": (0, 300, 160, 331, 191, floor, -1)}
    cands, host, agree, recs = {}, {}, {}, {}
    for name, reg in regions.items():
        q_d = torch.from_numpy(as_relief_queries([reg])).to(dev)

        def records(q_d=q_d):  # (a) without the label map
            rec, scan, _ = ruler.find_objects_device(disp, planes_t, q_d, labels_out=None, **OBJ)
            return rec.cpu(), scan.cpu()

        def labelled(q_d=q_d):  # (a) with it
            rec, scan, lo = ruler.find_objects_device(disp, planes_t, q_d, labels_out=True, **OBJ)
            return rec.cpu(), scan.cpu(), lo.cpu()

        def on_host(reg=reg):  # (d)
            return OR.find_objects(disp.cpu().numpy(), planes, reg, Qw, **OBJ)

        cands[f"a_find_objects_records_{name}"] = records
        cands[f"a_find_objects_records_and_labels_{name}"] = labelled
        host[f"d_frame_to_host_numpy_{name}"] = on_host
        rec, scan, lo = labelled()
        rec = rec.numpy().reshape(-1).view(OBJECT_DTYPE)
        scan = scan.numpy().view(OBJECT_SCAN_DTYPE)[0]
        want = on_host()
        agree[name] = (rec.tobytes() == want[0].tobytes() and scan.tobytes() == want[1].tobytes()
                       and np.array_equal(lo.numpy(), want[2]))
        n = int(scan["count"])
        recs[name] = {"flags": int(scan["flags"]), "n": int(scan["n"]), "n_components": int(scan["n_components"]),
                      "n_kept": int(scan["n_kept"]), "largest_dropped": int(scan["largest_dropped"]),
                      "objects_n": rec["n"][:n].tolist(),
                      "truth_of_objects": [[int(((lo.numpy() == k) & (truth == t)).sum()) for t in (1, 2)]
                                           for k in range(n)]}

    def speckle():  # (b)
        work16.copy_(disp16)
        sdr.filterSpeckles(work16, -16, 64, 16)
        torch.cuda.synchronize()

    def search():  # (c)
        p, c, _, _ = ruler.find_planes_device(disp, None)
        return p.cpu(), c.cpu()

    cands["b_filter_speckles_frame"] = speckle
    cands["c_find_planes_default_frame"] = search

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
    result = {"map": [H, W], "disparity_frame_bytes": H * W * 4, "label_map_bytes": H * W, "find_objects": OBJ,
              "reps_per_block": a.reps, "host_reps_per_block": a.host_reps, "planes_found": n_found,
              "floor_plane": floor,
              "truth_pixels": {"box": int((truth == 1).sum()), "hemisphere": int((truth == 2).sum())},
              "regions": {k: list(v) for k, v in regions.items()}, "records": recs,
              "scratch_bytes": (8 * H * W + (8 * OBJ["max_objects"] + 16) * ((H * W + 2047) // 2048)
                                + 16 * ((H + 31) // 32) * ((W + 31) // 32) + 3616),
              "method": "host clock around call + copy-out (synchronises); candidates alternated round-robin inside "
                        "a block; median over blocks of the block medians, with the lowest and highest block",
              "device": torch.cuda.get_device_name(0),
              "host_restatement_gives_the_same_records_and_labels": agree,
              "candidates": {k: over_blocks(v) for k, v in blocks.items()}}

    # ---- a C4 LiveLoop frame with / without one whole-frame find_objects behind it ----
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
    labs = [torch.empty((h2, w2), dtype=torch.uint8, device=dev) for _ in range(ns)]
    live = dict(OBJ, h_range=(-1048576.0, 1048576.0))  # the frame is no scene: every height

    def block(with_objects):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            k = i % ns
            with torch.cuda.stream(streams[k]):
                loops[k].enqueue(frames[k], streams[k])
                if with_objects:
                    loops[k].find_objects(plane_d, reg_d, streams[k], labels_out=labs[k], **live)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.frames

    for _ in range(2):
        block(False)
        block(True)
    ab = {"frame_only": [], "frame_and_find_objects": []}
    for _ in range(a.blocks):
        ab["frame_only"].append(block(False))
        ab["frame_and_find_objects"].append(block(True))
    result["live_loop_frame"] = {
        "frame": [Hf, 2 * Wf, 3], "map": [h2, w2], "streams": ns, "frames_per_block": a.frames,
        "plane_flags": int(plane_d.cpu().numpy().reshape(-1).view(PLANE_DTYPE)["flags"][0]),
        "method": "host clock over a block of frames issued round-robin on six streams, ended by a synchronise; "
                  "blocks alternate without / with one whole-frame LiveLoop.find_objects (plane and query on the "
                  "device, labels written) a frame; us a frame",
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
