#!/usr/bin/env python3
"""What the clearance of two labelled things costs on a 640x360 float disparity frame holding a box
top and a hemisphere on a tilted floor (noise, 5 % outliers, 20 % holes), above the floor plane the
search finds, under the label map find_objects writes.

In one process, in blocks; inside a block the candidates alternate round-robin so that drift hits
every one alike.  A candidate's figure is the median over the blocks of the block's median, its
spread the lowest and highest block median.  Each repetition is a host clock from the call to the
end of the copy-out of the one 128-byte record (which synchronises):
  (a) Ruler.clearance_device, the box against the hemisphere, radius 0 / min_count 1 and radius 2 /
      min_count 9;
  (b) the same call on two labels that split the whole frame, touching (left half / right half) and
      far apart (left third / right third), radius 0, with the prune and with sdr_clearance_debug_knob's
      SDR_DEBUG_CLEARANCE_PRUNE at 0 (every block pair runs), over every valid pixel (the outliers too, whose points lie anywhere
      along their rays) and over the pixels within -20 .. 250 mm of the floor (the scene's surfaces);
  (c) torch.cdist + min on the two point sets gathered on the device from a reprojected XYZ map (the
      sets of (a) at radius 0; the split frames in row chunks of 4096, --slow-reps repetitions a
      block only): float32 distances, no index tie-break, no medians;
  (d) the only route before: the disparity frame (921.6 kB) and the label map (230.4 kB) copied out
      and the numpy restatement (tests/clearance_ref.py) run on them (the box against the hemisphere
      only, --slow-reps repetitions a block; its records are checked against (a)'s on every bit).

usage: scripts/clearance_bench.py [--blocks 5] [--reps 20] [--out profiles/clearance_bench_c4.json]
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

import clearance_ref as CR  # noqa: E402
import footprint_ref as FR  # noqa: E402
import objects_ref as OR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd._lib import DEBUG_CLEARANCE_PRUNE, check, lib  # noqa: E402
from stereo_depth_ruler_amd.ruler import (CLEARANCE_DTYPE, OBJECT_SCAN_DTYPE, PLANE_DTYPE,  # noqa: E402
                                          as_clearance_queries)

H, W = 360, 640
OBJ = dict(h_range=(10.0, 1000.0), max_diff=1.0, connectivity=8, min_pixels=64, max_objects=16)
BAND = (-20.0, 250.0)  # heights of the scene's surfaces above the floor: leaves the outliers out of the sets


def over_blocks(block_medians):
    a = np.asarray(block_medians, np.float64)
    return {"median_us": round(float(np.median(a)), 2), "lowest_block_us": round(float(a.min()), 2),
            "highest_block_us": round(float(a.max()), 2), "blocks": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_bench_c4.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    Qw = FR.scene_q(S.REFERENCE_Q)
    d, truth, _ = OR.two_object_scene(Qw, H=H, W=W)
    disp = torch.from_numpy(d).to(dev)
    r0, r2 = sdr.Ruler(Qw), sdr.Ruler(Qw, radius=2, min_count=9)
    planes_t, count, _, plab = r0.find_planes_device(disp, None, max_planes=3, hypotheses=256, min_inliers=1000,
                                                     labels=True)
    planes = planes_t.cpu().numpy().reshape(-1).view(PLANE_DTYPE)
    n_found = int(count.cpu()[0])
    floor = int(np.argmax([((plab.cpu().numpy() == i) & (truth == 0)).sum() for i in range(n_found)]))
    whole = (0, 0, 0, W - 1, H - 1, floor)
    _, scan_t, lab_t = r0.find_objects_device(disp, planes_t, whole + (-1,), labels_out=True, **OBJ)
    lab = lab_t.cpu().numpy()
    n_obj = int(scan_t.cpu().numpy().view(OBJECT_SCAN_DTYPE)[0]["count"])
    box_k, ball_k = (int(np.argmax([((lab == k) & (truth == t)).sum() for k in range(n_obj)])) for t in (1, 2))
    # two labels that split the frame: touching halves, and the outer thirds
    xx = np.broadcast_to(np.arange(W), (H, W))
    splits = {"touching": np.where(xx < W // 2, 0, 1).astype(np.uint8),
              "far_apart": np.where(xx < W // 3, 0, np.where(xx >= W - W // 3, 1, 255)).astype(np.uint8)}
    split_t = {k: torch.from_numpy(v).to(dev) for k, v in splits.items()}
    q_obj = torch.from_numpy(as_clearance_queries([whole + (box_k, ball_k)])).to(dev)
    q_split = torch.from_numpy(as_clearance_queries([whole + (0, 1)])).to(dev)
    xyz = sdr.reprojectImageTo3D(disp[0], Qw)  # (H, W, 3) on the device, for (c)
    valid = disp[0] > -1.0

    def call(ruler, q, labels, prune=True, h_range=None):
        def fn():
            check(lib().sdr_clearance_debug_knob(DEBUG_CLEARANCE_PRUNE, int(prune)))
            try:
                return ruler.clearance_device(disp, planes_t, q, labels, h_range=h_range).cpu()
            finally:
                check(lib().sdr_clearance_debug_knob(DEBUG_CLEARANCE_PRUNE, 1))
        return fn

    def cdist(labels, la, lb, chunk=None):
        def fn():
            pa, pb = xyz[(labels == la) & valid], xyz[(labels == lb) & valid]
            if chunk is None:
                return float(torch.cdist(pa, pb).min().cpu())
            best = torch.full((), float("inf"), device=dev)
            for i in range(0, pa.shape[0], chunk):
                best = torch.minimum(best, torch.cdist(pa[i:i + chunk], pb).min())
            return float(best.cpu())
        return fn

    def on_host():
        return CR.clearance(disp.cpu().numpy(), planes, [whole + (box_k, ball_k)], Qw, lab_t.cpu().numpy())

    cands = {"a_box_hemisphere_radius0": call(r0, q_obj, lab_t), "a_box_hemisphere_radius2_min9": call(r2, q_obj, lab_t),
             "c_cdist_min_box_hemisphere": cdist(lab_t, box_k, ball_k)}
    slow = {"d_frame_and_labels_to_host_numpy_box_hemisphere": on_host}
    for name, lt in split_t.items():
        cands[f"b_split_{name}_pruned"] = call(r0, q_split, lt)
        cands[f"b_split_{name}_every_block_pair"] = call(r0, q_split, lt, prune=False)
        cands[f"b_split_{name}_band_pruned"] = call(r0, q_split, lt, h_range=BAND)
        cands[f"b_split_{name}_band_every_block_pair"] = call(r0, q_split, lt, prune=False, h_range=BAND)
        slow[f"c_cdist_min_chunked_split_{name}"] = cdist(lt, 0, 1, chunk=4096)

    def rec(t):
        return t.numpy().reshape(-1).view(CLEARANCE_DTYPE)[0]

    records, agree = {}, {}
    for name, fn in cands.items():
        if name[0] != "c":
            r = rec(fn())
            records[name] = {k: (r[k].tolist() if hasattr(r[k], "tolist") else r[k]) for k in
                             ("distance", "along", "across", "xa", "ya", "xb", "yb", "n_a", "n_b", "m_a", "m_b", "flags")}
    agree["box_hemisphere_radius0"] = rec(cands["a_box_hemisphere_radius0"]()).tobytes() == on_host()[0].tobytes()
    for name in split_t:
        for band in ("", "_band"):
            agree[f"split_{name}{band}_pruned_equals_every_block_pair"] = (
                cands[f"b_split_{name}{band}_pruned"]().numpy().tobytes()
                == cands[f"b_split_{name}{band}_every_block_pair"]().numpy().tobytes())
    cdist_mm = {k: fn() for k, fn in list(cands.items()) + list(slow.items()) if k[0] == "c"}

    blocks = {k: [] for k in list(cands) + list(slow)}
    for _ in range(a.warmup):
        for fn in cands.values():
            fn()
    for _ in range(a.blocks):
        times = {k: [] for k in blocks}
        for rep in range(a.reps):
            for name, fn in list(cands.items()) + (list(slow.items()) if rep < a.slow_reps else []):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e6)
        for k, v in times.items():
            blocks[k].append(float(np.median(v)))
    result = {"map": [H, W], "disparity_frame_bytes": H * W * 4, "label_map_bytes": H * W,
              "reps_per_block": a.reps, "slow_reps_per_block": a.slow_reps, "planes_found": n_found, "floor_plane": floor,
              "objects_found": n_obj, "box_label": box_k, "hemisphere_label": ball_k,
              "truth_pixels": {"box": int((truth == 1).sum()), "hemisphere": int((truth == 2).sum())},
              "split_band_mm": list(BAND), "scratch_bytes": 21 * H * W + 304 * (H * W // 256 + 1) + 2048,
              "records": records, "cdist_min_mm": cdist_mm,
              "method": "host clock around call + copy-out of the record (synchronises); candidates alternated "
                        "round-robin inside a block; median over blocks of the block medians, with the lowest and "
                        "highest block",
              "device": torch.cuda.get_device_name(0), "agreement": agree,
              "candidates": {k: over_blocks(v) for k, v in blocks.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
