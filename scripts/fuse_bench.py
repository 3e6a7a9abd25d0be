#!/usr/bin/env python3
"""What the ruler over time costs: Ruler.fuse_device on stacks of F = 4, 8, 16, 32 frames of 640x360
(the noisy wall of tests/test_fuse_cpu.py: sigma 0.25 px on 1/16 px, 15 % holes, 3 % outliers), as
float32 and as int16, in both modes, with the record and without the two optional maps.

In one process, in blocks; inside a block the candidates alternate round-robin so that drift hits
every one alike.  A candidate's figure is the median over the blocks of the block's median, its
spread the lowest and highest block median.
  (1) the device call with its record: device events around --inner calls enqueued back to back, over
      their number.  `rotating`: every call reads another copy of the stack, the copies together
      larger than --rotate-mb (beyond the 256 MiB the last-level cache holds), so the reads come from
      HBM; `resident`: the same stack every call, as a loop that fuses what it has just computed
      finds it.  Also the host clock around one call and the copy-out of its 64-byte record.
  (2) the same rule in torch ops on the device, in the same run, with the same events: torch.sort
      along F, gather of the median, mask, sums (float64 sum in torch's order, not the frame order;
      its map is compared with the call's and the count of differing pixels reported).
  (3) the only route before: the stack copied out and the numpy restatement (tests/fuse_ref.py) run
      on it (MEAN only, --slow-reps repetitions a block, host clock; checked against (1) on every
      bit).
  (4) the call's algorithmic bytes (F * H * W elements read, 4 + 4 bytes a pixel and the record
      written) over its rotating time, and that rate over the 6.4 TB/s DESIGN.md measured for reads
      on this device.
  (5) LiveLoop at batch 8 on 1280x720 side-by-side frames (640x360 disparities): device events
      around a frame alone and around a frame with fuse() behind it.

usage: scripts/fuse_bench.py [--blocks 5] [--reps 10] [--out profiles/fuse_bench_c4.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import fuse_ref as FR  # noqa: E402
import stereo_depth_ruler_amd as sdr  # noqa: E402
from stereo_depth_ruler_amd import synthetic as S  # noqa: E402
from stereo_depth_ruler_amd.ruler import FUSION_DTYPE  # noqa: E402

H, W = 360, 640
HBM_READ_TBS = 6.4  # what a read-only stream reaches on this device
TOL, MIN_COUNT, MIN_DISP = 1.0, 2, -1.0


def wall_stack(F, seed=0):
    """F frames of the wall as int16 (1/16 px)."""
    rng = np.random.default_rng(seed)
    d = np.round((40.0 + rng.normal(0.0, 0.25, (F, H, W))) * 16)
    u = rng.random((F, H, W))
    d[u < 0.15] = -16
    out = (u >= 0.15) & (u < 0.18)
    d[out] = np.round(rng.uniform(1, 79, int(out.sum())) * 16)
    return d.astype(np.int16)


def over_blocks(block_medians):
    a = np.asarray(block_medians, np.float64)
    return {"median_us": round(float(np.median(a)), 2), "lowest_block_us": round(float(a.min()), 2),
            "highest_block_us": round(float(a.max()), 2), "blocks": len(a)}


def torch_fuse(stack, mode):
    """The rule in torch ops: (fused (H, W), record counts as a tensor)."""
    v = stack.float() * 0.0625 if stack.dtype == torch.int16 else stack
    ok = torch.isfinite(v) & (v > MIN_DISP)
    key = torch.where(ok, v, torch.full_like(v, float("inf")))
    srt, _ = torch.sort(key, dim=0, stable=True)
    n = ok.sum(0)
    m = srt.gather(0, ((n - 1).clamp(min=0) // 2)[None])[0]
    agree = ok & ((v - m[None]).abs() <= TOL)
    n_in = agree.sum(0)
    fused = n_in >= MIN_COUNT
    if mode == FR.MEDIAN:
        val = m
    else:
        val = (torch.where(agree, v.double(), torch.zeros((), dtype=torch.float64, device=v.device)).sum(0)
               / n_in.clamp(min=1)).float()
    out = torch.where(fused, val, torch.full_like(val, MIN_DISP))
    last_ok, last_in = ok[-1], agree[-1]
    counts = torch.stack([fused.sum(), (n == 0).sum(), (~fused & (n > 0) & (n < MIN_COUNT)).sum(),
                          (~fused & (n >= MIN_COUNT)).sum(), (fused & ~last_ok).sum(),
                          (fused & last_ok & ~last_in).sum(), (n_in * fused).sum(), ((n - n_in) * fused).sum()])
    return out, counts


def live_loop(batch):
    from stereo_depth_ruler_amd.pipeline import LiveLoop
    from stereo_depth_ruler_amd.rectify import StereoRectifier

    fw, fh = 2 * W, 2 * H
    sbs = S.sbs_bgr_frame(fh, fw, 80, seed=21)
    rng = np.random.default_rng(4)
    frames = np.clip(sbs[None].astype(np.int16) + rng.integers(-3, 4, (batch,) + sbs.shape), 0, 255).astype(np.uint8)
    K = np.array([[700.0, 0, fw / 2], [0, 700.0, fh / 2], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    cfg = types.SimpleNamespace(imageSize=(fw, fh), cameraMatrixLeft=K, cameraMatrixRight=K, distCoeffsLeft=None,
                                distCoeffsRight=None, R1=np.eye(3), R2=np.eye(3), P1=P, P2=P)
    rect = StereoRectifier(cfg)
    loop = LiveLoop(rect, S.REFERENCE_Q, batch, ruler=dict(conf_min=100.0))
    return loop, torch.from_numpy(frames).cuda(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-reps", type=int, default=1)
    ap.add_argument("--rotate-mb", type=int, default=600)
    ap.add_argument("--frames", type=int, nargs="*", default=[4, 8, 16, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench_c4.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    r = sdr.Ruler(S.REFERENCE_Q, min_disp=MIN_DISP)
    stream = torch.cuda.current_stream(dev)

    def events(fn, inner):
        """us a call of `inner` calls enqueued back to back."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(inner):
            fn(i)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner

    def host_clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    result = {"map": [H, W], "tol": TOL, "min_count": MIN_COUNT, "reps_per_block": a.reps, "inner_calls": a.inner,
              "slow_reps_per_block": a.slow_reps, "rotate_mb": a.rotate_mb, "hbm_read_tb_s": HBM_READ_TBS,
              "device": torch.cuda.get_device_name(0), "stacks": {}}
    for F in a.frames:
        s16 = wall_stack(F)
        for dname, host in (("float32", s16.astype(np.float32) * np.float32(0.0625)), ("int16", s16)):
            one = torch.from_numpy(host).to(dev)
            copies = max(2, -(-a.rotate_mb * (1 << 20) // host.nbytes))
            ring = [one] + [one.clone() for _ in range(copies - 1)]
            out = torch.empty((H, W), dtype=torch.float32, device=dev)
            algo_bytes = host.nbytes + 8 * H * W + 64
            entry = {"frames": F, "dtype": dname, "stack_bytes": host.nbytes, "copies_rotated": copies,
                     "algorithmic_bytes": algo_bytes, "modes": {}}
            for mname, mode in (("mean", FR.MEAN), ("median", FR.MEDIAN)):
                kw = dict(tol=TOL, min_count=MIN_COUNT, mode=mode, out=out)
                cands = {
                    "1_call_rotating": lambda: events(lambda i: r.fuse_device(ring[i % copies], **kw), a.inner),
                    "1_call_resident": lambda: events(lambda i: r.fuse_device(one, **kw), a.inner),
                    "1_call_and_record_to_host": lambda: host_clock(lambda: r.fuse_device(one, **kw)[1].cpu()),
                    "2_torch_ops_resident": lambda: events(lambda i: torch_fuse(one, mode), max(a.inner // 4, 1)),
                }
                slow = {}
                if mode == FR.MEAN:
                    slow["3_stack_to_host_numpy"] = lambda: host_clock(
                        lambda: FR.fuse(one.cpu().numpy(), tol=TOL, min_count=MIN_COUNT, mode=mode))
                # what the candidates compute
                fused, rec = r.fuse_device(one, **kw)
                got = fused.cpu().numpy()[0].copy()
                grec = rec.cpu().numpy().view(FUSION_DTYPE)[0]
                want = FR.fuse(host, tol=TOL, min_count=MIN_COUNT, mode=mode)
                t_out, t_counts = torch_fuse(one, mode)
                agree = {"call_equals_numpy_bits": bool(np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
                                                        and grec.tobytes() == want[1].tobytes()),
                         "torch_pixels_differing": int((t_out.cpu().numpy().view(np.uint32) != got.view(np.uint32)).sum()),
                         "torch_counts_equal": t_counts.cpu().tolist() == [int(grec[k]) for k in FUSION_DTYPE.names[4:12]]}
                blocks = {k: [] for k in list(cands) + list(slow)}
                for _ in range(a.warmup):
                    for fn in cands.values():
                        fn()
                for _ in range(a.blocks):
                    times = {k: [] for k in blocks}
                    for rep in range(a.reps):
                        for name, fn in list(cands.items()) + (list(slow.items()) if rep < a.slow_reps else []):
                            times[name].append(fn())
                    for k, v in times.items():
                        blocks[k].append(float(np.median(v)))
                c = {k: over_blocks(v) for k, v in blocks.items()}
                rate = algo_bytes / (c["1_call_rotating"]["median_us"] * 1e-6) / 1e12
                entry["modes"][mname] = {
                    "record": {k: int(grec[k]) for k in FUSION_DTYPE.names[:12]}, "agreement": agree, "candidates": c,
                    "4_algorithmic_tb_s_rotating": round(rate, 3),
                    "4_fraction_of_hbm_read_rate": round(rate / HBM_READ_TBS, 3)}
                print(F, dname, mname, json.dumps(entry["modes"][mname]["candidates"]), flush=True)
            result["stacks"][f"F{F}_{dname}"] = entry
            del ring

    # (5) the live loop with and without a fuse behind the frame
    batch = 8
    loop, frames = live_loop(batch)
    side = torch.cuda.Stream(dev)
    side.wait_stream(stream)

    def frame_only():
        loop.enqueue(frames, side)

    def frame_and_fuse():
        loop.enqueue(frames, side)
        loop.fuse(side, tol=TOL, min_count=MIN_COUNT)

    def loop_events(fn, inner=4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record(side)
            for _ in range(inner):
                fn()
            e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner

    cands = {"5_live_loop_batch8_frame": lambda: loop_events(frame_only),
             "5_live_loop_batch8_frame_and_fuse": lambda: loop_events(frame_and_fuse)}
    blocks = {k: [] for k in cands}
    for _ in range(a.warmup):
        for fn in cands.values():
            fn()
    for _ in range(a.blocks):
        times = {k: [] for k in cands}
        for _ in range(a.reps):
            for name, fn in cands.items():
                times[name].append(fn())
        for k, v in times.items():
            blocks[k].append(float(np.median(v)))
    with torch.cuda.stream(side):
        rec = loop.fuse(side, tol=TOL, min_count=MIN_COUNT)[1]
    side.synchronize()
    grec = rec.cpu().numpy().view(FUSION_DTYPE)[0]
    result["live_loop"] = {"batch": batch, "sbs_frame": [2 * H, 4 * W, 3], "disparity": [loop.h2, loop.w2],
                           "record": {k: int(grec[k]) for k in FUSION_DTYPE.names[:12]},
                           "candidates": {k: over_blocks(v) for k, v in blocks.items()}}
    loop.close()
    result["method"] = ("device events around `inner_calls` calls enqueued back to back (the live loop: 4 frames), "
                        "over their number; host clock where a copy-out ends the call; candidates alternated "
                        "round-robin inside a block; median over blocks of the block medians, with the lowest and "
                        "highest block")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["live_loop"]))


if __name__ == "__main__":
    main()
