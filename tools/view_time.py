"""Time a view of a file (decode_frames(frames=, crop=): AGMV_DecodeViewTensorDev of include/agmv.h) on a T-frame 1920x1080 file of
agmv_synth_v1 frames, in one process, warm-up first, median and min..max of REPS, the sides alternated (the method of
tools/upscale_time.py):
  1  16 frames at stride 4 from frame 120, a 224 x 224 window, as F16 with the ImageNet normalisation: the view against the way
     without one, decode_frames(path, fmt="f16") followed by [120:184:4, :, y:y+224, x:x+224].contiguous().  Wall time of the
     call and the peak of torch.cuda.max_memory_allocated over it; both give the same bits, which is checked
  2  k_view alone (agmv_hip_view_frames_async) on T x 1080p resident frames: the 224 x 224 window of every frame, and the full
     frame of every fourth, HIP events around K launches, as a share of the HBM bound -- the bytes moved are twice the output,
     over the 8 TB/s peak
usage: view_time.py [T=256] [reps=5]"""
import os
import sys
import tempfile
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

import libagmv_amd
from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 10
W, H = 1920, 1080
FIRST, STOP, STEP, Y0, X0, WIN = 120, 184, 4, 428, 848, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM = 8.0e12


def wall(fn):
    """(seconds, peak bytes allocated over the call, its result)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base, out


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K


def main():
    hip = AgmvHip(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "clip.agmv")
    clip = hip.synth_dev(W, H, 1, T).reshape(T, H, W)
    t0 = time.perf_counter()
    libagmv_amd.encode_frames(path, clip, schedule=libagmv_amd.SCHEDULE_FULL)
    print("file: %d x %dx%d agmv_synth_v1, %.1f MB, encoded in %.1f s; %d repetitions, the sides alternated" % (T, W, H, os.path.getsize(path) / 1e6, time.perf_counter() - t0, REPS),
          flush=True)
    del clip
    view = lambda: libagmv_amd.decode_frames(path, fmt="f16", mean=MEAN, std=STD, frames=range(FIRST, STOP, STEP), crop=(Y0, X0, WIN, WIN))[0]
    detour = lambda: libagmv_amd.decode_frames(path, fmt="f16", mean=MEAN, std=STD)[0][FIRST:STOP:STEP, :, Y0:Y0 + WIN, X0:X0 + WIN].contiguous()
    print("-- 1: frames %d:%d:%d, window %d x %d at (%d, %d), F16: the view against the full decode sliced by torch" % (FIRST, STOP, STEP, WIN, WIN, X0, Y0), flush=True)
    a, b = view(), detour()
    assert a.shape == b.shape == (len(range(FIRST, STOP, STEP)), 3, WIN, WIN) and torch.equal(a.view(torch.int16), b.view(torch.int16))
    del a, b
    res = {"view": [], "detour": []}
    for _ in range(REPS):
        for name, fn in (("view", view), ("detour", detour)):
            s, peak, out = wall(fn)
            del out
            res[name].append((s, peak))
    for name in ("view", "detour"):
        ts = [r[0] for r in res[name]]
        print("%-8s wall median of %d = %8.3f s (min %.3f .. max %.3f); peak device memory allocated by torch %.3f GB"
              % (name, REPS, float(np.median(ts)), min(ts), max(ts), max(r[1] for r in res[name]) / 1e9), flush=True)
    print("detour / view = %.2f in wall time (medians)" % (np.median([r[0] for r in res["detour"]]) / np.median([r[0] for r in res["view"]])), flush=True)

    print("-- 2: k_view alone on %d resident frames, K = %d launches per timing" % (T, K), flush=True)
    src = hip.synth_dev(W, H, 1, T)
    for name, (first, step, count, x, y, w, h) in (("224 x 224 window of every frame", (0, 1, T, X0, Y0, WIN, WIN)),
                                                  ("full frame of every fourth", (0, 4, T // 4, 0, 0, W, H))):
        out = torch.empty((count, h, w), dtype=torch.int32, device="cuda")
        fn = lambda: hip.view_frames_async(src, W, H, first, step, count, x, y, w, h, out=out)
        fn()
        ts = [events(fn) for _ in range(REPS)]
        ms, moved = float(np.median(ts)), 2 * out.numel() * 4
        print("%-34s median of %d = %8.4f ms (min %.4f .. max %.4f); %.3f GB moved = %.2f TB/s = %.0f %% of the 8 TB/s HBM peak"
              % (name, REPS, ms, min(ts), max(ts), moved / 1e9, moved / ms / 1e9, 100 * moved / (ms * 1e-3) / HBM), flush=True)


if __name__ == "__main__":
    main()
