"""Time the encoder's view of its source (encode_frames(select=, crop=, size=): AGMV_EncodeViewDev of include/agmv.h) on one MI355X, in
one process.  HIP events around K launches (or K runs of a front end), the median and min..max of REPS timings behind one warm-up:
  1  k_view_src alone (agmv_hip_view_source_async) on T1 resident 1920 x 1080 frames, the centred 1440 x 1080 window of every
     frame, per layout; XRGB32 is k_view.  Traffic = the window's bytes read in the source's layout + the bytes written, over the
     time, beside the 8 TB/s HBM peak
  2  the front end of 1080p NV12 -> 240 x 160 at a quarter of the frame rate, on T2 frames: what stands between the caller's
     tensor and D, the XRGB32 clip at the target's size that the encoder runs on.  The view: per staging batch one
     agmv_hip_view_source_async and one agmv_hip_scale_area_dev on the batch as an XRGB32 source, the launches AGMV_EncodeViewDev
     makes.  The detour without a view: both planes sliced, joined and made contiguous by torch, then agmv_hip_scale_area_dev on
     that NV12 clip, which is what encode_frames(size=) runs first.  Time to have D and the peak of
     torch.cuda.max_memory_allocated above the source; both give the same D, which is checked
  3  the whole call, both ways, once each for the wall time, and AGMV_GetEncodeViewStats of the view's
usage: view_source_time.py [T1=256] [T2=1024] [reps=5]"""
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

T1 = int(sys.argv[1]) if len(sys.argv) > 1 else 256
T2 = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
K = 10
W, H = 1920, 1080
X0, Y0, WW, WH = 240, 0, 1440, 1080
STEP, DW, DH = 4, 240, 160
STAGE_BYTES = 256 << 20
HBM = 8.0e12
# name -> (bytes per pixel read, shape of T frames, dtype)
LAYOUTS = {"xrgb32": (4, lambda t: (t, H, W), torch.int32), "rgb24": (3, lambda t: (t, H, W, 3), torch.uint8), "bgr24": (3, lambda t: (t, H, W, 3), torch.uint8),
           "rgba32": (4, lambda t: (t, H, W, 4), torch.uint8), "rgb8p": (3, lambda t: (t, 3, H, W), torch.uint8),
           "nv12": (1.5, lambda t: (t, H * 3 // 2, W), torch.uint8), "i420": (1.5, lambda t: (t, H * 3 // 2, W), torch.uint8)}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = [events(fn) for _ in range(REPS)]
    return float(np.median(ts)), min(ts), max(ts)


def peak_above(fn):
    """the peak of torch's allocations over one run of fn above what is allocated before it, and fn's result"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def nv12_clip(hip, t):
    """t frames of agmv_synth_v1 at 1920 x 1080 as NV12, made 64 frames at a time"""
    out = torch.empty((t, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    for f0 in range(0, t, 64):
        n = min(64, t - f0)
        hip.yuv_from_xrgb_dev("nv12", hip.synth_dev(W, H, 1 + f0, n).reshape(n, W * H), W, H, out=out[f0:f0 + n].reshape(n, -1))
    torch.cuda.synchronize()
    return out


def main():
    hip = AgmvHip(0)
    print("-- 1: k_view_src alone: %d x %dx%d resident frames, the %d x %d window at (%d, %d) of every frame; K = %d launches per timing, median of %d"
          % (T1, W, H, WW, WH, X0, Y0, K, REPS), flush=True)
    out = torch.empty((T1, WH, WW), dtype=torch.int32, device="cuda")
    for name, (bpp, shape, dtype) in LAYOUTS.items():
        src = torch.randint(0, 256, shape(T1), dtype=torch.uint8, device="cuda") if dtype == torch.uint8 else torch.randint(0, 1 << 24, shape(T1), dtype=dtype, device="cuda")
        fn = lambda: hip.view_source(name, src, W, H, 0, 1, T1, X0, Y0, WW, WH, out=out)
        ms, lo, hi = timed(fn)
        moved = (bpp + 4) * WW * WH * T1
        print("%-7s median of %d = %8.4f ms (min %.4f .. max %.4f); %.3f GB read + written = %.2f TB/s = %.0f %% of the 8 TB/s HBM peak"
              % (name, REPS, ms, lo, hi, moved / 1e9, moved / ms / 1e9, 100 * moved / (ms * 1e-3) / HBM), flush=True)
        del src
    del out
    torch.cuda.empty_cache()

    n = len(range(0, T2, STEP))
    stage = max(1, STAGE_BYTES // (4 * WW * WH))
    print("-- 2: the front end of %d x %dx%d NV12 -> every %dth frame, the %d x %d window at (%d, %d), area to %d x %d: %d frames of D; staging batches of %d windows"
          % (T2, W, H, STEP, WW, WH, X0, Y0, DW, DH, n, stage), flush=True)
    src = nv12_clip(hip, T2)

    def view():
        d = torch.empty((n, DH, DW), dtype=torch.int32, device="cuda")
        staging = torch.empty((min(stage, n), WH, WW), dtype=torch.int32, device="cuda")
        for j in range(0, n, stage):
            nb = min(stage, n - j)
            hip.view_source("nv12", src, W, H, j * STEP, STEP, nb, X0, Y0, WW, WH, out=staging)
            hip.scale_area_dev("xrgb32", staging, WW, WH, nb, DW, DH, out=d[j:j + nb])
        return d

    def detour():
        luma, chroma = src[::STEP, :H, X0:X0 + WW], src[::STEP, H:, X0:X0 + WW]
        joined = torch.cat((luma, chroma), dim=1).contiguous()
        return hip.scale_area_dev("nv12", joined, WW, WH, n, DW, DH)

    a, b = view(), detour()
    assert a.shape == b.shape == (n, DH, DW) and torch.equal(a, b), "the two front ends give different clips"
    del a, b
    for name, fn in (("view", view), ("detour", detour)):
        peak, d = peak_above(fn)
        del d
        ms, lo, hi = timed(fn)
        print("%-7s time to have D: median of %d = %8.3f ms (min %.3f .. max %.3f); peak allocated above the source %.3f GB" % (name, REPS, ms, lo, hi, peak / 1e9), flush=True)

    print("-- 3: the whole call on the same clip, once each (OPT_III, PDIFS, LZSS)", flush=True)
    tmp = tempfile.mkdtemp()
    for name, fn in (("view", lambda p: libagmv_amd.encode_frames(p, src, fmt="nv12", select=slice(None, None, STEP), crop=(Y0, X0, WH, WW), size=(DH, DW))),
                     ("detour", lambda p: libagmv_amd.encode_frames(p, torch.cat((src[::STEP, :H, X0:X0 + WW], src[::STEP, H:, X0:X0 + WW]), dim=1).contiguous(),
                                                                   fmt="nv12", size=(DH, DW)))):
        for rep in ("warm-up", "timed"):
            path = os.path.join(tmp, "%s_%s.agmv" % (name, rep))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(path)
            s = time.perf_counter() - t0
        print("%-7s wall %.3f s, file %.2f MB" % (name, s, os.path.getsize(path) / 1e6), flush=True)
        if name == "view":
            print("        AGMV_GetEncodeViewStats: frames %d, clip_bytes %d, staging_bytes %d" % libagmv_amd.encode_view_stats(), flush=True)
    same = open(os.path.join(tmp, "view_timed.agmv"), "rb").read() == open(os.path.join(tmp, "detour_timed.agmv"), "rb").read()
    print("the two files are %s" % ("equal" if same else "DIFFERENT"), flush=True)


if __name__ == "__main__":
    main()
