"""Time the exact box-filter downscale (agmv_hip_scale_area_dev, AGMV_SCALE_AREA of include/agmv.h) on T x 1920x1080 -> 320x240
agmv_synth_v1 frames resident on the GPU, per layout, in one process: warm-up first, HIP events around K back-to-back launches,
median and min..max of REPS, the two sides of every comparison alternated (the method of tools/pixfmt_time.py).
  1  agmv_hip_scale_area_dev: time, and the algorithmic bytes (source bytes + 4 * 320 * 240 per frame) over time as a share of
     the 8 TB/s HBM peak
  2  the yardstick: the existing conversion of the same clip to XRGB32 (agmv_hip_pixels_to_xrgb_dev / agmv_hip_yuv_to_xrgb_dev;
     for XRGB32 a device-to-device copy), which reads the same source bytes with the same per-pixel reading; the ratio of the two
  3  torch's interpolate(mode="area") of the RGB24 clip in float: time and peak extra device memory only (it is not exact and its
     pixels are not compared)
  4  end to end: AGMV_EncodeFramesScaledDev(RGB24) against the torch scale followed by AGMV_EncodeFramesDev: wall time and peak
     extra device memory (the files differ: torch's scale is not the library's)
usage: scale_time.py [T=256] [reps=5]"""
import os
import sys
import tempfile
import threading
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip, seq

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 10
W, Hh, DW, DH = 1920, 1080, 320, 240
NPX = W * Hh
HBM_PEAK = 8e12
LAYOUTS = ["xrgb32", "rgb24", "bgr24", "rgba32", "rgb8p", "nv12", "i420"]
FRAME_BYTES = {"xrgb32": 4 * NPX, "rgb24": 3 * NPX, "bgr24": 3 * NPX, "rgba32": 4 * NPX, "rgb8p": 3 * NPX, "nv12": NPX * 3 // 2, "i420": NPX * 3 // 2}


def timed(fn):
    """ms per call: K calls between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K


def alternate(sides):
    """sides: [(name, fn)]; each rep runs every side once, in turn; returns {name: [ms] * REPS}"""
    for _, fn in sides:
        fn()                                                  # warm-up of every shape
    torch.cuda.synchronize()
    out = {name: [] for name, _ in sides}
    for _ in range(REPS):
        for name, fn in sides:
            out[name].append(timed(fn))
    return out


def line(name, ts, nbytes=None):
    ms = float(np.median(ts))
    s = "%-44s median of %d = %8.3f ms (min %.3f .. max %.3f)" % (name, len(ts), ms, min(ts), max(ts))
    if nbytes:
        s += "; %.2f GB = %.2f TB/s = %.0f %% of the 8 TB/s HBM peak" % (nbytes / 1e9, nbytes / ms / 1e9, 100 * nbytes / (ms * 1e-3) / HBM_PEAK)
    print(s, flush=True)


def torch_area(rgb):
    """uint8 [T, H, W, 3] -> int32 [T, DH, DW] of 0x00RRGGBB through float32 (rounded to nearest; not the library's integers)"""
    x = torch.nn.functional.interpolate(rgb.permute(0, 3, 1, 2).float(), size=(DH, DW), mode="area")
    x = x.round_().clamp_(0, 255).to(torch.int32)
    return (x[:, 0] << 16) | (x[:, 1] << 8) | x[:, 2]


class LowestFree(threading.Thread):
    """polls the free device memory while a blocking library call runs in the main thread"""

    def __init__(self):
        super().__init__(daemon=True)
        self.low = torch.cuda.mem_get_info()[0]
        self.stop = False

    def run(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.002)


def main():
    hip = AgmvHip(0)
    packed = hip.synth_dev(W, Hh, 1, T).reshape(T, NPX)
    print("clip: %d x %dx%d agmv_synth_v1 -> %dx%d, K = %d launches per timing, %d repetitions, the sides of a comparison alternated"
          % (T, W, Hh, DW, DH, K, REPS), flush=True)

    print("-- 1, 2: agmv_hip_scale_area_dev beside the conversion of the same clip to XRGB32, per layout", flush=True)
    small = torch.empty((T, DH, DW), dtype=torch.int32, device="cuda")
    full = torch.empty_like(packed)
    ratios = {}
    for name in LAYOUTS:
        if name == "xrgb32":
            clip = packed
            convert = lambda: hip.pixels_to_xrgb_dev("xrgb32", clip, NPX, T, out=full)
        elif name in ("nv12", "i420"):
            clip = hip.yuv_from_xrgb_dev(name, packed, W, Hh)
            convert = lambda: hip.yuv_to_xrgb_dev(name, clip, W, Hh, T, out=full)
        else:
            clip = hip.pixels_from_xrgb_dev(name, packed)
            convert = lambda: hip.pixels_to_xrgb_dev(name, clip, NPX, T, out=full)
        scale = lambda: hip.scale_area_dev(name, clip, W, Hh, T, DW, DH, out=small)
        res = alternate([("%s area scale (k_scale_area)" % name, scale), ("%s -> xrgb32 (the conversion)" % name, convert)])
        a, b = res["%s area scale (k_scale_area)" % name], res["%s -> xrgb32 (the conversion)" % name]
        line("%s area scale (k_scale_area)" % name, a, T * (FRAME_BYTES[name] + 4 * DW * DH))
        line("%s -> xrgb32 (the conversion)" % name, b, T * (FRAME_BYTES[name] + 4 * NPX))
        ratios[name] = float(np.median(a)) / float(np.median(b))
        print("%s: area scale / conversion = %.2f (medians)" % (name, ratios[name]), flush=True)
        # the scale of the layout is the scale of the clip it stands for
        convert()
        assert torch.equal(hip.scale_area_dev("xrgb32", full, W, Hh, T, DW, DH), hip.scale_area_dev(name, clip, W, Hh, T, DW, DH)), name
        del clip
    print("ratios area scale / conversion: " + ", ".join("%s %.2f" % (n, ratios[n]) for n in LAYOUTS), flush=True)

    print("-- 3: torch interpolate(mode=\"area\") of the RGB24 clip in float32 (not exact; pixels not compared)", flush=True)
    rgb = hip.pixels_from_xrgb_dev("rgb24", packed).reshape(T, Hh, W, 3)
    del full, packed
    torch.cuda.empty_cache()
    torch_area(rgb)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = alternate([("torch interpolate(mode=\"area\") via float32", lambda: torch_area(rgb)),
                     ("rgb24 area scale (k_scale_area)", lambda: hip.scale_area_dev("rgb24", rgb, W, Hh, T, DW, DH, out=small))])
    for name, ts in res.items():
        line(name, ts)
    print("torch route: peak extra device memory %.2f GB (the kernel: none beyond its %.3f GB result)"
          % ((torch.cuda.max_memory_allocated() - base) / 1e9, small.numel() * 4 / 1e9), flush=True)

    print("-- 4: end to end, %d x %dx%d -> %dx%d, OPT_III, LOW quality, LZSS on the host pool, AGMV_SCHEDULE_FULL" % (T, W, Hh, DW, DH), flush=True)
    del small
    routes = (("AGMV_EncodeFramesScaledDev(RGB24, AREA)", lambda p: seq.encode_frames(p, rgb, opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL, size=(DH, DW))),
              ("torch area scale + AGMV_EncodeFramesDev", lambda p: seq.encode_frames(p, torch_area(rgb), opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL)))
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        times = {name: [] for name, _ in routes}
        extra = {name: 0 for name, _ in routes}
        for name, fn in routes:
            fn("warm.agmv")                                   # warm-up: contexts, tables, the pool
        for _ in range(REPS):
            for name, fn in routes:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                before = torch.cuda.mem_get_info()[0]
                watch = LowestFree()
                watch.start()
                t0 = time.perf_counter()
                fn("out.agmv")
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
                watch.stop = True
                watch.join()
                extra[name] = max(extra[name], before - watch.low)
        os.chdir(R)
    for name, ts in times.items():
        ms = float(np.median(ts))
        print("%-42s wall, median of %d = %8.1f ms (min %.1f .. max %.1f) = %.1f frames/s; peak extra device memory %.2f GB" %
              (name, len(ts), ms, min(ts), max(ts), T / (ms * 1e-3), extra[name] / 1e9), flush=True)


if __name__ == "__main__":
    main()
