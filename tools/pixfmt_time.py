"""Time the kernels that read and write a clip in the caller's pixel layout, on T x 1920x1080 agmv_synth_v1 frames resident on the
GPU, in one process: warm-up first, HIP events around K back-to-back launches, median and min..max of REPS, the two sides of
every comparison alternated.
  1  agmv_hip_pixels_to_xrgb_dev / _from_xrgb_dev for RGB24, BGR24, RGBA32, RGB8P, and agmv_hip_histogram_fmt_dev /
     agmv_hip_similarity_fmt_dev beside the packed kernels they generalise: time, algorithmic bytes over time, share of the
     8 TB/s HBM peak
  2  the comparator: the torch expression a caller had to write before, (r.int() << 16) | (g.int() << 8) | b.int() on the same
     uint8 [T, H, W, 3] tensor, and its inverse; both routes must give the same bytes
  3  end to end: AGMV_EncodeFramesFmtDev(RGB24) against torch packing + AGMV_EncodeFramesDev, same clip, same file, host LZ
     pool; wall time and the peak extra device memory of each route (free memory before against its lowest point during the
     call, torch.cuda.mem_get_info polled from a thread)
usage: pixfmt_time.py [T=256] [reps=5]"""
import hashlib
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
W, Hh = 1920, 1080
NPX = W * Hh
HBM_PEAK = 8e12
BPP = {"xrgb32": 4, "rgb24": 3, "bgr24": 3, "rgba32": 4, "rgb8p": 3}


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
    s = "%-46s median of %d = %8.3f ms (min %.3f .. max %.3f)" % (name, len(ts), ms, min(ts), max(ts))
    if nbytes:
        s += "; %.2f GB = %.2f TB/s = %.0f %% of the 8 TB/s HBM peak" % (nbytes / 1e9, nbytes / ms / 1e9, 100 * nbytes / (ms * 1e-3) / HBM_PEAK)
    print(s, flush=True)


def torch_pack(rgb):
    return (rgb[..., 0].int() << 16) | (rgb[..., 1].int() << 8) | rgb[..., 2].int()


def torch_unpack(p):
    return torch.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], dim=-1).to(torch.uint8)


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
    print("clip: %d x %dx%d agmv_synth_v1, K = %d launches per timing, %d repetitions, the sides of a comparison alternated" % (T, W, Hh, K, REPS), flush=True)

    print("-- 1: the kernels", flush=True)
    clips = {}
    for name in ("rgb24", "bgr24", "rgba32", "rgb8p"):
        clips[name] = hip.pixels_from_xrgb_dev(name, packed)
    out = torch.empty_like(packed)
    sides, moved = [], {}
    for name, c in clips.items():
        sides.append(("%s -> xrgb32 (k_pix_to_xrgb)" % name, lambda name=name, c=c: hip.pixels_to_xrgb_dev(name, c, NPX, T, out=out)))
        sides.append(("xrgb32 -> %s (k_pix_from_xrgb)" % name, lambda name=name, c=c: hip.pixels_from_xrgb_dev(name, packed, out=c)))
        moved[sides[-1][0]] = moved[sides[-2][0]] = T * NPX * (4 + BPP[name])          # read once, written once
    res = alternate(sides)
    for name, _ in sides:
        line(name, res[name], moved[name])
    for name, c in clips.items():                             # the round trip gives the packed clip back
        assert torch.equal(hip.pixels_to_xrgb_dev(name, c, NPX, T), packed), name
    hist = torch.zeros(1 << 19, dtype=torch.int32, device="cuda")
    counts = torch.empty(T - 1, dtype=torch.int32, device="cuda")
    sides = [("xrgb32 histogram (k_histogram)", lambda: hip.histogram_dev(packed, 3, hist)),
             ("xrgb32 similarity (k_similarity)", lambda: hip.similarity_dev(packed, counts))]
    for name, c in clips.items():
        sides.append(("%s histogram (k_histogram_fmt)" % name, lambda name=name, c=c: hip.histogram_fmt_dev(name, c, NPX, T, NPX, 3, hist)))
        sides.append(("%s similarity (k_similarity_fmt)" % name, lambda name=name, c=c: hip.similarity_fmt_dev(name, c, T, NPX, counts)))
    res = alternate(sides)
    for name, _ in sides:
        line(name, res[name], T * NPX * BPP[name.split(" ")[0]])
    ref_h, ref_c = hip.histogram_dev(packed, 3), hip.similarity_dev(packed).clone()
    for name, c in clips.items():
        assert torch.equal(hip.histogram_fmt_dev(name, c, NPX, T, NPX, 3), ref_h) and torch.equal(hip.similarity_fmt_dev(name, c, T, NPX), ref_c), name
    print("every format: same histogram and same counts as the packed kernels", flush=True)

    print("-- 2: RGB24 <-> XRGB32 against the torch expressions on the same uint8 [T, H, W, 3] tensor", flush=True)
    rgb = clips["rgb24"].reshape(T, Hh, W, 3)
    assert torch.equal(torch_pack(rgb).reshape(T, NPX), hip.pixels_to_xrgb_dev("rgb24", clips["rgb24"], NPX, T))
    assert torch.equal(torch_unpack(packed).reshape(T, -1), clips["rgb24"])
    res = alternate([("k_pix_to_xrgb rgb24", lambda: hip.pixels_to_xrgb_dev("rgb24", clips["rgb24"], NPX, T, out=out)),
                     ("torch (r.int() << 16) | (g.int() << 8) | b.int()", lambda: torch_pack(rgb)),
                     ("k_pix_from_xrgb rgb24", lambda: hip.pixels_from_xrgb_dev("rgb24", packed, out=clips["rgb24"])),
                     ("torch stack of shifts .to(uint8)", lambda: torch_unpack(packed))])
    for name, ts in res.items():
        line(name, ts, T * NPX * 7 if name.startswith("k_") else None)
    k, t = res["k_pix_to_xrgb rgb24"], res["torch (r.int() << 16) | (g.int() << 8) | b.int()"]
    print("RGB24 -> XRGB32: kernel %.3f .. %.3f ms, torch %.3f .. %.3f ms: the kernel's range lies %s torch's" %
          (min(k), max(k), min(t), max(t), "entirely below" if max(k) < min(t) else "NOT entirely below"), flush=True)
    k, t = res["k_pix_from_xrgb rgb24"], res["torch stack of shifts .to(uint8)"]
    print("XRGB32 -> RGB24: kernel %.3f .. %.3f ms, torch %.3f .. %.3f ms: the kernel's range lies %s torch's" %
          (min(k), max(k), min(t), max(t), "entirely below" if max(k) < min(t) else "NOT entirely below"), flush=True)

    print("-- 3: end to end, %d x %dx%d, OPT_III, LOW quality, LZSS on the host pool, AGMV_SCHEDULE_FULL" % (T, W, Hh), flush=True)
    rgb = rgb.clone()
    del clips, out, packed, hist, counts
    shas = {}

    def route_fmt(path):
        seq.encode_frames(path, rgb, opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL)

    def route_torch(path):
        seq.encode_frames(path, torch_pack(rgb), opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL)

    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        times = {"AGMV_EncodeFramesFmtDev(RGB24)": [], "torch packing + AGMV_EncodeFramesDev": []}
        extra = {k: 0 for k in times}
        for name, fn in (("AGMV_EncodeFramesFmtDev(RGB24)", route_fmt), ("torch packing + AGMV_EncodeFramesDev", route_torch)):
            fn("warm.agmv")                                   # warm-up: contexts, tables, the pool
        for _ in range(REPS):
            for name, fn in (("AGMV_EncodeFramesFmtDev(RGB24)", route_fmt), ("torch packing + AGMV_EncodeFramesDev", route_torch)):
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
                shas.setdefault(name, set()).add(hashlib.sha256(open("out.agmv", "rb").read()).hexdigest())
        os.chdir(R)
    for name, ts in times.items():
        ms = float(np.median(ts))
        print("%-40s wall, median of %d = %8.1f ms (min %.1f .. max %.1f) = %.1f frames/s; peak extra device memory %.2f GB" %
              (name, len(ts), ms, min(ts), max(ts), T / (ms * 1e-3), extra[name] / 1e9), flush=True)
    all_shas = set().union(*shas.values())
    print("both routes wrote the same file every time: %s (sha256 %s...)" % (len(all_shas) == 1, sorted(all_shas)[0][:16]), flush=True)
    assert len(all_shas) == 1


if __name__ == "__main__":
    main()
