"""Time the kernels that read and write a clip in 8-bit YUV 4:2:0 (NV12, I420), on T x 1920x1080 agmv_synth_v1 frames resident on
the GPU, in one process: warm-up of every shape first, HIP events around K back-to-back launches, median and min..max of REPS,
the sides of every comparison alternated.  The lines go to stdout and to profiles/pixfmt/yuv_time.txt (or argv[3]).
  1  agmv_hip_yuv_to_xrgb_dev / _from_xrgb_dev / _histogram_dev / _similarity_dev for both layouts, beside the planar RGB8
     kernels (the nearest yardstick: the same contiguous loads, more bytes) and the packed reductions: time, algorithmic bytes
     over time (5.5 B/px for the conversions, 1.5 B/px for the reductions), share of the 8 TB/s HBM peak
  2  the comparator: NV12 -> packed XRGB32 as a torch expression on the same uint8 [T, H * 3 / 2, W] tensor (chroma terms at
     quarter resolution, broadcast over the 2 x 2 blocks, in-place clamps); both routes must give the same pixels
  3  end to end: AGMV_EncodeFramesFmtDev(NV12) against that expression + AGMV_EncodeFramesDev, same clip, same file, host LZ
     pool; wall time and the peak extra device memory of each route
usage: yuv_time.py [T=256] [reps=5] [out=profiles/pixfmt/yuv_time.txt]"""
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
OUT = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.join(R, "profiles", "pixfmt", "yuv_time.txt")
K = 10
W, Hh = 1920, 1080
NPX = W * Hh
HBM_PEAK = 8e12
LOG = []


def say(s):
    print(s, flush=True)
    LOG.append(s)


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
    say(s)


def torch_nv12_to_packed(t):
    """BT.601 limited range, the arithmetic of include/agmv.h: uint8 [T, H * 3 / 2, W] -> int32 [T, H, W]"""
    n = t.shape[0]
    c = t[:, :Hh].to(torch.int32).sub_(16).mul_(298).view(n, Hh // 2, 2, W // 2, 2)
    uv = t[:, Hh:].view(n, Hh // 2, W // 2, 2).to(torch.int32).sub_(128)
    d, e = uv[..., 0], uv[..., 1]

    def channel(term):                                        # term at chroma resolution, rounding included
        return c.add(term[:, :, None, :, None]).bitwise_right_shift_(8).clamp_(0, 255)

    out = channel(e * 409 + 128).bitwise_left_shift_(16)
    out.bitwise_or_(channel(128 - d * 100 - e * 208).bitwise_left_shift_(8))
    out.bitwise_or_(channel(d * 516 + 128))
    return out.view(n, Hh, W)


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
    say("clip: %d x %dx%d agmv_synth_v1, K = %d launches per timing, %d repetitions, the sides of a comparison alternated" % (T, W, Hh, K, REPS))

    say("-- 1: the kernels (BT.601 limited range; the matrix is kernel data, not code)")
    clips = {name: hip.yuv_from_xrgb_dev(name, packed, W, Hh) for name in ("nv12", "i420")}
    planar = hip.pixels_from_xrgb_dev("rgb8p", packed)
    out = torch.empty_like(packed)
    sides = [("rgb8p -> xrgb32 (k_pix_to_xrgb)", lambda: hip.pixels_to_xrgb_dev("rgb8p", planar, NPX, T, out=out)),
             ("xrgb32 -> rgb8p (k_pix_from_xrgb)", lambda: hip.pixels_from_xrgb_dev("rgb8p", packed, out=planar))]
    moved = {sides[0][0]: T * NPX * 7, sides[1][0]: T * NPX * 7}
    for name, c in clips.items():
        sides.append(("%s -> xrgb32 (k_yuv_to_xrgb)" % name, lambda name=name, c=c: hip.yuv_to_xrgb_dev(name, c, W, Hh, T, out=out)))
        sides.append(("xrgb32 -> %s (k_yuv_from_xrgb)" % name, lambda name=name, c=c: hip.yuv_from_xrgb_dev(name, packed, W, Hh, out=c)))
        moved[sides[-1][0]] = moved[sides[-2][0]] = T * NPX * 11 // 2          # 4 + 1.5 bytes per pixel
    res = alternate(sides)
    for name, _ in sides:
        line(name, res[name], moved[name])
    conv = {name: hip.yuv_to_xrgb_dev(name, c, W, Hh, T) for name, c in clips.items()}       # the XRGB32 clip a YUV clip stands for
    assert torch.equal(conv["nv12"], conv["i420"])
    hist = torch.zeros(1 << 19, dtype=torch.int32, device="cuda")
    counts = torch.empty(T - 1, dtype=torch.int32, device="cuda")
    sides = [("xrgb32 histogram (k_histogram)", lambda: hip.histogram_dev(packed, 3, hist)),
             ("xrgb32 similarity (k_similarity)", lambda: hip.similarity_dev(packed, counts)),
             ("rgb8p histogram (k_histogram_fmt)", lambda: hip.histogram_fmt_dev("rgb8p", planar, NPX, T, NPX, 3, hist)),
             ("rgb8p similarity (k_similarity_fmt)", lambda: hip.similarity_fmt_dev("rgb8p", planar, T, NPX, counts))]
    moved = {sides[0][0]: T * NPX * 4, sides[1][0]: T * NPX * 4, sides[2][0]: T * NPX * 3, sides[3][0]: T * NPX * 3}
    for name, c in clips.items():
        sides.append(("%s histogram (k_yuv_histogram)" % name, lambda name=name, c=c: hip.yuv_histogram_dev(name, c, W, Hh, T, NPX, 3, hist)))
        sides.append(("%s similarity (k_yuv_similarity)" % name, lambda name=name, c=c: hip.yuv_similarity_dev(name, c, W, Hh, T, counts)))
        moved[sides[-1][0]] = moved[sides[-2][0]] = T * NPX * 3 // 2
    res = alternate(sides)
    for name, _ in sides:
        line(name, res[name], moved[name])
    ref_h, ref_c = hip.histogram_dev(conv["nv12"], 3), hip.similarity_dev(conv["nv12"]).clone()
    for name, c in clips.items():
        assert torch.equal(hip.yuv_histogram_dev(name, c, W, Hh, T, NPX, 3), ref_h) and torch.equal(hip.yuv_similarity_dev(name, c, W, Hh, T), ref_c), name
    say("both layouts: the histogram and the counts of the packed kernels on the converted clip")
    del conv, planar

    say("-- 2: NV12 -> XRGB32 against the torch expression on the same uint8 [T, H * 3 / 2, W] tensor")
    nv12 = clips["nv12"].view(T, Hh * 3 // 2, W)
    assert torch.equal(torch_nv12_to_packed(nv12).view(T, NPX), hip.yuv_to_xrgb_dev("nv12", nv12, W, Hh, T))
    res = alternate([("k_yuv_to_xrgb nv12", lambda: hip.yuv_to_xrgb_dev("nv12", nv12, W, Hh, T, out=out)),
                     ("torch: chroma terms broadcast, clamp, shift, or", lambda: torch_nv12_to_packed(nv12))])
    for name, ts in res.items():
        line(name, ts, T * NPX * 11 // 2 if name.startswith("k_") else None)
    k, t = res["k_yuv_to_xrgb nv12"], res["torch: chroma terms broadcast, clamp, shift, or"]
    say("NV12 -> XRGB32: kernel %.3f .. %.3f ms, torch %.3f .. %.3f ms: the kernel's range lies %s torch's" %
        (min(k), max(k), min(t), max(t), "entirely below" if max(k) < min(t) else "NOT entirely below"))

    say("-- 3: end to end, %d x %dx%d, OPT_III, LOW quality, LZSS on the host pool, AGMV_SCHEDULE_FULL" % (T, W, Hh))
    nv12 = nv12.clone()
    del clips, out, packed, hist, counts
    shas = {}

    def route_fmt(path):
        seq.encode_frames(path, nv12, opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL, fmt="nv12")

    def route_torch(path):
        seq.encode_frames(path, torch_nv12_to_packed(nv12), opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL)

    routes = (("AGMV_EncodeFramesFmtDev(NV12)", route_fmt), ("torch conversion + AGMV_EncodeFramesDev", route_torch))
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        times = {name: [] for name, _ in routes}
        extra = {k: 0 for k in times}
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
                shas.setdefault(name, set()).add(hashlib.sha256(open("out.agmv", "rb").read()).hexdigest())
        os.chdir(R)
    for name, ts in times.items():
        ms = float(np.median(ts))
        say("%-40s wall, median of %d = %8.1f ms (min %.1f .. max %.1f) = %.1f frames/s; peak extra device memory %.2f GB" %
            (name, len(ts), ms, min(ts), max(ts), T / (ms * 1e-3), extra[name] / 1e9))
    a, b = times[routes[0][0]], times[routes[1][0]]
    say("end to end: the ranges %s" % ("overlap" if max(a) >= min(b) and max(b) >= min(a) else "do not overlap"))
    all_shas = set().union(*shas.values())
    say("both routes wrote the same file every time: %s (sha256 %s...)" % (len(all_shas) == 1, sorted(all_shas)[0][:16]))
    assert len(all_shas) == 1
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
