"""Time the deblocking of a decoded clip (agmv_hip_deblock_frames_async, k_deblock; include/agmv.h holds the rule) beside the copy
that moves the same bytes with no arithmetic (agmv_hip_view_frames_async of whole frames at stride 1, k_view), in one process.
 1. 256 x 1920x1080 and 8192 x 320x240: agmv_synth_v1 with every 4x4 block replaced by its mean (flat FILL blocks, what the filter
    is for), source and destination apart; strengths 4 and 16.  Warm-up first, then
    HIP events around 10 launches, median and min..max of REPS, the sides alternated.  Bytes moved: every frame read once and
    written once.
 2. decode_frames of a 256-frame 1080p file (agmv_synth_v1, every frame coded) into XRGB32 and into NV12 at 1920x1080, without
    and with deblock=16: wall time of the call, median and min..max of REPS, the sides alternated.
usage: deblock_time.py [reps=5] [out=profiles/deblock/deblock_time.txt]"""
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

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(R, "profiles", "deblock", "deblock_time.txt")
LAUNCHES = 10
HBM_PEAK = 8.0e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def flat_blocks(clip, n, h, w):
    """every 4x4 block of an int32 [n, h, w] clip replaced by its channel means: what FILL blocks decode to"""
    out = torch.empty_like(clip)
    for k in range(0, n, 16):                                 # a few frames at a time: the int64 temporaries stay small
        c = clip[k:k + 16].to(torch.int64)
        m = 0
        for sh in (16, 8, 0):
            v = ((c >> sh) & 255).reshape(-1, h // 4, 4, w // 4, 4).sum(dim=(2, 4)) // 16
            m = m | (v << sh)
        out[k:k + 16] = m.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2).to(torch.int32)
    return out


def kernel_times(hip, w, h, n):
    src = flat_blocks(hip.synth_dev(w, h, 1, n).reshape(n, h, w), n, h, w).reshape(-1)
    dst = torch.empty_like(src)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    sides = [("k_view, whole frames at stride 1", lambda: hip.view_frames_async(src, w, h, 0, 1, n, 0, 0, w, h, out=dst))]
    sides += [("k_deblock, strength %d" % s, (lambda s: lambda: hip.deblock_frames(src, w, h, s, dst, counts))(s)) for s in (4, 16)]
    lines = {}
    for k, fn in sides:                                       # warm-up, and the counters of each strength
        counts.zero_()
        fn()
        torch.cuda.synchronize()
        lines[k] = counts.tolist()
    hip.check()
    ts = {k: [] for k, _ in sides}
    for _ in range(REPS):
        for k, fn in sides:
            ts[k].append(events(fn))
    copy = float(np.median(ts[sides[0][0]]))
    moved = 2 * n * w * h * 4
    examined = n * ((w // 4 - 1) * h + (h // 4 - 1) * w)
    for k, _ in sides:
        ms = float(np.median(ts[k]))
        line = "%5d x %dx%d  %-34s median of %d = %8.3f ms (min %.3f .. max %.3f); %.3f GB moved = %.2f TB/s = %2.0f %% of the 8 TB/s HBM peak" % (
            n, w, h, k, REPS, ms, min(ts[k]), max(ts[k]), moved / 1e9, moved / ms / 1e9, 100.0 * moved / (ms * 1e-3) / HBM_PEAK)
        if k != sides[0][0]:
            line += "; %.3f x the copy; %d weak + %d strong of %d lines" % (ms / copy, lines[k][0], lines[k][1], examined)
        say(line)
    hip.check()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return time.perf_counter() - t0


def end_to_end(hip):
    w, h, n = 1920, 1080, 256
    say("")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "clip.agmv")
        libagmv_amd.encode_frames(path, hip.synth_dev(w, h, 1, n).reshape(n, h, w), schedule=libagmv_amd.SCHEDULE_FULL)
        say("decode_frames of a %d-frame %dx%d file (agmv_synth_v1, every frame coded, %.1f MB): wall time of the call" % (n, w, h, os.path.getsize(path) / 1e6))
        for fmt in ("xrgb32", "nv12"):
            sides = [("plain", None), ("deblock=16", 16)]
            for _, s in sides:                                # warm-up
                wall(lambda: libagmv_amd.decode_frames(path, fmt=fmt, deblock=s))
            ts = {k: [] for k, _ in sides}
            for _ in range(REPS):
                for k, s in sides:
                    ts[k].append(wall(lambda: libagmv_amd.decode_frames(path, fmt=fmt, deblock=s)))
            st = libagmv_amd.deblock_stats()
            base = float(np.median(ts["plain"]))
            for k, _ in sides:
                t = float(np.median(ts[k]))
                say("%-7s %-11s median of %d = %7.3f s (min %.3f .. max %.3f)%s" % (
                    fmt, k, REPS, t, min(ts[k]), max(ts[k]), "" if k == "plain" else "; %.3f x plain; %d weak + %d strong of %d lines" % (t / base, st["weak"], st["strong"], st["lines"])))


def main():
    hip = AgmvHip(0)
    say("%s; source and destination apart; HIP events around %d launches" % (torch.cuda.get_device_name(0), LAUNCHES))
    kernel_times(hip, 1920, 1080, 256)
    torch.cuda.empty_cache()
    kernel_times(hip, 320, 240, 8192)
    torch.cuda.empty_cache()
    end_to_end(hip)
    hip.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
