"""Time the pattern dithering (agmv_hip_dither_frames_async, k_dither; include/agmv.h holds the definition) beside the encode of the
same frames (agmv_hip_encode_frames_dev, k_encode), in one process: 256 x 1920x1080 agmv_synth_v1 and 32 x 1920x1080 noise, both
against the HIGH_QUALITY OPT_III palette of the synthetic clip (the bench's), strengths 16, 32 and 64.  The dither works in place
and a dithered clip is a fixed point, so every timed call starts from a fresh copy of the clip; the copy lies outside the events.
Warm-up first, then HIP events around one call, median and min..max of REPS, the sides alternated.
usage: dither_time.py [reps=5] [out=profiles/dither/dither_time.txt]"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import hostlib as H
from libagmv_amd import AgmvHip

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(R, "profiles", "dither", "dither_time.txt")
W, Hh = 1920, 1080
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, before):
    before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(hip, name, clip, n):
    work = torch.empty_like(clip)
    out = torch.empty((n, hip.max_usize(W, Hh)), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int32, device="cuda")
    fresh = lambda: work.copy_(clip)
    sides = [("k_encode (agmv_hip_encode_frames_dev)", lambda: hip.encode_dev(work, n, W, Hh, out=out, sizes=sizes))]
    sides += [("k_dither, strength %d" % s, (lambda s: lambda: hip.dither_frames(work.reshape(-1), W, Hh, s))(s)) for s in (16, 32, 64)]
    for _, fn in sides:                                       # warm-up of every shape
        fresh()
        fn()
    torch.cuda.synchronize()
    hip.check()
    ts = {k: [] for k, _ in sides}
    for _ in range(REPS):
        for k, fn in sides:
            ts[k].append(timed(fn, fresh))
    enc = float(np.median(ts[sides[0][0]]))
    for k, _ in sides:
        ms = float(np.median(ts[k]))
        say("%-12s %-40s median of %d = %8.3f ms (min %.3f .. max %.3f) = %6.2f Gpx/s%s"
            % (name, k, REPS, ms, min(ts[k]), max(ts[k]), n * W * Hh / ms / 1e6, "" if k == sides[0][0] else "; %.1f x k_encode" % (ms / enc)))
    hip.check()


def main():
    hip = AgmvHip(0)
    synth = hip.synth_dev(W, Hh, 0, 256)
    hist = hip.histogram_dev(synth.reshape(-1), 1)
    torch.cuda.synchronize()
    p0, p1 = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    H.lib().AGMV_BuildPalette(hist.cpu().numpy().view(np.uint32), 1, 3, p0, p1)
    hip.set_palette(p0.astype(np.uint32), p1.astype(np.uint32), True)
    say("%s; 1920x1080, 512 colours, in place, every timed call on a fresh copy of the clip; HIP events around one call" % torch.cuda.get_device_name(0))
    measure(hip, "synth x 256", synth, 256)
    del synth
    noise = torch.randint(0, 1 << 24, (32, Hh, W), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    measure(hip, "noise x 32", noise, 32)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
