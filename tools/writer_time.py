"""Time a writer session (libagmv_amd.Writer: include/agmv_writer.h) against the one-shot call, on T x 1920x1080 agmv_synth_v1 frames
resident on the GPU, AGMV_SCHEDULE_FULL, in one process: one warm-up of every side first, then REPS repetitions with the sides
alternated; wall time around each whole encode (open, palette, chunks, close) with the device synchronised on both sides; median and
min..max.
  a  encode_frames of the XRGB32 clip
  b  the same clip through a Writer: analyse, then write, in calls of 32 frames
  c  the clip as NV12 through a Writer, the same way (and, for scale, encode_frames of the NV12 clip: c1)
Peak device memory above the source clip for each: the smallest torch.cuda.mem_get_info()[0] a sampling thread sees during the call
(every 2 ms: the library allocates outside torch's allocator), taken from the free memory just before it.  b and c must write a's
and c1's bytes, which is checked.  With AGMV_TRACE=1 in the environment the library's own stage times go to stderr.
usage: writer_time.py [T=256] [reps=3]"""
import os
import sys
import tempfile
import threading
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

import libagmv_amd
from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W, H, N = 1920, 1080, 32
FULL = libagmv_amd.SCHEDULE_FULL


def measured(fn):
    """(wall seconds, peak bytes above the free memory before the call) of fn()"""
    torch.cuda.synchronize()
    free0, low, stop = torch.cuda.mem_get_info()[0], [None], threading.Event()
    low[0] = free0

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.002)
    th = threading.Thread(target=sample)
    th.start()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    stop.set()
    th.join()
    return s, free0 - low[0]


def report(name, runs):
    ts, peaks = [r[0] for r in runs], [r[1] for r in runs]
    print("%-34s wall median of %d = %7.3f s (min %.3f .. max %.3f); peak device memory above the source %7.1f MB"
          % (name, len(ts), float(np.median(ts)), min(ts), max(ts), max(peaks) / 1e6), flush=True)
    return float(np.median(ts))


def through_writer(path, clip, fmt, stats):
    with libagmv_amd.Writer(path, H, W, fmt=fmt, schedule=FULL) as w:
        for p in range(0, T, N):
            w.analyse(clip[p:p + N])
        for p in range(0, T, N):
            w.write(clip[p:p + N])
        stats.update(w.stats())


def main():
    hip = AgmvHip(0)
    d = tempfile.mkdtemp()
    paths = {k: os.path.join(d, k + ".agmv") for k in ("a", "b", "c", "c1")}
    clip = hip.synth_dev(W, H, 1, T).reshape(T, H, W)
    libagmv_amd.encode_frames(paths["a"], clip, schedule=FULL)
    nv12 = libagmv_amd.decode_frames(paths["a"], fmt="nv12")[0].contiguous()
    print("clip: %d x %dx%d agmv_synth_v1, XRGB32 %.0f MB, NV12 %.0f MB; calls of %d frames; %d repetitions, the sides alternated"
          % (T, W, H, clip.numel() * 4 / 1e6, nv12.numel() / 1e6, N, REPS), flush=True)
    stats = {"b": {}, "c": {}}
    sides = (("a  encode_frames, XRGB32", lambda: libagmv_amd.encode_frames(paths["a"], clip, schedule=FULL)),
             ("b  Writer, XRGB32", lambda: through_writer(paths["b"], clip, "xrgb32", stats["b"])),
             ("c1 encode_frames, NV12", lambda: libagmv_amd.encode_frames(paths["c1"], nv12, fmt="nv12", schedule=FULL)),
             ("c  Writer, NV12", lambda: through_writer(paths["c"], nv12, "nv12", stats["c"])))
    for _, fn in sides:                                           # warm-up
        fn()
    for x, y in (("a", "b"), ("c1", "c")):
        assert open(paths[x], "rb").read() == open(paths[y], "rb").read(), "the writer's file differs from the one-shot call's (%s, %s)" % (x, y)
    print("files: b == a and c == c1, byte for byte; a is %.1f MB; writer b %s; writer c %s" % (os.path.getsize(paths["a"]) / 1e6, stats["b"], stats["c"]), flush=True)
    runs = {name: [] for name, _ in sides}
    for _ in range(REPS):
        for name, fn in sides:
            runs[name].append(measured(fn))
    med = {name[:2].strip(): report(name, runs[name]) for name, _ in sides}
    spread = (max(r[0] for r in runs[sides[0][0]]) - min(r[0] for r in runs[sides[0][0]])) / med["a"]
    print("b / a = %.3f, c / c1 = %.3f in wall time (medians); the run-to-run spread of a is %.1f %% of its median" % (med["b"] / med["a"], med["c"] / med["c1"], 100 * spread),
          flush=True)


if __name__ == "__main__":
    main()
