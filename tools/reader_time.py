"""Time a reader session (libagmv_amd.Reader: include/agmv_reader.h) against the way without one, on the T-frame 1920x1080 file of
agmv_synth_v1 frames of tools/view_time.py, in one process, warm-up first, median and min..max of REPS, the sides alternated (the
method of tools/view_time.py):
  1  the file walked in 16 chunks of 16 frames, a 224 x 224 window of each as F16 with the ImageNet normalisation: 16 reads of one
     Reader (its open and close inside the time) against 16 calls decode_frames(frames=, crop=), the loop of views.  Both give the
     same bits, which is checked
  2  one backward seek to frame 120 and a read of 16 frames, behind a full pass: with the seek index (the default budget) and with a
     budget of one buffer, which leaves checkpoint 0 alone; against the one view decode_frames(frames=range(120, 136), crop=)
usage: reader_time.py [T=256] [reps=5]"""
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
W, H = 1920, 1080
N, SEEK, Y0, X0, WIN = 16, 120, 428, 848, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KW = dict(fmt="f16", mean=MEAN, std=STD, crop=(Y0, X0, WIN, WIN))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def report(name, ts):
    print("%-22s wall median of %d = %8.3f s (min %.3f .. max %.3f)" % (name, len(ts), float(np.median(ts)), min(ts), max(ts)), flush=True)
    return float(np.median(ts))


def main():
    hip = AgmvHip(0)
    path = os.path.join(tempfile.mkdtemp(), "clip.agmv")
    clip = hip.synth_dev(W, H, 1, T).reshape(T, H, W)
    libagmv_amd.encode_frames(path, clip, schedule=libagmv_amd.SCHEDULE_FULL)
    del clip
    print("file: %d x %dx%d agmv_synth_v1, %.1f MB; %d repetitions, the sides alternated" % (T, W, H, os.path.getsize(path) / 1e6, REPS), flush=True)

    def by_reader():
        with libagmv_amd.Reader(path, **KW) as r:
            return list(r.batches(N)), r.stats()

    def by_views():
        return [libagmv_amd.decode_frames(path, frames=range(p, p + N), **KW)[0] for p in range(0, T, N)]

    print("-- 1: %d chunks of %d frames, window %d x %d at (%d, %d), F16: one Reader against the loop of views" % (T // N, N, WIN, WIN, X0, Y0), flush=True)
    (a, st), b = by_reader(), by_views()
    assert len(a) == len(b) == T // N and all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
    print("reader: %s" % st, flush=True)
    del a, b
    res = {"reader": [], "views": []}
    for _ in range(REPS):
        for name, fn in (("reader", by_reader), ("views", by_views)):
            s, out = wall(fn)
            del out
            res[name].append(s)
    reader, views = report("reader, 16 reads", res["reader"]), report("16 views", res["views"])
    print("views / reader = %.2f in wall time (medians); per chunk %.4f s against %.4f s" % (views / reader, reader / (T // N), views / (T // N)), flush=True)

    print("-- 2: behind a full pass, seek(%d) and a read of %d frames; and the one view of those frames" % (SEEK, N), flush=True)
    lz_cap = W * H * 33 // 16 + 4096
    want = libagmv_amd.decode_frames(path, frames=range(SEEK, SEEK + N), **KW)[0]
    res = {}
    readers = {"indexed": libagmv_amd.Reader(path, **KW), "index of one buffer": libagmv_amd.Reader(path, index_bytes=lz_cap, **KW)}
    for name, r in readers.items():
        for _ in r.batches(64):
            pass
        print("%s: behind the pass %s" % (name, r.stats()), flush=True)

    def seek_read(r):
        r.seek(SEEK)
        return r.read(N)
    for _ in range(REPS):
        for name, r in readers.items():
            before = r.stats()["lz_frames"]
            s, out = wall(lambda: seek_read(r))
            assert torch.equal(out.view(torch.int16), want.view(torch.int16))
            res.setdefault(name, []).append(s)
            res.setdefault(name + " lz", []).append(r.stats()["lz_frames"] - before)
            r.seek(T)                                                # (so that the next seek to 120 is a seek)
        s, out = wall(lambda: libagmv_amd.decode_frames(path, frames=range(SEEK, SEEK + N), **KW)[0])
        res.setdefault("one view", []).append(s)
    for name in readers:
        report("seek + read, " + name, res[name])
        print("    frames through the LZ stage per seek + read: %s" % sorted(set(res[name + " lz"])), flush=True)
    report("one view", res["one view"])
    for r in readers.values():
        r.close()


if __name__ == "__main__":
    main()
