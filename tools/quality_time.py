"""Time agmv_hip_measure_frames_async (k_measure) on T x 1920x1080 frames resident on the GPU, in one process: warm-up first, HIP
events around K back-to-back launches, median and min..max of REPS, the sides of every comparison alternated.
  1  the kernel with the reference in XRGB32, RGB24 and NV12: time, algorithmic bytes T * (4 * w * h + the reference's frame
     bytes) over time, share of the 8 TB/s HBM peak
  2  the comparator: the torch expression for the plain SSE per frame and channel of the same clips (unpack both sides, subtract,
     square, sum), for the XRGB32 and the RGB24 reference -- SSE alone, without the block sums, the maximum and SSIM; both routes
     must give the same integers.  (Torch has no reading of NV12: that reference has no comparator.)
The test clip is agmv_synth_v1 with its low bits cleared, as a quantiser leaves them; the reference is the clip itself.
The lines are printed and written to profiles/quality/quality_time.txt (or the path given).
usage: quality_time.py [T=256] [reps=5] [out=profiles/quality/quality_time.txt]"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(R, "profiles", "quality", "quality_time.txt")
K = 10
W, Hh = 1920, 1080
NPX = W * Hh
HBM_PEAK = 8e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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
    say(s)


def channels(p):
    return torch.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], dim=-1)


def torch_sse(test, ref, packed_ref):
    """int64 [T, 3]: the plain squared error per frame and channel"""
    d = channels(test) - (channels(ref) if packed_ref else ref.int())
    return (d * d).sum(dim=1, dtype=torch.int64)


def main():
    hip = AgmvHip(0)
    ref = hip.synth_dev(W, Hh, 1, T).reshape(T, NPX)
    test = ref & 0xF8FCF8
    say("clips: %d x %dx%d agmv_synth_v1 (reference) and the same with the low bits cleared (test); K = %d launches per timing, %d repetitions, "
        "the sides of a comparison alternated" % (T, W, Hh, K, REPS))
    refs = {"xrgb32": ref, "rgb24": hip.pixels_from_xrgb_dev("rgb24", ref), "nv12": hip.yuv_from_xrgb_dev("nv12", ref, W, Hh)}
    out = torch.empty((T, 12), dtype=torch.int64, device="cuda")
    say("-- 1: the kernel")
    sides = [("k_measure, reference %s" % name, lambda name=name, c=c: hip.measure_frames(test, name, c, W, Hh, T, out=out)) for name, c in refs.items()]
    res = alternate(sides)
    for (name, _), c in zip(sides, refs.values()):
        line(name, res[name], T * 4 * NPX + c.numel() * c.element_size())
    say("-- 2: against the torch expression for the plain SSE of the same clips")
    rgb = refs["rgb24"].reshape(T, NPX, 3)
    for name, c, packed_ref in (("xrgb32", ref, True), ("rgb24", rgb, False)):
        got = hip.measure_frames(test, name, refs[name], W, Hh, T)[:, :3]
        assert torch.equal(got, torch_sse(test, c, packed_ref)), name
    say("both routes give the same sums for both references")
    res = alternate([("k_measure, reference xrgb32", sides[0][1]), ("torch SSE, reference xrgb32", lambda: torch_sse(test, ref, True)),
                     ("k_measure, reference rgb24", sides[1][1]), ("torch SSE, reference rgb24", lambda: torch_sse(test, rgb, False))])
    for name, ts in res.items():
        line(name, ts, T * NPX * (8 if name.endswith("xrgb32") else 7) if name.startswith("k_") else None)
    for name in ("xrgb32", "rgb24"):
        k, t = res["k_measure, reference " + name], res["torch SSE, reference " + name]
        say("reference %s: kernel (SSE, block SSE, maximum, SSIM) %.3f .. %.3f ms, torch (SSE) %.3f .. %.3f ms: the kernel's range lies %s torch's" %
            (name, min(k), max(k), min(t), max(t), "entirely below" if max(k) < min(t) else "NOT entirely below"))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
