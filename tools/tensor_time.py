"""Time the normalised float tensor paths (agmv_hip_tensor_from_xrgb_async, agmv_hip_tensor_to_xrgb_async; AGMV_TENSORFMT of
include/agmv.h) on T x 320x240 agmv_synth_v1 frames resident on the GPU, each against the detour a caller had to take without them,
in one process: warm-up first, HIP events around K back-to-back launches, median and min..max of REPS, the two sides of every
comparison alternated (the method of tools/upscale_time.py).
  1  the decoder's sink, bilinear, ImageNet normalisation: 320x240 -> 224x224 F16 and 320x240 -> 1920x1080 F32, one launch, against
     agmv_hip_scale_frames_async into RGB8P followed by torch's x.float().div(255).sub(mean).div(std).to(dtype).  The bytes written
     over the time as a share of the 6.0 TB/s that plain stores reach on the MI355X, and the detour's peak extra device memory
  2  the encoder's source on T x 320x240 F16 and F32: one launch into XRGB32, against torch's
     x.float().mul(std).add(mean).mul(255).clamp(0, 255).round().to(uint8) into the RGB8P clip the encoder would then take
The detours' values are torch's floats, not the library's rules, and are not compared; the kernels' results are checked against
each other (the tensor read back is the scaled clip).
usage: tensor_time.py [T=256] [reps=5]"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip
from libagmv_amd.hip import tensor_table

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 10
SW, SH = 320, 240
STORE_RATE = 6.0e12                              # plain stores, MI355X
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = {"f16": torch.float16, "f32": torch.float32}
SINKS = [("f16", 224, 224), ("f32", 1920, 1080)]


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
    s = "%-58s median of %d = %8.3f ms (min %.3f .. max %.3f)" % (name, len(ts), ms, min(ts), max(ts))
    if nbytes:
        s += "; %.2f GB written = %.2f TB/s = %.0f %% of the 6.0 TB/s of plain stores" % (nbytes / 1e9, nbytes / ms / 1e9, 100 * nbytes / (ms * 1e-3) / STORE_RATE)
    print(s, flush=True)
    return ms


def compare(what, detour, kernel, nbytes):
    """both sides alternated; the claim is that the kernel's median lies below the detour's fastest repetition"""
    detour()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    name_t, name_k = what + ": torch detour", what + ": one launch"
    res = alternate([(name_t, detour), (name_k, kernel)])
    t, k = line(name_t, res[name_t]), line(name_k, res[name_k], nbytes)
    print("%s: detour / kernel = %.1f (medians); kernel median %s the detour's fastest repetition (%.3f ms); the detour's peak extra device memory %.2f GB, "
          "the kernel's none beyond its %.2f GB result" % (what, t / k, "BELOW" if k < min(res[name_t]) else "NOT below", min(res[name_t]),
                                                           (torch.cuda.max_memory_allocated() - base) / 1e9, nbytes / 1e9), flush=True)


def main():
    hip = AgmvHip(0)
    packed = hip.synth_dev(SW, SH, 1, T).reshape(-1)
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    print("clip: %d x %dx%d agmv_synth_v1, ImageNet normalisation, K = %d launches per timing, %d repetitions, the sides of a comparison alternated"
          % (T, SW, SH, K, REPS), flush=True)
    print("-- 1: the sink: agmv_hip_tensor_from_xrgb_async (bilinear) against agmv_hip_scale_frames_async into RGB8P + the torch expression", flush=True)
    for name, dw, dh in SINKS:
        dtype, es = DTYPES[name], 2 if name == "f16" else 4
        table = torch.from_numpy(tensor_table(name, MEAN, STD).view(np.int16 if es == 2 else np.int32)).cuda()
        out = torch.empty((T, 3, dh, dw), dtype=dtype, device="cuda")
        planes = torch.empty((T, 3, dh, dw), dtype=torch.uint8, device="cuda")

        def detour():
            hip.scale_frames_async(3, packed, SW, SH, T, "rgb8p", dw, dh, out=planes)
            return planes.float().div(255).sub(mean).div(std).to(dtype)

        def kernel():
            return hip.tensor_from_xrgb_async(name, packed, SW, SH, T, table, out, 3, dw, dh)
        compare("sink %s %dx%d -> %dx%d" % (name, SW, SH, dw, dh), detour, kernel, T * 3 * dw * dh * es)
        # the tensor read back by the source kernel is the scaled clip
        a = (255.0 * np.asarray(STD, np.float32).astype(np.float64)).astype(np.float32).tolist()
        b = (255.0 * np.asarray(MEAN, np.float32).astype(np.float64)).astype(np.float32).tolist()
        back = hip.tensor_to_xrgb_async(name, kernel(), dw * dh, T, a + b)
        ref = hip.scale_frames_async(3, packed, SW, SH, T, "xrgb32", dw, dh).view(torch.int32).reshape(T, dw * dh)
        assert torch.equal(back, ref)
        del out, planes, back, ref
        torch.cuda.empty_cache()

    print("-- 2: the source: agmv_hip_tensor_to_xrgb_async against the torch expression into RGB8P", flush=True)
    for name in ("f16", "f32"):
        dtype = DTYPES[name]
        table = torch.from_numpy(tensor_table(name, MEAN, STD).view(np.int16 if name == "f16" else np.int32)).cuda()
        x = torch.empty((T, 3, SH, SW), dtype=dtype, device="cuda")
        hip.tensor_from_xrgb_async(name, packed, SW, SH, T, table, x)
        clip = torch.empty((T, SH * SW), dtype=torch.int32, device="cuda")

        def detour():
            return x.float().mul(std).add(mean).mul(255).clamp(0, 255).round().to(torch.uint8)

        def kernel():
            return hip.tensor_to_xrgb_async(name, x, SH * SW, T, a + b, out=clip)
        compare("source %s %dx%d" % (name, SW, SH), detour, kernel, T * SH * SW * 4)
        assert torch.equal(kernel(), packed.reshape(T, SH * SW) & 0xFFFFFF)


if __name__ == "__main__":
    main()
