"""Time the decoder's scaling sink (agmv_hip_scale_frames_async, AGMV_SCALE_NEAREST / AGMV_SCALE_BILINEAR of include/agmv.h) on
T x 320x240 agmv_synth_v1 frames resident on the GPU scaled to 1920x1080 (x6 by x4.5), into XRGB32, RGB24 and NV12, in one process:
warm-up first, HIP events around K back-to-back launches, median and min..max of REPS, the sides of every comparison alternated
(the method of tools/scale_time.py).
  1  k_scale_up_wide per filter and layout: time, and the bytes written over that time as a share of the 6.0 TB/s that plain stores
     reach on the MI355X (what the kernel moves: 0.3 MB in, 8.3 / 6.2 / 3.1 MB out per frame; the source stays in L2)
  2  the detour a caller takes today, bilinear only: unpack the XRGB32 clip to float planes, torch's
     interpolate(mode="bilinear", align_corners=False), round and repack into the layout.  A yardstick for time and peak extra
     device memory only: its values are torch's floats, not the library's integers, and are not compared
usage: upscale_time.py [T=256] [reps=5]"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 10
SW, SH, DW, DH = 320, 240, 1920, 1080
NPX = DW * DH
STORE_RATE = 6.0e12                              # plain stores, MI355X
FILTERS = {"nearest": 1, "bilinear": 3}
FRAME_BYTES = {"xrgb32": 4 * NPX, "rgb24": 3 * NPX, "nv12": NPX * 3 // 2}


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
        s += "; %.2f GB written = %.2f TB/s = %.0f %% of the 6.0 TB/s of plain stores" % (nbytes / 1e9, nbytes / ms / 1e9, 100 * nbytes / (ms * 1e-3) / STORE_RATE)
    print(s, flush=True)
    return ms


def torch_detour(packed, layout):
    """int32 [T, SH, SW] -> the clip at DW x DH in `layout` through float32 (torch's bilinear; not the library's integers)"""
    x = torch.stack([(packed >> 16) & 255, (packed >> 8) & 255, packed & 255], dim=1).float()
    x = torch.nn.functional.interpolate(x, size=(DH, DW), mode="bilinear", align_corners=False)
    if layout == "nv12":                                      # BT.601 limited range in float: luma per pixel, chroma of the 2 x 2 mean
        r, g, b = x[:, 0], x[:, 1], x[:, 2]
        y = (0.257 * r + 0.504 * g + 0.098 * b + 16).round_().clamp_(0, 255).to(torch.uint8)
        m = torch.nn.functional.avg_pool2d(x, 2)
        u = (-0.148 * m[:, 0] - 0.291 * m[:, 1] + 0.439 * m[:, 2] + 128).round_().clamp_(0, 255).to(torch.uint8)
        v = (0.439 * m[:, 0] - 0.368 * m[:, 1] - 0.071 * m[:, 2] + 128).round_().clamp_(0, 255).to(torch.uint8)
        return torch.cat([y.reshape(T, -1), torch.stack([u, v], dim=3).reshape(T, -1)], dim=1)
    q = x.round_().clamp_(0, 255)
    if layout == "rgb24":
        return q.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    q = q.to(torch.int32)
    return (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]


def main():
    hip = AgmvHip(0)
    packed = hip.synth_dev(SW, SH, 1, T).reshape(T, SH, SW)
    flat = packed.reshape(-1)
    print("clip: %d x %dx%d agmv_synth_v1 -> %dx%d, K = %d launches per timing, %d repetitions, the sides of a comparison alternated"
          % (T, SW, SH, DW, DH, K, REPS), flush=True)
    print("-- 1: agmv_hip_scale_frames_async (k_scale_up_wide, plain gathers of the L2-resident source), per filter and layout", flush=True)
    outs = {name: torch.empty((T, fb), dtype=torch.uint8, device="cuda") for name, fb in FRAME_BYTES.items()}
    sides = [("%s %s (k_scale_up_wide)" % (layout, f), (lambda f=f, layout=layout: hip.scale_frames_async(FILTERS[f], flat, SW, SH, T, layout, DW, DH, out=outs[layout])))
             for layout in FRAME_BYTES for f in FILTERS]
    res = alternate(sides)
    kernel_ms = {name: line(name, ts, T * FRAME_BYTES[name.split()[0]]) for name, ts in res.items()}
    # the layouts agree: the RGB24 clip read back is the XRGB32 clip
    a = hip.scale_frames_async(3, flat, SW, SH, T, "xrgb32", DW, DH, out=outs["xrgb32"]).view(torch.int32).reshape(T, NPX)
    b = hip.pixels_to_xrgb_dev("rgb24", hip.scale_frames_async(3, flat, SW, SH, T, "rgb24", DW, DH, out=outs["rgb24"]).reshape(-1), NPX, T)
    assert torch.equal(a, b)
    del a, b

    print("-- 2: the torch detour (unpack, interpolate(mode=\"bilinear\", align_corners=False), repack) beside the bilinear kernel; values not compared", flush=True)
    for layout in FRAME_BYTES:
        torch_detour(packed, layout)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        name_t, name_k = "%s torch detour via float32" % layout, "%s bilinear (k_scale_up_wide)" % layout
        res = alternate([(name_t, lambda: torch_detour(packed, layout)),
                         (name_k, lambda: hip.scale_frames_async(3, flat, SW, SH, T, layout, DW, DH, out=outs[layout]))])
        t, k = line(name_t, res[name_t]), line(name_k, res[name_k], T * FRAME_BYTES[layout])
        print("%s: torch detour / kernel = %.1f (medians); the detour's peak extra device memory %.2f GB, the kernel's none beyond its %.2f GB result"
              % (layout, t / k, (torch.cuda.max_memory_allocated() - base) / 1e9, T * FRAME_BYTES[layout] / 1e9), flush=True)
    print("kernel medians: " + ", ".join("%s %.3f ms" % (n.replace(" (k_scale_up_wide)", ""), ms) for n, ms in kernel_ms.items()), flush=True)


if __name__ == "__main__":
    main()
