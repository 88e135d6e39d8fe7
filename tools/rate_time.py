"""Time the encoder's change of frame rate (encode_frames(rate=, time=): AGMV_EncodeViewRateDev of include/agmv.h) on one MI355X, in one
process.  HIP events around K launches (or K runs of an expression), the median and min..max of REPS timings behind one warm-up, on
T resident 1920 x 1080 frames in NV12 and in RGB24, for the full frame and for the centred 1440 x 1080 window:
  1  k_time alone (agmv_hip_time_frames_async) at 4 : 1 and 5 : 2 AREA and 4 : 1 NEAREST.  Traffic = the bytes of the taps read in the
     source's layout (one window per tap with a weight above 0) + the bytes written, over the time, beside the 8 TB/s HBM peak
  2  k_view_src (agmv_hip_view_source_async) on every 4th frame of the same selection: it reads a quarter of the frames and writes
     the same clip as 4 : 1, so it is a floor for the write side, nothing more
  3  the torch expression 4 : 1 AREA replaces: the frames sliced into groups of four, the window cut, float mean over each group,
     rounded half up and repacked to 0x00RRGGBB; for NV12 behind the conversion to XRGB32 the caller would need first
     (yuv_to_xrgb_dev of the frames that are used).  Its result is checked against k_time's, and the peak of
     torch.cuda.max_memory_allocated above the source goes next to the time
usage: rate_time.py [T=1024] [reps=5]"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K, K_TORCH = 10, 2
W, H = 1920, 1080
WINDOWS = {"full frame": (0, 0, W, H), "1440 x 1080 window": (240, 0, 1440, 1080)}
RATES = [((4, 1), "area"), ((5, 2), "area"), ((4, 1), "nearest")]
HBM = 8.0e12
# name -> (bytes per pixel read, shape of t frames)
LAYOUTS = {"nv12": (1.5, lambda t: (t, H * 3 // 2, W)), "rgb24": (3, lambda t: (t, H, W, 3))}


def events(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def timed(fn, k=K):
    fn()
    torch.cuda.synchronize()
    ts = [events(fn, k) for _ in range(REPS)]
    return float(np.median(ts)), min(ts), max(ts)


def peak_above(fn):
    """the peak of torch's allocations over one run of fn above what is allocated before it, and fn's result"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def taps(nv, rate, time):
    """the frames read: one per tap with a weight above 0, summed over the output frames"""
    sn, dn = rate
    m = nv * dn // sn
    return m if time == "nearest" else sum(((j + 1) * sn - 1) // dn - j * sn // dn + 1 for j in range(m))


def source(hip, name, t):
    """t frames of agmv_synth_v1 at 1920 x 1080 in the layout, made 64 frames at a time"""
    out = torch.empty(LAYOUTS[name][1](t), dtype=torch.uint8, device="cuda")
    for f0 in range(0, t, 64):
        n = min(64, t - f0)
        x = hip.synth_dev(W, H, 1 + f0, n).reshape(n, W * H)
        if name == "nv12":
            hip.yuv_from_xrgb_dev("nv12", x, W, H, out=out[f0:f0 + n].reshape(n, -1))
        else:
            hip.pixels_from_xrgb_dev("rgb24", x, out=out[f0:f0 + n].reshape(n, -1))
    torch.cuda.synchronize()
    return out


def group_mean(hip, name, src, m, win):
    """what 4 : 1 AREA replaces, in torch: int32 [m, wh, ww]"""
    x0, y0, ww, wh = win
    if name == "nv12":
        x = hip.yuv_to_xrgb_dev("nv12", src[:4 * m].reshape(4 * m, -1), W, H, 4 * m).view(m, 4, H, W)[:, :, y0:y0 + wh, x0:x0 + ww]
        ch = torch.stack(((x >> 16) & 255, (x >> 8) & 255, x & 255), dim=-1)
    else:
        ch = src[:4 * m].view(m, 4, H, W, 3)[:, :, y0:y0 + wh, x0:x0 + ww]
    q = torch.floor(ch.float().mean(dim=1) + 0.5).to(torch.int32)
    return q[..., 0] << 16 | q[..., 1] << 8 | q[..., 2]


def main():
    hip = AgmvHip(0)
    print("%d resident frames of %d x %d; K = %d launches per timing (torch: %d runs), median of %d" % (T, W, H, K, K_TORCH, REPS), flush=True)
    for name, (bpp, _) in LAYOUTS.items():
        src = source(hip, name, T)
        for label, win in WINDOWS.items():
            x0, y0, ww, wh = win
            print("-- %s, %s" % (name, label), flush=True)
            kept = None
            for rate, time in RATES:
                m = T * rate[1] // rate[0]
                out = torch.empty((m, wh, ww), dtype=torch.int32, device="cuda")
                ms, lo, hi = timed(lambda: hip.time_frames(name, src, W, H, T, 0, 1, T, x0, y0, ww, wh, rate, time=time, out=out))
                moved = (bpp * taps(T, rate, time) + 4 * m) * ww * wh
                print("k_time %d:%d %-7s %4d frames out: median of %d = %8.4f ms (min %.4f .. max %.4f); %.3f GB read + written = %.2f TB/s = %.0f %% of the 8 TB/s HBM peak"
                      % (rate[0], rate[1], time, m, REPS, ms, lo, hi, moved / 1e9, moved / ms / 1e9, 100 * moved / (ms * 1e-3) / HBM), flush=True)
                if (rate, time) == ((4, 1), "area"):
                    kept = out
                else:
                    del out
            m = T // 4
            out = torch.empty((m, wh, ww), dtype=torch.int32, device="cuda")
            ms, lo, hi = timed(lambda: hip.view_source(name, src, W, H, 0, 4, m, x0, y0, ww, wh, out=out))
            moved = (bpp + 4) * m * ww * wh
            print("k_view_src every 4th  %4d frames out: median of %d = %8.4f ms (min %.4f .. max %.4f); %.3f GB read + written = %.2f TB/s (a quarter of the reads: a floor)"
                  % (m, REPS, ms, lo, hi, moved / 1e9, moved / ms / 1e9), flush=True)
            del out
            peak, ref = peak_above(lambda: group_mean(hip, name, src, m, win))
            same = torch.equal(ref, kept)
            del ref
            ms, lo, hi = timed(lambda: group_mean(hip, name, src, m, win), K_TORCH)
            print("torch  4:1 group mean %4d frames out: median of %d = %8.3f ms (min %.3f .. max %.3f); peak allocated above the source %.3f GB; result %s k_time's"
                  % (m, REPS, ms, lo, hi, peak / 1e9, "equals" if same else "DIFFERS FROM"), flush=True)
            del kept
            torch.cuda.empty_cache()
        del src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
