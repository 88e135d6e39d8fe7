"""Time the palette build with the refinement ("palette refinement" of include/agmv.h) over two histograms at HIGH quality: the
212 frames of the foxlogo clip (tests/golden/foxlogo212.npz, 320 x 240) and T frames of 1920 x 1080 agmv_synth_v1.  Per histogram
and palette size (512 colours with 511 free, 256 colours):
  1  the pick alone: AGMV_BuildPalette on the host (wall time)
  2  agmv_hip_palette_refine_dev, 16 rounds from that pick, on the resident histogram: HIP events around one call (its
     2 * 17 launches), median and min..max of REPS; rounds that moved a colour, distortion before and after
  3  AGMV_BuildPaletteRefined, 16 rounds: pick, upload of the histogram, refinement, download, slot map (wall time)
There is no target: the stage runs once per file.  What is printed is also written to profiles/palette/refine_time.txt (or argv[3]).
usage: palette_time.py [T=32] [reps=5] [out]"""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip, seq

T = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(R, "profiles", "palette", "refine_time.txt")
HIGH, ROUNDS = 1, 16
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def start_of(p0, p1, mode512):
    """the pick list as colours out of AGMV_BuildPalette's palettes (the inverse of its slot map), centroid 511 = 0"""
    if not mode512:
        return p0.astype(np.uint32)
    return np.concatenate([p0[:126], p1[:127], p0[127:], p1[127:], np.zeros(1, np.uint64)]).astype(np.uint32)


def main():
    hip = AgmvHip(0)
    L = seq.load_library()
    rgb = np.load(os.path.join(R, "tests", "golden", "foxlogo212.npz"))["rgb"].astype(np.uint32)
    fox = torch.from_numpy((rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]).view(np.int32)).cuda()
    clips = (("foxlogo, 212 x 320x240", fox), ("agmv_synth_v1, %d x 1920x1080" % T, hip.synth_dev(1920, 1080, 1, T)))
    say("palette build at HIGH quality, %d rounds of refinement, %d repetitions" % (ROUNDS, REPS))
    for name, clip in clips:
        d_hist = hip.histogram_dev(clip, HIGH)
        torch.cuda.synchronize()
        hist = d_hist.cpu().numpy().view(np.uint32)
        say("-- %s: %d pixels in %d occupied bins" % (name, int(hist.sum(dtype=np.uint64)), int((hist != 0).sum())))
        for opt, k, n_free in ((3, 512, 511), (2, 256, 256)):
            p0, p1 = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
            pick = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                L.AGMV_BuildPalette(hist.ctypes.data, HIGH, opt, p0.ctypes.data, p1.ctypes.data)
                pick.append(1e3 * (time.perf_counter() - t0))
            start = torch.from_numpy(start_of(p0, p1, k == 512).view(np.int32)).cuda()
            ms = []
            for rep in range(REPS + 1):                           # the first call is the warm-up
                pal = start.clone()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rounds, sse = hip.palette_refine_dev(d_hist, HIGH, pal, n_free, ROUNDS)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(e0.elapsed_time(e1))
            e = sse.cpu().numpy().view(np.uint64)
            whole = []
            assert L.AGMV_BuildPaletteRefined(hist.ctypes.data, HIGH, opt, p0.ctypes.data, p1.ctypes.data, 1, None) == 0      # warm-up: the library's context
            for _ in range(REPS):
                t0 = time.perf_counter()
                assert L.AGMV_BuildPaletteRefined(hist.ctypes.data, HIGH, opt, p0.ctypes.data, p1.ctypes.data, ROUNDS, None) == 0
                whole.append(1e3 * (time.perf_counter() - t0))
            say("%3d colours: pick on the host %.2f ms (min %.2f .. max %.2f); refinement on the GPU %.3f ms (min %.3f .. max %.3f), %d rounds moved a colour, "
                "distortion %d -> %d (x %.3f); AGMV_BuildPaletteRefined %.2f ms (min %.2f .. max %.2f)"
                % (k, np.median(pick), min(pick), max(pick), np.median(ms), min(ms), max(ms), int(rounds.item()), int(e[0]), int(e[1]),
                   int(e[1]) / max(int(e[0]), 1), np.median(whole), min(whole), max(whole)))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
