"""Time agmv_hip_similarity_dev (k_similarity: the equal-grey count of every adjacent pair of a clip) over T x 1920x1080
agmv_synth_v1 frames resident on the GPU: HIP events, median of REPS after a warm-up, and the algorithmic bytes (T * npx * 4: each
frame is read once) over that time as a share of the 8 TB/s HBM peak.  Beside it the host library's AGMV_CompareFrameSimilarity
over the same T - 1 pairs on one core, and the check that both give the same counts.
usage: similarity_time.py [T=256] [reps=7]"""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import hostlib as H
from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W, Hh = 1920, 1080
HBM_PEAK = 8e12


def main():
    hip = AgmvHip(0)
    frames = hip.synth_dev(W, Hh, 1, T)
    counts = hip.similarity_dev(frames)                           # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.similarity_dev(frames, counts)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    nbytes = T * W * Hh * 4
    print("k_similarity %d x %dx%d (memset of the counts + kernel, HIP events): median of %d = %.3f ms (min %.3f, max %.3f); "
          "%.2f GB read once = %.2f TB/s = %.0f %% of the 8 TB/s HBM peak" % (T, W, Hh, REPS, ms, min(ts), max(ts), nbytes / 1e9,
                                                                          nbytes / ms / 1e9, 100 * nbytes / (ms * 1e-3) / HBM_PEAK), flush=True)
    L = H.lib()
    gpu = counts.cpu().numpy().view(np.uint32)
    prev = frames[0].cpu().numpy().view(np.uint32).reshape(-1).astype(np.uint64)
    host_s, same = 0.0, True
    for f in range(1, T):
        cur = frames[f].cpu().numpy().view(np.uint32).reshape(-1).astype(np.uint64)
        t0 = time.perf_counter()
        ratio = L.AGMV_CompareFrameSimilarity(prev, cur, W, Hh)
        host_s += time.perf_counter() - t0
        same = same and int(np.rint(float(ratio) * W * Hh)) == int(gpu[f - 1])
        prev = cur
    print("host AGMV_CompareFrameSimilarity, the same %d pairs on one core: %.3f s = %.2f ms per pair; counts equal to the GPU's: %s"
          % (T - 1, host_s, 1e3 * host_s / (T - 1), same), flush=True)
    assert same


if __name__ == "__main__":
    main()
