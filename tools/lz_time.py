"""Time the LZSS stage on the GPU (agmv_hip_lzss_frames_dev) against the host pool (agmv_lzss_mem on N threads) on the same
bytes, in one process: the c3 bitstreams (T x 1920x1080 agmv_synth_v1, HIGH_QUALITY palette, OPT_III, encoded on the GPU
as bench.py does) and the worst-case shapes (all-zero, period 2, period 15, noise).  GPU: HIP events, median of REPS.
usage: lz_time.py [T=1024] [threads=16] [reps=5]"""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import hostlib as H
from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
THREADS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def gpu_time(hip, bits, sizes, n):
    out, cs = hip.lzss_frames_dev(bits, sizes, n)                  # warm-up (grows the work areas)
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.lzss_frames_dev(bits, sizes, n, out=out, csize=cs)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out, cs


def host_pool(rows):
    L = H.lib()
    outs = [np.zeros(2 * len(x) + 64, np.uint8) for x in rows]
    ins = [np.concatenate([x, np.zeros(8, np.uint8)]) for x in rows]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        cs = list(ex.map(lambda k: int(L.agmv_lzss_mem(ins[k], len(rows[k]), outs[k])), range(len(rows))))
    dt = time.perf_counter() - t0
    return dt * 1e3, [o[:c] for o, c in zip(outs, cs)], cs


def same(out, cs, host_pay, host_cs):
    cs = cs.cpu().numpy().view(np.uint32)
    o = out.cpu().numpy()
    return all(int(cs[f]) == host_cs[f] and (o[f, :cs[f]] == host_pay[f]).all() for f in range(len(host_cs)))


def main():
    hip = AgmvHip(0)
    W, Hh, q = 1920, 1080, 1
    frames = hip.synth_dev(W, Hh, 0, T)
    hist = hip.histogram_dev(frames.reshape(-1), q)
    torch.cuda.synchronize()
    p0, p1 = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    H.lib().AGMV_BuildPalette(hist.cpu().numpy().view(np.uint32), q, 3, p0, p1)
    hip.set_palette(p0.astype(np.uint32), p1.astype(np.uint32), True)
    bits, sizes = hip.encode_dev(frames, T, W, Hh)
    hip.check()
    del frames
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy().view(np.uint32)
    total = int(sz.sum())
    g_ms, out, cs = gpu_time(hip, bits, sizes, T)
    b = bits.cpu().numpy()
    rows = [b[f, :sz[f]].copy() for f in range(T)]
    del b
    h_ms, hp, hc = host_pool(rows)
    ok = same(out, cs, hp, hc)
    print("c3 %d x 1920x1080: %.1f MB pre-LZ -> %.1f MB | GPU %.1f ms (%.2f GB/s) | host pool %d threads %.1f ms | %.1fx | bit-exact %s"
          % (T, total / 1e6, sum(hc) / 1e6, g_ms, total / g_ms / 1e6, THREADS, h_ms, h_ms / g_ms, ok), flush=True)
    c3_rate = total / g_ms
    del out, cs, bits
    rng = np.random.default_rng(5)
    n = 4 << 20
    shapes = {"zero": np.zeros(n, np.uint8),
              "period2": np.tile(rng.integers(0, 256, 2, dtype=np.uint8), n // 2),
              "period15": np.tile(rng.integers(0, 256, 15, dtype=np.uint8), n // 15 + 1)[:n],
              "noise": rng.integers(0, 256, 4_300_000, dtype=np.uint8)}
    for name, x in shapes.items():
        d = torch.from_numpy(x[None, :].copy()).cuda()
        s = torch.tensor([len(x)], dtype=torch.int32, device="cuda")
        g, out, cs = gpu_time(hip, d, s, 1)
        h, hp, hc = host_pool([x])
        print("%-9s %.1f MB: GPU %.1f ms (%.2f GB/s, %.1fx the c3 time per byte) | host 1 thread %.1f ms | bit-exact %s"
              % (name, len(x) / 1e6, g, len(x) / g / 1e6, c3_rate / (len(x) / g), h, same(out, cs, hp, hc)), flush=True)
    hip.close()


if __name__ == "__main__":
    main()
