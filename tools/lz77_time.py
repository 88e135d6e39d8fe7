"""Time the LZ77 stage on the GPU (agmv_hip_lz77_peek_dev + agmv_hip_lz77_frames_dev) against the host pool (agmv_lz77_mem
on N threads) on the same bytes, in one process: the c3 bitstreams (T x 1920x1080 agmv_synth_v1, HIGH_QUALITY palette,
OPT_III, encoded on the GPU as bench.py does) and single 4.2 MB frames (all-zero, period 2, period 256, noise, 4-symbol
noise) against one host thread.  GPU: HIP events around peek + compress, median of REPS (min..max shown); the host pool
is timed REPS times too.  The host needs minutes for 4.2 MB of zeros, so its time is taken on 300 KB of zeros and the GPU
output of the 4.2 MB frame is checked against the closed form (tests/lz77_cases.py).
usage: lz77_time.py [T=256] [threads=16] [reps=5]"""
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
import lz77_cases as Z
from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 256
THREADS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def gpu_time(hip, bits, sizes, n):
    plen = bits.stride(0) + 64
    persist = torch.zeros(plen, dtype=torch.uint8, device="cuda")
    peek = hip.lz77_peek_dev(bits, sizes, n, persist)
    out, cs = hip.lz77_frames_dev(bits, sizes, n, peek=peek)        # warm-up (grows the work areas)
    ts = []
    for _ in range(REPS):
        persist.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.lz77_peek_dev(bits, sizes, n, persist, peek=peek)
        hip.lz77_frames_dev(bits, sizes, n, peek=peek, out=out, csize=cs)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts, out, cs, peek.cpu().numpy()[:n]


def host_pool(rows, peek, threads, reps):
    L = H.lib()
    outs = [np.zeros(4 * len(x) + 64, np.uint8) for x in rows]
    ins = [np.concatenate([x, np.full(8, peek[k], np.uint8)]) for k, x in enumerate(rows)]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            cs = list(ex.map(lambda k: int(L.agmv_lz77_mem(ins[k], len(rows[k]), outs[k])), range(len(rows))))
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, [o[:c] for o, c in zip(outs, cs)], cs


def same(out, cs, host_pay, host_cs):
    cs = cs.cpu().numpy().view(np.uint32)
    o = out.cpu().numpy()
    return all(int(cs[f]) == host_cs[f] and (o[f, :cs[f]] == host_pay[f]).all() for f in range(len(host_cs)))


def spread(ts):
    return "%.1f ms (%.1f..%.1f)" % (float(np.median(ts)), min(ts), max(ts))


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
    g_ts, out, cs, peek = gpu_time(hip, bits, sizes, T)
    reparsed = hip.lz77_reparsed_segments()
    nseg = int(sum((int(s) + Z.SEG - 1) // Z.SEG for s in sz))
    b = bits.cpu().numpy()
    rows = [b[f, :sz[f]].copy() for f in range(T)]
    exp_peek = Z.prepare_batch_peek([b[f] for f in range(T)], sz, np.zeros(bits.stride(0) + 64, np.uint8))
    del b
    h_ts, hp, hc = host_pool(rows, exp_peek, THREADS, min(REPS, 3))
    ok = same(out, cs, hp, hc) and bool((peek == exp_peek).all())
    g_ms, h_ms = float(np.median(g_ts)), float(np.median(h_ts))
    print("c3 %d x 1920x1080: %.1f MB pre-LZ -> %.1f MB, %d tokens | GPU %s (%.2f GB/s) | host pool %d threads %s | %.1fx | "
          "%d of %d segments re-parsed (%.0f %%) | bit-exact %s"
          % (T, total / 1e6, sum(hc) / 1e6, sum(hc) // 4, spread(g_ts), total / g_ms / 1e6, THREADS, spread(h_ts), h_ms / g_ms,
             reparsed, nseg, 100.0 * reparsed / nseg, ok), flush=True)
    c3_rate = total / g_ms
    del out, cs, bits
    rng = np.random.default_rng(5)
    n = 4 << 20
    shapes = {"zero": np.zeros(n, np.uint8),
              "period2": np.tile(rng.integers(0, 256, 2, dtype=np.uint8), n // 2),
              "period256": np.tile(rng.permutation(256).astype(np.uint8), n // 256),
              "noise": rng.integers(0, 256, 4_300_000, dtype=np.uint8),
              "noise4": rng.integers(0, 4, n, dtype=np.uint8)}
    for name, x in shapes.items():
        d = torch.from_numpy(x[None, :].copy()).cuda()
        s = torch.tensor([len(x)], dtype=torch.int32, device="cuda")
        g_ts, out, cs, _ = gpu_time(hip, d, s, 1)
        g = float(np.median(g_ts))
        if name == "zero":
            small = 300_000
            h_ts, _, _ = host_pool([x[:small]], [0], 1, 1)
            exp = Z.zeros_closed_form(len(x), 0)
            ok = int(cs[0]) == len(exp) and bool((out[0, :len(exp)].cpu().numpy() == exp).all())
            host = "host 1 thread %.1f ms for %.1f MB of it (closed form checked at full size)" % (h_ts[0], small / 1e6)
        else:
            h_ts, hp, hc = host_pool([x], [0], 1, 1)
            ok = same(out, cs, hp, hc)
            host = "host 1 thread %.1f ms" % h_ts[0]
        print("%-9s %.1f MB: GPU %s (%.2f GB/s, %.1fx the c3 time per byte) | %s | bit-exact %s"
              % (name, len(x) / 1e6, spread(g_ts), len(x) / g / 1e6, c3_rate / (len(x) / g), host, ok), flush=True)
    hip.close()


if __name__ == "__main__":
    main()
