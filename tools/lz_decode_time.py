"""Time the decoder's LZ stage on the GPU (agmv_hip_lz_decode_frames_dev + agmv_hip_lz_decode_commit_dev) against the host
pool (agmv_lz_decode_mem on N threads, as the sequence decoder runs it) on the same bytes, in one process.  Payloads: the
c3 bitstreams (T x 1920x1080 agmv_synth_v1, HIGH_QUALITY palette, OPT_III, encoded on the GPU as bench.py does),
compressed with LZSS (agmv_hip_lzss_frames_dev, bit-exact with the host) and with LZ77 (host agmv_lz77_mem, T77 frames), laid
out as in a file (chunk header, payload, 0xFF guard); then worst-case shapes (all-literal noise, a frame-long offset-1 chain,
all-zero LZ77 runs).  GPU: HIP events, median of REPS.  Every result is compared with the host's: bpos, used and the bytes.
usage: lz_decode_time.py [T=1024] [threads=16] [reps=5] [T77=256]"""
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
import lz_decode_cases as Z
from libagmv_amd import AgmvHip

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
THREADS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
T77 = int(sys.argv[4]) if len(sys.argv) > 4 else 256


def layout(pays, usizes):
    """file image: header, payload, guard per frame -> device src / off / avail / usize / csize"""
    parts, off, pos = [], [], 0
    for p, u in zip(pays, usizes):
        hdr = b"AGFC" + bytes(4) + int(u).to_bytes(4, "little") + len(p).to_bytes(4, "little")
        parts += [np.frombuffer(hdr, np.uint8), p, np.frombuffer(Z.GUARD[:8], np.uint8)]
        off.append(pos + 16)
        pos += 16 + len(p) + 8
    src = np.concatenate(parts)
    avail = [len(src) - o for o in off]
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int64).astype(np.uint32).view(np.int32)).cuda()   # noqa: E731
    return src, off, (torch.from_numpy(src).cuda(), torch.tensor(off, dtype=torch.int64).cuda(), i32(avail), i32(usizes),
                      i32([len(p) for p in pays]))


def gpu_time(hip, version, dev, n, cap):
    bits = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
    per = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hip.lz_decode_frames_dev(version, *dev, n, cap, bits=bits)                 # warm-up (grows the work areas)
    ts = []
    for _ in range(REPS):
        per.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, bpos, used = hip.lz_decode_frames_dev(version, *dev, n, cap, bits=bits)
        hip.lz_decode_commit_dev(bits, bpos, n, per)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), bits, bpos, used, hip.lz_decode_fallback_frames()


def host_pool(version, src, off, usizes, csizes, cap, threads):
    L = H.lib()
    rows = [np.zeros(cap, np.uint8) for _ in off]
    bp = [0] * len(off)
    us = [0] * len(off)

    def one(k):
        u = C.c_size_t(0)
        view = src[off[k]:]
        bp[k] = int(L.agmv_lz_decode_mem(version, view, len(view), int(usizes[k]), int(csizes[k]), rows[k], cap, C.byref(u)))
        us[k] = u.value
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(len(off))))
    return (time.perf_counter() - t0) * 1e3, rows, bp, us


def same(bits, bpos, used, rows, bp, us):
    gb = bpos.cpu().numpy().view(np.uint32)
    gu = used.cpu().numpy().view(np.uint32)
    if list(gb) != bp or list(gu) != us:
        return False
    for k in range(len(bp)):
        if not torch.equal(bits[k, :bp[k]], torch.from_numpy(rows[k][:bp[k]]).cuda()):
            return False
    return True


def compare(name, hip, version, pays, usizes, threads):
    src, off, dev = layout(pays, usizes)
    cap = int(max(usizes)) + 4096
    n = len(pays)
    g, bits, bpos, used, fb = gpu_time(hip, version, dev, n, cap)
    h, rows, bp, us = host_pool(version, src, off, usizes, [len(p) for p in pays], cap, threads)
    ok = same(bits, bpos, used, rows, bp, us)
    out = sum(bp)
    print("%-22s %4d frames: %.1f MB payload -> %.1f MB | GPU decode+commit %.1f ms (%.2f GB/s out) | host pool %d thread(s) %.1f ms | "
          "%.2fx | fallback frames %d | bit-exact %s" % (name, n, sum(len(p) for p in pays) / 1e6, out / 1e6, g, out / g / 1e6, threads, h,
                                                         h / g, fb, ok), flush=True)


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
    pay, cs = hip.lzss_frames_dev(bits, sizes, T)
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy().view(np.uint32)
    csz = cs.cpu().numpy().view(np.uint32)
    p = pay.cpu().numpy()
    pays = [p[f, :csz[f]].copy() for f in range(T)]
    del p, pay
    compare("c3 LZSS", hip, 1, pays, sz, THREADS)
    b = bits[:T77].cpu().numpy()
    rows = [np.concatenate([b[f, :sz[f]], np.zeros(8, np.uint8)]) for f in range(T77)]
    del b, bits
    outs = [np.zeros(4 * len(x) + 64, np.uint8) for x in rows]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        c77 = list(ex.map(lambda k: int(H.lib().agmv_lz77_mem(rows[k], len(rows[k]) - 8, outs[k])), range(T77)))
    print("(host agmv_lz77_mem on %d threads: %d x 1080p frames in %.1f s)" % (THREADS, T77, time.perf_counter() - t0), flush=True)
    compare("c3 LZ77", hip, 3, [o[:c] for o, c in zip(outs, c77)], sz[:T77], THREADS)
    del rows, outs
    rng = np.random.default_rng(5)
    n = 4 << 20
    noise, _ = H.lzss(rng.integers(0, 256, n, dtype=np.uint8))
    compare("noise (all-literal)", hip, 1, [noise], [n], 1)
    chain = Z.lzss_frame([("L", 0x5A)] + [("M", 1, 15)] * (n // 15))
    compare("offset-1 chain LZSS", hip, 1, [np.frombuffer(chain.payload, np.uint8)], [chain.usize], 1)
    zeros, _ = H.lz77(np.zeros(n, np.uint8))
    compare("zero runs LZ77", hip, 3, [zeros], [n], 1)
    hip.close()


if __name__ == "__main__":
    main()
