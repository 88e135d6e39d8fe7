"""Time the temporal stabilisation (agmv_hip_stabilise_frames_async, k_stabilise; include/agmv.h holds the rule) beside the encode
of the same frames (agmv_hip_encode_frames_dev, k_encode), in one process, and record what it does to files.
 1. 256 x 1920x1080: a still noisy clip (frame 0 of agmv_synth_v1 held, Gaussian noise of 3 levels per frame and channel) and the
    moving clip (agmv_synth_v1 itself), strengths 8, 16 and 32, against the HIGH_QUALITY OPT_III palette of the synthetic clip (the
    bench's).  The stabilisation works in place and a stabilised clip is a fixed point, so every timed call starts from a fresh
    copy of the clip; the copy lies outside the events.  Warm-up first, then HIP events around one call, median and min..max of
    REPS, the sides alternated.  Bytes moved: every frame read once plus 64 bytes written per replaced block (the device counter).
 2. Files (every frame coded, OPT_III, HIGH_QUALITY, LZSS): the noisy still clip of tests/stabilise_cases.py at sigma 0, 2, 3, 4 and
    the golden clip itself, plain and at strengths 8, 16 and 32: the file's bytes, the raw stream bytes of its chunks, the blocks
    replaced, and file_quality against the clean and against the noisy source.
usage: stabilise_time.py [reps=5] [out=profiles/stabilise/stabilise_time.txt]"""
import os
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import hostlib as H
import libagmv_amd
import stabilise_cases as S
from libagmv_amd import AgmvHip

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(R, "profiles", "stabilise", "stabilise_time.txt")
W, Hh, N = 1920, 1080, 256
STRENGTHS = (8, 16, 32)
HBM_PEAK = 8.0e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, before):
    before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(hip, name, clip, n):
    work = torch.empty_like(clip)
    out = torch.empty((n, hip.max_usize(W, Hh)), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    fresh = lambda: work.copy_(clip)
    sides = [("k_encode (agmv_hip_encode_frames_dev)", lambda: hip.encode_dev(work, n, W, Hh, out=out, sizes=sizes))]
    sides += [("k_stabilise, strength %d" % s, (lambda s: lambda: hip.stabilise_frames(work.reshape(-1), W, Hh, s, 0, count))(s)) for s in STRENGTHS]
    replaced = {}
    for k, fn in sides:                                       # warm-up of every shape; the counter of each strength
        fresh()
        count.zero_()
        fn()
        torch.cuda.synchronize()
        replaced[k] = int(count.item())
    hip.check()
    ts = {k: [] for k, _ in sides}
    for _ in range(REPS):
        for k, fn in sides:
            ts[k].append(timed(fn, fresh))
    enc = float(np.median(ts[sides[0][0]]))
    examined = (n - (n + 3) // 4) * (W * Hh // 16)
    for k, _ in sides:
        ms = float(np.median(ts[k]))
        line = "%-12s %-40s median of %d = %8.3f ms (min %.3f .. max %.3f)" % (name, k, REPS, ms, min(ts[k]), max(ts[k]))
        if k != sides[0][0]:
            moved = n * W * Hh * 4 + replaced[k] * 64
            line += "; %5.1f %% of %d blocks replaced, %.3f GB moved = %.2f TB/s = %2.0f %% of the 8 TB/s HBM peak; %.3f x k_encode" % (
                100.0 * replaced[k] / examined, examined, moved / 1e9, moved / ms / 1e9, 100.0 * moved / (ms * 1e-3) / HBM_PEAK, ms / enc)
        say(line)
    hip.check()


def kernel_times():
    hip = AgmvHip(0)
    synth = hip.synth_dev(W, Hh, 0, N)
    hist = hip.histogram_dev(synth.reshape(-1), 1)
    torch.cuda.synchronize()
    p0, p1 = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    H.lib().AGMV_BuildPalette(hist.cpu().numpy().view(np.uint32), 1, 3, p0, p1)
    hip.set_palette(p0.astype(np.uint32), p1.astype(np.uint32), True)
    say("%s; %d x 1920x1080, in place, every timed call on a fresh copy of the clip; HIP events around one call" % (torch.cuda.get_device_name(0), N))
    measure(hip, "moving", synth, N)
    g = torch.Generator(device="cuda").manual_seed(7)
    still = torch.empty_like(synth)
    f0 = synth[0].to(torch.int64)
    for k in range(N):                                        # frame by frame: the noise of one frame at a time
        ch = [torch.clamp(((f0 >> sh) & 255) + torch.round(torch.randn((Hh, W), device="cuda", generator=g) * 3.0).to(torch.int64), 0, 255) for sh in (16, 8, 0)]
        still[k] = (ch[0] << 16 | ch[1] << 8 | ch[2]).to(torch.int32)
    del synth
    measure(hip, "still+noise", still, N)
    hip.close()


def stream_bytes(path):
    """the sum of the usize fields of a file's frame chunks (no audio): the raw bitstream bytes before LZ"""
    data = open(path, "rb").read()
    total, pos = 0, data.find(b"AGFC")
    while 0 <= pos and pos + 16 <= len(data):
        total += int.from_bytes(data[pos + 8:pos + 12], "little")
        pos += 24 + int.from_bytes(data[pos + 12:pos + 16], "little")           # (eight bytes 0xFF lie behind every payload)
        assert pos == len(data) or data[pos:pos + 4] == b"AGFC"
    return total


def files():
    import dither_cases as D
    say("")
    say("files: AGMV_SCHEDULE_FULL, OPT_III, HIGH_QUALITY, LZSS; PSNR of the decoded file (file_quality) against the clean and the noisy source")
    fox = D.fox()[0]
    clips = [("still, sigma %d" % sg,) + S.noisy_still_clip(sg) if sg else ("still, sigma 0",) + (S.noisy_still_clip(1)[1],) * 2 for sg in (0, 2, 3, 4)]
    clips.append(("golden clip", fox, fox))
    with tempfile.TemporaryDirectory() as d:
        for name, noisy, clean in clips:
            dn, dc = (torch.from_numpy(x.view(np.int32).copy()).cuda() for x in (noisy, clean))
            for s in (0,) + STRENGTHS:
                path = os.path.join(d, "f.agmv")
                libagmv_amd.encode_frames(path, dn, opt=3, quality=1, compression=1, schedule=1, **({"stabilise": s} if s else {}))
                examined, replaced = libagmv_amd.stabilise_stats()
                say("%-16s %-12s file %8d bytes, streams %8d bytes, %6d of %6d blocks replaced, PSNR %6.2f dB against the clean source, %6.2f dB against the noisy one"
                    % (name, "strength %d" % s if s else "plain", os.path.getsize(path), stream_bytes(path), replaced, examined,
                       libagmv_amd.file_quality(path, dc).psnr(), libagmv_amd.file_quality(path, dn).psnr()))


def main():
    kernel_times()
    torch.cuda.empty_cache()
    files()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
