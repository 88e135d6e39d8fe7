"""Time the audio kernels ("audio tracks" of include/agmv.h) on 10 minutes of 48 kHz stereo, 57.6 M samples, as S16 and as F32P:
  1  agmv_hip_audio_compand_async and agmv_hip_audio_expand_async on resident buffers: HIP events around one launch, warm, median
     and min..max of REPS launches; the bytes each launch must move (PCM + one code byte per sample) over that time, and that
     rate as a fraction of the 8 TB/s peak of the memory
  2  what a caller has without the kernels: the download of the PCM to pinned host memory (events), and this library's own
     AGMV_CompressAudio over the track on one host thread (wall time)
There is no target.  What is printed is also written to profiles/audio/audio_time.txt (or argv[3]).
usage: audio_time.py [seconds=600] [reps=20] [out]"""
import ctypes as C
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from libagmv_amd import AgmvHip, seq

SECONDS = int(sys.argv[1]) if len(sys.argv) > 1 else 600
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(R, "profiles", "audio", "audio_time.txt")
RATE, CH, PEAK = 48000, 2, 8.0e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    """median, min, max in ms of REPS launches after a warm-up"""
    ms = []
    for rep in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    hip = AgmvHip(0)
    L = seq.load_library()
    n = SECONDS * RATE
    total = n * CH
    say("audio kernels on %d s of %d Hz, %d channels: %.1f M samples, %d launches each" % (SECONDS, RATE, CH, total / 1e6, REPS))
    s16 = torch.randint(-32768, 32768, (n, CH), dtype=torch.int16, device="cuda")
    f32 = (torch.rand((CH, n), device="cuda") * 2 - 1).contiguous()
    codes = torch.empty((n, CH), dtype=torch.uint8, device="cuda")
    for name, fmt, pcm, width in (("S16", "s16", s16, 2), ("F32P", "f32p", f32, 4)):
        moved = total * (width + 1)
        back = torch.empty_like(pcm)
        for what, fn in (("compand", lambda: hip.audio_compand(fmt, pcm, codes=codes)), ("expand", lambda: hip.audio_expand(fmt, codes, pcm=back))):
            med, lo, hi = timed(fn)
            say("%-4s %-7s %.3f ms (min %.3f .. max %.3f): %d bytes moved, %.2f TB/s, %.1f %% of the 8 TB/s peak"
                % (name, what, med, lo, hi, moved, moved / (med * 1e-3) / 1e12, 100.0 * moved / (med * 1e-3) / PEAK))
    # the host side: the PCM comes down, then one thread compands it
    pinned = torch.empty((n, CH), dtype=torch.int16).pin_memory()
    med, lo, hi = timed(lambda: pinned.copy_(s16, non_blocking=True))
    say("S16  download of the PCM to pinned host memory %.2f ms (min %.2f .. max %.2f), %.1f GB/s" % (med, lo, hi, total * 2 / (med * 1e-3) / 1e9))
    a = L.CreateAGMV(1, 4, 4, 1)
    L.AGMV_SetAudioSize(a, total)
    host = pinned.numpy().view(np.uint16)
    out = np.zeros(total, np.uint8)
    track = C.c_void_p.from_address(a + 4216).value               # AGMV.audio_track -> pcm, AGMV.audio_chunk -> atsample (include/agmv.h)
    chunk = C.c_void_p.from_address(a + 4184).value
    C.c_void_p.from_address(track + 16).value = host.ctypes.data
    C.c_void_p.from_address(chunk + 16).value = out.ctypes.data
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        L.AGMV_CompressAudio(a)
        wall.append(1e3 * (time.perf_counter() - t0))
    C.c_void_p.from_address(track + 16).value = None              # the buffers are numpy's: the object must not free them
    C.c_void_p.from_address(chunk + 16).value = None
    got = hip.audio_compand("s16", s16).cpu().numpy().reshape(-1)
    say("S16  AGMV_CompressAudio on one host thread %.1f ms (min %.1f .. max %.1f); its codes equal the kernel's: %s"
        % (float(np.median(wall)), min(wall), max(wall), bool((got == out).all())))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
