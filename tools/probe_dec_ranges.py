# agmv_hip_decode_bitstreams_dev (the bench's decode call) cut into ranges of AGMV_DEC_RANGE_FRAMES frames: parser and
# k_decode + k_fixup event times summed over the ranges, each leg a median of 7 calls after 2, and a pixel checksum, on
#   synth    the bench clip, 1024 x 1080p
#   noise3   its NORMAL-heavy variant (3 bits of noise per channel), 512 x 1080p
#   720p     2048 x 1280x720 of the synthetic clip
#   qvga     8192 x 320x240 of the synthetic clip
# Range 0 is the uncut call (one range up to 65532 frames), range -1 the library's own choice (the variable unset).  One
# process; PROBE_LIB=path times another build of the library.
#   python tools/probe_dec_ranges.py [range ...]
import os
import sys

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import synth as S  # noqa: E402
from libagmv_amd import AgmvHip  # noqa: E402

RANGES = [int(a) for a in sys.argv[1:]] or [0, 128, 256, 340, 512]
hip = AgmvHip(0, lib=os.environ.get("PROBE_LIB"))
hip.enable_timing(True)
med = lambda a: sorted(a)[len(a) // 2]


def legs(kind, W, H, T, noise):
    p0, p1 = S.content_palettes([S.synth_frame(W, H, t) for t in range(2)])
    hip.set_palette(p0, p1, True)
    clip = hip.synth_dev(W, H, 0, T)
    if noise:
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for sh in (0, 8, 16):
            clip ^= torch.randint(0, 8, clip.shape, dtype=torch.int32, device="cuda", generator=g) << sh
    out, sizes = hip.encode_dev(clip, T, W, H)
    del clip
    dec = torch.empty((T, H, W), dtype=torch.int32, device="cuda")
    nent = torch.empty(T, dtype=torch.int32, device="cuda")
    usize = float(sizes.float().mean())
    for rng in RANGES:
        os.environ["AGMV_DEC_RANGE_FRAMES"] = str(rng)
        if rng < 0:
            del os.environ["AGMV_DEC_RANGE_FRAMES"]
        tp, td, ts = [], [], []
        dec.zero_()
        for i in range(9):
            hip.decode_bitstreams_dev(out, sizes, T, W, H, out=dec, nentered=nent)
            if i >= 2:
                tp.append(hip.last_kernel_ms(1))
                td.append(hip.last_kernel_ms(2))
                ts.append(tp[-1] + td[-1])
        hip.check()
        torch.cuda.synchronize()
        cs = int((dec.to(torch.int64) & 0xFFFFFF).sum().item())       # equal between two legs that decode the same
        print("%-7s %4dx%-4d T=%-5d range %-4d parse %.4f  k_decode+k_fixup %.4f  sum %.4f (min %.4f max %.4f) ms | mean usize %.0f | pixels %d" %
              (kind, W, H, T, rng, med(tp), med(td), med(ts), min(ts), max(ts), usize, cs), flush=True)
    del dec, out
    torch.cuda.empty_cache()


legs("synth", 1920, 1080, 1024, False)
legs("noise3", 1920, 1080, 512, True)
legs("720p", 1280, 720, 2048, False)
legs("qvga", 320, 240, 8192, False)
hip.close()
