# k_decode + k_fixup event time through agmv_hip_decode_bitstreams_dev (the bench's decode call), median of 7, on
#   synth   the bench clip: T x 1080p (default 1024 = c3) and its first 256 frames
#   noise3  the NORMAL-heavy variant (3 bits of noise per channel): 512 frames and the first 256
# PROBE_LIB=path times another build of the library (one process per build: the kernels carry the same names).
#   python tools/probe_dec_pipeline.py [label]
import os
import sys

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import synth as S  # noqa: E402
from libagmv_amd import AgmvHip  # noqa: E402

W, H, T = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080")), int(os.environ.get("T", "1024"))
label = sys.argv[1] if len(sys.argv) > 1 else "library"
hip = AgmvHip(0, lib=os.environ.get("PROBE_LIB"))
p0, p1 = S.content_palettes([S.synth_frame(W, H, t) for t in range(2)])
hip.set_palette(p0, p1, True)
hip.enable_timing(True)
frames = hip.synth_dev(W, H, 0, T)
dec = torch.empty((T, H, W), dtype=torch.int32, device="cuda")
nent = torch.empty(T, dtype=torch.int32, device="cuda")
med = lambda a: sorted(a)[len(a) // 2]


def leg(kind, clip, n):
    out, sizes = hip.encode_dev(clip[:n], n, W, H)
    tp, td = [], []
    for i in range(9):
        hip.decode_bitstreams_dev(out, sizes, n, W, H, out=dec[:n], nentered=nent[:n])
        if i >= 2:
            tp.append(hip.last_kernel_ms(1))
            td.append(hip.last_kernel_ms(2))
    hip.check()
    torch.cuda.synchronize()
    # a checksum of the pixels: equal between two builds that decode the same
    cs = int((dec[:n].view(torch.int32).to(torch.int64) & 0xFFFFFF).sum().item())
    print("%-10s %-6s T=%-4d parse %.3f  k_decode+k_fixup %.3f (min %.3f max %.3f) ms | mean usize %.0f | sum %d" %
          (label, kind, n, med(tp), med(td), min(td), max(td), float(sizes.float().mean()), cs), flush=True)


leg("synth", frames, T)
leg("synth", frames, min(T, 256))
n = min(T, 512)
g = torch.Generator(device="cuda")
g.manual_seed(7)
clip = frames[:n].clone()
for sh in (0, 8, 16):
    clip ^= torch.randint(0, 8, clip.shape, dtype=torch.int32, device="cuda", generator=g) << sh
leg("noise3", clip, n)
leg("noise3", clip, min(n, 256))
hip.close()
