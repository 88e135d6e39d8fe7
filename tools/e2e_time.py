"""End-to-end wall time of the two file flows of libagmv.so over the same synthetic clip, in one process:
  bmp   BMP files -> AGMV_EncodeFullAGMV -> .agmv -> AGMV_DecodeAGMV -> BMP files: disk + BMP parse / export + host LZ + PCIe + GPU
        (frames written with the host library's own BMP writer and synthetic generator)
  dev   frames in GPU memory (agmv_hip_synth_dev) -> AGMV_EncodeFramesDev(AGMV_SCHEDULE_FULL) -> .agmv -> AGMV_DecodeFramesDev ->
        frames in GPU memory (the clip and the destination are allocated outside the timed calls)
`both` alternates them `reps` times; the file sha of every run is printed, the two flows must agree on it.
usage: e2e_time.py W H T [batch=0 (library default)] [devices=1] [compression=1 (1 LZSS, 2 LZ77)] [flow=bmp (bmp, dev, both)] [reps=1]"""
import ctypes as C, glob, hashlib, os, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import hostlib as H
from libagmv_amd import abi
W, Hh, T = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 0
devices = int(sys.argv[5]) if len(sys.argv) > 5 else 1
comp = int(sys.argv[6]) if len(sys.argv) > 6 else 1
flow = sys.argv[7] if len(sys.argv) > 7 else "bmp"
reps = int(sys.argv[8]) if len(sys.argv) > 8 else 1
assert flow in ("bmp", "dev", "both")
L = abi.bind(C.CDLL(H.SO), abi.AGMV)
G = abi.bind(C.CDLL(os.path.join(R, "libagmv_amd", "libagmv_hip.so")), abi.HIP)
label = "%dx%d x %d frames (batch %d, %d GPU(s), %s)" % (W, Hh, T, batch, devices, "LZSS" if comp == 1 else "LZ77")


def sha_of(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def bmp_flow(t_gen):
    a = L.CreateAGMV(T, W, Hh, 24)
    t0 = time.perf_counter()
    L.AGMV_EncodeFullAGMV(a, b"out.agmv", b"fr", b"f", 1, 1, T, W, Hh, 24, 3, 1, comp)   # OPT_III, LOW quality
    t_enc = time.perf_counter() - t0
    size, sha = os.path.getsize("out.agmv"), sha_of("out.agmv")
    t0 = time.perf_counter()
    rc = L.AGMV_DecodeAGMV(b"out.agmv", 1, 1)
    t_dec = time.perf_counter() - t0
    print("e2e %s: write inputs %.2f s | AGMV_EncodeFullAGMV %.2f s = %.1f frames/s (file %.1f MB, sha %s) | AGMV_DecodeAGMV rc=%d %.2f s = %.1f frames/s"
          % (label, t_gen, t_enc, T / t_enc, size / 1e6, sha, rc, t_dec, T / t_dec), flush=True)
    for f in glob.glob("quick_export_*.bmp"):                  # (a repeat exports under new numbers: keep the disk at one clip)
        os.unlink(f)


def dev_flow(d_clip, d_out):
    t0 = time.perf_counter()
    rc = L.AGMV_EncodeFramesDev(b"dev.agmv", d_clip, T, W, Hh, 24, 3, 1, comp, 1)         # OPT_III, LOW quality, AGMV_SCHEDULE_FULL
    t_enc = time.perf_counter() - t0
    assert rc == 0, rc
    size, sha = os.path.getsize("dev.agmv"), sha_of("dev.agmv")
    t0 = time.perf_counter()
    n = L.AGMV_DecodeFramesDev(b"dev.agmv", d_out, T, None)
    t_dec = time.perf_counter() - t0
    print("e2e device frames %s: AGMV_EncodeFramesDev %.2f s = %.1f frames/s (file %.1f MB, sha %s) | AGMV_DecodeFramesDev %d frames %.2f s = %.1f frames/s"
          % (label, t_enc, T / t_enc, size / 1e6, sha, n, t_dec, T / t_dec), flush=True)


with tempfile.TemporaryDirectory(dir="/tmp") as td:
    os.chdir(td)
    L.AGMV_SetBatchFrames(batch)
    L.AGMV_SetDevices(devices)
    t_gen, d_clip, d_out = 0.0, None, None
    if flow != "dev":
        os.mkdir("fr")
        buf = np.zeros(W * Hh, np.uint32)
        t0 = time.perf_counter()
        for t in range(1, T + 1):
            L.AGMV_SynthFrame(buf.ctypes.data, W, Hh, t, 0xA6D5)
            H.write_bmp("fr/f%d.bmp" % t, buf.reshape(Hh, W))
        t_gen = time.perf_counter() - t0
    if flow != "bmp":                          # the same frames 1 .. T, made on the card of the library's own context
        ctx = G.agmv_hip_create(int(os.environ.get("AGMV_DEVICE", "0")))
        d_clip, d_out = G.agmv_hip_malloc(4 * W * Hh * T), G.agmv_hip_malloc(4 * W * Hh * T)
        assert ctx and d_clip and d_out, G.agmv_hip_last_error()
        assert G.agmv_hip_synth_dev(ctx, d_clip, W, Hh, 1, T, 0xA6D5, None) == 0 and G.agmv_hip_sync() == 0, G.agmv_hip_last_error()
    for _ in range(reps):
        if flow != "dev":
            bmp_flow(t_gen)
        if flow != "bmp":
            dev_flow(d_clip, d_out)
    G.agmv_hip_free(d_clip); G.agmv_hip_free(d_out)
