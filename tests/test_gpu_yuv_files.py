"""Whole files from and to clips in 8-bit YUV 4:2:0: AGMV_EncodeFramesFmtDev / AGMV_DecodeFramesFmtDev of libagmv_amd/libagmv.so
with AGMV_PIXFMT_NV12 / AGMV_PIXFMT_I420, and libagmv_amd.seq on torch tensors.

Encode: the clips of tests/memseq_cases.py are written to YUV in numpy (tests/yuv_cases.py) and read back in numpy; that is the
comparator clip, the XRGB32 clip the YUV clip stands for.  AGMV_EncodeFramesFmtDev(YUV clip) must write the bytes that
AGMV_EncodeFramesDev(comparator clip) writes in the same child: the palette then comes from agmv_hip_yuv_histogram_dev, plain
frames from agmv_hip_yuv_to_xrgb_dev, scaled ones from agmv_hip_yuv_gather_dev, midpoints from both, and on the mixed clip the
counts of agmv_hip_yuv_similarity_dev decide which frames exist.  Decode: agmv_splash.agmv (escape frames and stale tails) into
a YUV sink must be numpy's writing of the XRGB32 decode.  Child processes as in tests/test_gpu_pixfmt_files.py.  Needs an MI355X."""
import functools
import json
import os
import textwrap

import numpy as np
import pytest

import children as K
import memseq_cases as MC
import yuv_cases as Y

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden")
FULL, PDIFS, ADAPTIVE = 1, 2, 3
NV12_601, I420_601 = Y.NV12, Y.I420
NV12_709F, I420_709F = Y.NV12 | Y.BT709 | Y.FULL_RANGE, Y.I420 | Y.BT709 | Y.FULL_RANGE
LENIENCY = {3: 0.2282, 1: 0.2282}                  # AGMV_OPT_III, AGMV_OPT_I (heavy PDIFS)

CHILD = textwrap.dedent("""
    L.AGMV_SetBatchFrames(job["batch"])
    res = {"enc_rc": [], "dec": []}

    for e in job.get("enc", []):             # the YUV clip through FmtDev, then the comparator clip through AGMV_EncodeFramesDev
        raw, packed = np.load(e["yuv"]), np.load(e["packed"])
        n, h, w = packed.shape
        args = [n, w, h, 24, e["opt"], e["quality"], e["compression"], e["schedule"]]
        d = upload(raw)
        rc = [L.AGMV_EncodeFramesFmtDev(e["out"].encode(), d, e["fmt"], *args)]
        free(d)
        d = upload(packed)
        rc.append(L.AGMV_EncodeFramesDev((e["out"] + ".packed").encode(), d, *args))
        free(d)
        res["enc_rc"].append(rc)
    for e in job.get("dec", []):             # fmt 1: the XRGB32 decode
        path = e["path"].encode()
        info = INFO()
        rc_info = L.AGMV_DecodeFramesFmtDev(path, None, e["fmt"], 0, C.byref(info))
        n, w, h = info.number_of_frames, info.width, info.height
        fb = 4 * w * h if e["fmt"] == 1 else G.agmv_hip_yuv_frame_bytes(e["fmt"], w, h)
        d = poisoned(n * fb)                                            # what a frame that is not decoded keeps
        rc = L.AGMV_DecodeFramesFmtDev(path, d, e["fmt"], e.get("cap", n), None)
        np.save(e["out"], download(d, n * fb))
        free(d)
        res["dec"].append({"info_rc": rc_info, "rc": rc, "n": n, "w": w, "h": h, "fb": fb})
    print(json.dumps(res))
""")

# libagmv_amd.seq on torch tensors, in a child as well (the drivers keep process-wide state)
SEQ_CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    nv12 = torch.from_numpy(np.load("nv12.npy")).cuda()                     # uint8 [n, h * 3 / 2, w]
    i420 = torch.from_numpy(np.load("i420.npy")).cuda()
    libagmv_amd.encode_frames("nv12.agmv", nv12, fmt="nv12")
    libagmv_amd.encode_frames("i420.agmv", i420, fmt="i420", yuv="bt709", full_range=True)
    refused = 0
    try:
        libagmv_amd.encode_frames("none.agmv", nv12)                        # a YUV layout is never inferred
    except ValueError:
        refused = 1
    a, info = libagmv_amd.decode_frames("nv12.agmv", fmt="nv12")
    b, _ = libagmv_amd.decode_frames("nv12.agmv", fmt="i420", yuv="bt709", full_range=True)
    packed, _ = libagmv_amd.decode_frames("nv12.agmv")
    np.save("dec_nv12.npy", a.cpu().numpy()); np.save("dec_i420.npy", b.cpu().numpy()); np.save("dec_packed.npy", packed.cpu().numpy())
    print(json.dumps({"nv12": [str(a.dtype), list(a.shape)], "i420": [str(b.dtype), list(b.shape)], "refused": refused,
                      "frames": int(info.number_of_frames)}))
""")


def run_child(cwd, job, env=None, script=CHILD):
    return K.run_child(cwd, script, job, env, prelude="" if script is SEQ_CHILD else K.PRELUDE)


@functools.lru_cache(maxsize=None)
def clips(which, fmt):
    """(the clip written to YUV in numpy: uint8 [n, frame bytes], the comparator clip read back from it: uint32 [n, h, w])"""
    src = {"synth": lambda: MC.synth_clip(160, 128, 12), "odd": lambda: MC.synth_clip(321, 243, 8), "mixed": MC.mixed_clip}[which]()
    n, h, w = src.shape
    raw = Y.from_packed(fmt, src, w, h)
    packed = Y.to_packed(fmt, raw, w, h)
    raw.setflags(write=False)
    packed.setflags(write=False)
    return raw, packed


def grey(p):
    return (((p >> 16) & 255) + ((p >> 8) & 255) + (p & 255)) // 3


def chain_of(packed, opt):
    """the decisions AGMV_SCHEDULE_ADAPTIVE takes on a clip, from the grey-equality counts of its adjacent pairs in numpy"""
    n, h, w = packed.shape
    g = grey(packed.reshape(n, -1))
    ratio = [np.float32((g[k] == g[k + 1]).sum()) / np.float32(w * h) for k in range(n - 1)]          # pair (k + 1, k + 2)
    return MC.adaptive_chain(lambda x: ratio[x - 1] >= np.float32(LENIENCY[opt]), n, opt == 1)


# (format, clip, schedule, opt, quality, compression)
ENCODE = [(NV12_601, "synth", PDIFS, 3, 3, 1), (I420_709F, "synth", PDIFS, 3, 3, 1), (NV12_709F, "synth", FULL, 1, 2, 1),
          (I420_601, "synth", PDIFS, 1, 3, 2), (I420_601, "synth", FULL, 3, 1, 1), (NV12_601, "mixed", ADAPTIVE, 3, 3, 1),
          (I420_709F, "mixed", ADAPTIVE, 3, 3, 1), (NV12_709F, "mixed", ADAPTIVE, 1, 3, 1), (NV12_709F, "odd", PDIFS, 7, 3, 1),
          (I420_601, "odd", PDIFS, 5, 3, 1), (NV12_601, "odd", ADAPTIVE, 8, 3, 1)]


def case_id(c):
    return "%s-%s-%s-sched%d-opt%d-q%d-lz%d" % (Y.NAMES[c[0] & 0xFF], Y.FLAG_NAMES[c[0] & 0x300], c[1], c[2], c[3], c[4], c[5])


def encode_both(tmp_path, case, env=None):
    fmt, which, schedule, opt, quality, compression = case
    raw, packed = clips(which, fmt)
    np.save(tmp_path / "yuv.npy", raw)
    np.save(tmp_path / "packed.npy", packed)
    job = {"fmt": fmt, "yuv": "yuv.npy", "packed": "packed.npy", "out": "out.agmv", "opt": opt, "quality": quality, "compression": compression,
           "schedule": schedule}
    res = run_child(tmp_path, {"batch": 8, "enc": [job]}, env)
    assert res["enc_rc"] == [[0, 0]]
    a, b = open(tmp_path / "out.agmv", "rb").read(), open(tmp_path / "out.agmv.packed", "rb").read()
    assert len(b) > 1000 and int.from_bytes(b[4:8], "little") >= 1
    assert a == b, "the file from the YUV clip differs from the file of the XRGB32 clip it stands for (%d / %d bytes)" % (len(a), len(b))


@pytest.mark.parametrize("case", ENCODE, ids=[case_id(c) for c in ENCODE])
def test_encode_from_yuv_clip_equals_encode_of_the_clip_it_stands_for(case, tmp_path):
    fmt, which, schedule, opt = case[:4]
    if schedule == ADAPTIVE and which == "mixed":
        chain = chain_of(clips(which, fmt)[1], opt)
        assert chain.count(True) >= 2 and chain.count(False) >= 2, chain         # the adaptive chain takes both branches
    encode_both(tmp_path, case)


def test_encode_with_the_lz_stage_on_the_device(tmp_path):
    encode_both(tmp_path, ENCODE[0], {"AGMV_LZ_DEVICE": "1"})


@pytest.mark.parametrize("batch_env", [None, "8"], ids=["default-batches", "batches-of-8"])
def test_decode_into_yuv_sinks(batch_env, tmp_path):
    """agmv_splash.agmv (escape frames and stale tails: the state must come from the packed double buffer, not from the caller's
    bytes) into NV12 and I420 equals numpy's writing of the XRGB32 decode; with cap_frames below the file's count the frames
    behind the cap keep their 0xA5; with AGMV_BATCH_FRAMES=8 the batches cross GOPs"""
    path = os.path.join(GOLDEN, "agmv_splash.agmv")
    fmts = (NV12_601, I420_709F, I420_601, NV12_709F)
    jobs = [{"path": path, "fmt": 1, "out": "packed.npy"}] + [{"path": path, "fmt": f, "out": "f%d.npy" % f} for f in fmts]
    jobs += [{"path": path, "fmt": f, "cap": 11, "out": "cap%d.npy" % f} for f in fmts[:2]]
    res = run_child(tmp_path, {"batch": 0, "dec": jobs}, {"AGMV_BATCH_FRAMES": batch_env} if batch_env else None)["dec"]        # (0: the environment decides)
    gold = json.load(open(os.path.join(GOLDEN, "golden.json")))["agmv_splash"]
    n, w, h = res[0]["n"], res[0]["w"], res[0]["h"]
    assert (n, w, h) == (gold["n"], gold["w"], gold["h"]) and n > 11
    packed = np.load(tmp_path / "packed.npy").view(np.uint32).reshape(n, h, w)
    for r, job in zip(res[1:], jobs[1:]):
        f, cap = job["fmt"], job.get("cap", n)
        assert r["info_rc"] == 0 and r["rc"] == cap and r["fb"] == Y.frame_bytes(f, w, h)
        raw = np.load(tmp_path / job["out"]).reshape(n, r["fb"])
        exp = Y.from_packed(f, packed[:cap], w, h)
        bad = sorted(set(np.argwhere(raw[:cap] != exp)[:, 0]))
        assert not bad, "%s: frames %s differ from numpy's writing of the XRGB32 decode" % (job["out"], bad[:8])
        assert (raw[cap:] == 0xA5).all(), "frames behind cap_frames were written"


def test_seq_takes_and_returns_the_yuv_tensor_shapes(tmp_path):
    raw_nv12, packed_nv12 = clips("synth", NV12_601)
    raw_i420, packed_i420 = clips("synth", I420_709F)
    n, h, w = packed_nv12.shape
    np.save(tmp_path / "nv12.npy", raw_nv12.reshape(n, h * 3 // 2, w))
    np.save(tmp_path / "i420.npy", raw_i420.reshape(n, h * 3 // 2, w))
    res = run_child(tmp_path, {"batch": 8}, {"AGMV_BATCH_FRAMES": "8"}, SEQ_CHILD)
    assert res["refused"] == 1 and not os.path.exists(tmp_path / "none.agmv")
    frames = res["frames"]
    assert res["nv12"] == ["torch.uint8", [frames, h * 3 // 2, w]] and res["i420"] == ["torch.uint8", [frames, h * 3 // 2, w]]
    packed = np.load(tmp_path / "dec_packed.npy").view(np.uint32)
    assert packed.shape == (frames, h, w)
    assert (np.load(tmp_path / "dec_nv12.npy").reshape(frames, -1) == Y.from_packed(NV12_601, packed, w, h)).all()
    assert (np.load(tmp_path / "dec_i420.npy").reshape(frames, -1) == Y.from_packed(I420_709F, packed, w, h)).all()
    assert os.path.getsize(tmp_path / "nv12.agmv") > 1000 and os.path.getsize(tmp_path / "i420.agmv") > 1000
