"""Whole files from and to normalised float tensors: AGMV_EncodeFramesTensorDev / AGMV_DecodeFramesTensorDev of
libagmv_amd/libagmv.so through libagmv_amd.encode_frames(mean=, std=) and decode_frames(fmt="f16" | "f32" | "bf16", mean=, std=,
size=, scale=) on torch tensors.

Encode: a tensor clip of model-like values (the canonical 64 x 48 clip normalised, with noise that crosses the rounding ties and
the clamp) must give, byte for byte, the file that encode_frames writes for the XRGB32 clip the reading rule gives in numpy
(tests/tensor_cases.py).  Decode: the tensor must be the table applied to what decode_frames(fmt="rgb8p") delivers, scaled in
numpy first where a size is given (tests/upscale_cases.py); a decode without the new arguments is what it was.  The library rounds
AGMV_BATCH_FRAMES=3 up to whole GOPs of 4, so the 8-frame clip takes two batches and the table uploaded once per call serves both.
Child processes as in tests/test_gpu_upscale_files.py (the drivers keep process-wide state).  Needs an MI355X."""
import textwrap

import children as K
import numpy as np
import pytest

import memseq_cases as MC
import tensor_cases as TC
import upscale_cases as U

pytestmark = pytest.mark.gpu

W, H0, T = 64, 48, 8
FULL, PDIFS = 1, 2

# job: enc: [{bits (npy of the tensor's bit patterns), type, mean, std, packed (npy of the XRGB32 clip), opt, schedule, compression, named}],
# dec: [{path, fmt, mean, std, size, scale, out}].  Answers one JSON line.
CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    DT = {"f32": (np.int32, torch.float32), "f16": (np.int16, torch.float16), "bf16": (np.int16, torch.bfloat16)}
    res = {"enc": [], "dec": []}
    for k, e in enumerate(job.get("enc", [])):
        store, dtype = DT[e["type"]]
        x = torch.from_numpy(np.load(e["bits"]).view(store)).cuda().view(dtype)
        kw = dict(opt=e["opt"], schedule=e["schedule"], compression=e["compression"], quality=e["quality"])
        libagmv_amd.encode_frames("t%d.agmv" % k, x, mean=e["mean"], std=e["std"], fmt=e["type"] if e["named"] else None, **kw)
        libagmv_amd.encode_frames("p%d.agmv" % k, torch.from_numpy(np.load(e["packed"]).view(np.int32)).cuda(), **kw)
        a, b = open("t%d.agmv" % k, "rb").read(), open("p%d.agmv" % k, "rb").read()
        res["enc"].append({"same": a == b, "len": len(a)})
    if job.get("dec"):
        path = job["path"]
        before, info = libagmv_amd.decode_frames(path)
        planes, _ = libagmv_amd.decode_frames(path, fmt="rgb8p")
        np.save("planes.npy", planes.cpu().numpy())
        for d in job["dec"]:
            got, info2 = libagmv_amd.decode_frames(path, fmt=d["fmt"], mean=d["mean"], std=d["std"], size=d["size"] and tuple(d["size"]), scale=d["scale"])
            assert (info2.width, info2.height) == (info.width, info.height) and got.dtype == DT[d["fmt"]][1] and got.is_contiguous()
            np.save(d["out"], got.view(torch.int32 if d["fmt"] == "f32" else torch.int16).cpu().numpy())
            res["dec"].append(list(got.shape))
        after, _ = libagmv_amd.decode_frames(path)
        res["same"] = bool((before == after).all())
        res["packed_is_planes"] = bool((before == (planes[:, 0].int() << 16 | planes[:, 1].int() << 8 | planes[:, 2].int())).all())
        res["frames"] = int(info.number_of_frames)
    print(json.dumps(res))
""")


def run_child(cwd, job, env=None):
    import torch  # noqa: F401  (torch's HIP runtime first, should this be the process's first use of the libraries)
    return K.run_child(cwd, CHILD, job, dict(dict.fromkeys(("AGMV_BATCH_FRAMES", "AGMV_LZ_DECODE_DEVICE", "AGMV_DITHER", "AGMV_PALETTE_REFINE")), **(env or {})),
                       prelude="")


def model_output(t, pix, mean, std, seed):
    """the clip normalised in float32 with noise of about one byte, so that ties, both clamps and values no table holds occur;
    a few elements are NaN and infinities.  -> bit patterns [n, 3, h, w]"""
    rng = np.random.default_rng(seed)
    ch = np.stack([(pix >> 16) & 255, (pix >> 8) & 255, pix & 255], axis=1).astype(np.float32)
    x = ch / np.float32(255) + rng.normal(0, 1.0 / 255, ch.shape).astype(np.float32)
    x = (x - TC.f32(mean)[None, :, None, None]) / TC.f32(std)[None, :, None, None]
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, 24)] = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0], np.float32).repeat(4)
    return TC.narrow(t, x)


# type, normalisation, opt (2: 256 colours, 3 and 1: 512), schedule, named (fmt= given, or inferred from the dtype)
ENCODES = [(TC.F16, "imagenet", 3, PDIFS, False), (TC.F32, "identity", 2, FULL, True), (TC.BF16, "half", 1, PDIFS, True), (TC.F32, "imagenet", 3, FULL, False)]


def test_the_file_of_a_tensor_clip_is_the_file_of_the_clip_it_stands_for(tmp_path):
    pix = MC.synth_clip(W, H0, T)
    jobs = []
    for k, (t, norm, opt, schedule, named) in enumerate(ENCODES):
        mean, std = TC.NORMS[norm]
        bits = model_output(t, pix, mean, std, 60 + k)
        packed = TC.to_packed(t, bits, mean, std)
        red = np.abs(((packed >> 16) & 255).astype(np.int64) - ((pix >> 16) & 255).astype(np.int64))
        assert (packed != pix).mean() > 0.2 and red.mean() < 2                                     # the noise moved bytes, and the clip is still the clip
        np.save(tmp_path / ("bits%d.npy" % k), bits)
        np.save(tmp_path / ("packed%d.npy" % k), packed)
        jobs.append({"bits": "bits%d.npy" % k, "packed": "packed%d.npy" % k, "type": TC.NAMES[t], "mean": list(mean), "std": list(std), "opt": opt,
                     "schedule": schedule, "compression": 1, "quality": 3, "named": named})
    res = run_child(tmp_path, {"enc": jobs}, {"AGMV_BATCH_FRAMES": "3"})
    assert [r["same"] for r in res["enc"]] == [True] * len(ENCODES), res
    assert all(r["len"] > 1000 for r in res["enc"])
    assert len({open(tmp_path / ("t%d.agmv" % k), "rb").read() for k in range(len(ENCODES))}) == len(ENCODES)


def dec(fmt, norm, size=None, scale="bilinear"):
    mean, std = TC.NORMS[norm]
    return {"fmt": fmt, "mean": list(mean), "std": list(std), "size": size and list(size), "scale": scale, "norm": norm,
            "out": "%s_%s_%s_%s.npy" % (fmt, norm, scale, "x".join(map(str, size or ())))}


# (h, w): 40 x 56 takes the element path (56 is no multiple of 16), 24 x 32 the box filter's batch of D, 96 x 128 the 16-byte stores
DECODES = [dec("f16", "imagenet"), dec("f16", "imagenet", (40, 56), "bilinear"), dec("f16", "imagenet", (24, 32), "area"), dec("f32", "half", (96, 128), "nearest"),
           dec("bf16", "identity"), dec("f32", "bytes", (48, 64), "bilinear")]


def test_the_decoded_tensor_is_the_table_applied_to_the_decoded_planes(tmp_path):
    """mean= and std= as three numbers; the last job scales to the file's own size, which is the identity"""
    pix = MC.synth_clip(W, H0, T)
    np.save(tmp_path / "packed.npy", pix)
    np.save(tmp_path / "bits.npy", TC.from_packed(TC.table(TC.F32, *TC.NORMS["identity"]), pix))    # the same clip as a tensor: t0.agmv = p0.agmv
    enc = {"bits": "bits.npy", "packed": "packed.npy", "type": "f32", "mean": [0, 0, 0], "std": [1, 1, 1], "opt": 3, "schedule": FULL, "compression": 1,
           "quality": 3, "named": True}
    res = run_child(tmp_path, {"enc": [enc], "path": "t0.agmv", "dec": DECODES}, {"AGMV_BATCH_FRAMES": "3"})
    assert res["enc"][0]["same"]
    assert res["frames"] == T and res["same"] and res["packed_is_planes"]
    planes = np.load(tmp_path / "planes.npy").astype(np.uint32)
    native = planes[:, 0] << 16 | planes[:, 1] << 8 | planes[:, 2]
    assert native.shape == (T, H0, W) and len(np.unique(native.reshape(T, -1), axis=0)) == T       # every frame its own content
    for d, shape in zip(DECODES, res["dec"]):
        t = {v: k for k, v in TC.NAMES.items()}[d["fmt"]]
        h, w = d["size"] or (H0, W)
        assert shape == [T, 3, h, w], d
        clip = native if d["size"] is None else U.scale({"nearest": U.NEAREST, "area": U.AREA, "bilinear": U.BILINEAR}[d["scale"]], native, w, h)
        exp = TC.from_packed(TC.table(t, *TC.NORMS[d["norm"]]), clip)
        got = np.load(tmp_path / d["out"]).view(TC.BITS[t])
        assert got.shape == exp.shape and (got == exp).all(), (d, np.argwhere(got != exp)[:4])
    ident = np.load(tmp_path / DECODES[-1]["out"]).view(np.uint32)
    assert (ident == TC.from_packed(TC.table(TC.F32, *TC.NORMS["bytes"]), native)).all()
    assert np.abs(TC.widen(TC.F32, ident) - np.stack([planes[:, 0], planes[:, 1], planes[:, 2]], axis=1)).max() < 1e-4      # 0 / (1/255): the bytes, to float32's 1 / 255
