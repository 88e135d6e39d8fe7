"""Writer sessions on whole files: libagmv_amd.Writer (AGMV_OpenWriterDev ... of include/agmv_writer.h) against the one-shot encode.

The reference of every comparison is the file libagmv_amd.encode_frames writes for the contiguous clip, made in the same child under
the same environment (which the file tests hold to the reference implementation); the writer's file must equal it byte for byte.
The clips are the seeded synthetic clip at 64 x 48 (128 x 96 for a target size, 240 x 160 for a GBA opt), 37 to 80 frames, in
other layouts by way of a decode of their file; AGMV_BATCH_FRAMES=8 makes a clip many batches, and the write sizes 1, 2, 5, 3, 8, 11,
7 cut GOPs and batches.  A child per test, which runs its cases one after the other (children as in tests/test_gpu_reader_files.py).
Needs an MI355X."""
import textwrap

import children as K
import numpy as np
import pytest

import memseq_cases as MC

pytestmark = pytest.mark.gpu

FULL, PDIFS = 1, 2
WRITES, ANALYSES = [1, 2, 5, 3, 8, 11, 7], [4, 9, 1, 6]
BATCH = 8
HEADER = 38                                                      # bytes of the header in front of its palettes

# job: clips {name: npy of an XRGB32 clip}, cases: [{kind, clip, n, fmt, layout_kw, enc, knobs, analyse, write, analyse_n, ring, reuse}].
# Answers one JSON line: per case a record.
CHILD = textwrap.dedent("""
    import json, os, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd as A
    clips = {}

    def base(name):
        if name not in clips:
            clips[name] = torch.from_numpy(np.load(job["clips"][name]).view(np.int32)).cuda()
        return clips[name]

    def layout(x, fmt, kw):
        if fmt == "xrgb32":
            return x
        A.encode_frames("layout.agmv", x, schedule=A.SCHEDULE_FULL)
        return A.decode_frames("layout.agmv", fmt=fmt, **kw)[0].contiguous()

    def size_of(x, fmt):
        s = tuple(x.shape)
        return (s[2], s[3]) if fmt in ("rgb8p", "f32", "f16", "bf16") else (s[1] * 2 // 3, s[2]) if fmt in ("nv12", "i420") else (s[1], s[2])

    def feed(call, x, sizes, upto, reuse):
        buf = torch.empty_like(x[:max(sizes)]) if reuse else None
        p, k = 0, 0
        while p < upto:
            n = min(sizes[k % len(sizes)], upto - p)
            if reuse:                                   # one buffer for every call, overwritten the moment the call returns
                buf[:n].copy_(x[p:p + n])
                call(buf[:n])
                buf.view(torch.uint8).fill_(0x5A)
                torch.cuda.synchronize()
            else:
                call(x[p:p + n])
            p, k = p + n, k + 1

    def tuples(kw):
        return {k: (tuple(v) if isinstance(v, list) else v) for k, v in kw.items()}

    def raised(call):
        try:
            call()
            return None
        except ValueError as e:
            return str(e)

    out = []
    for case in job["cases"]:
        fmt, n = case.get("fmt", "xrgb32"), case["n"]
        x = layout(base(case["clip"])[:n], fmt, tuples(case.get("layout_kw", {})))
        enc, knobs = dict(tuples(case["enc"]), fmt=fmt), case.get("knobs", {})
        h, w = size_of(x, fmt)
        for f in ("one.agmv", "two.agmv", "sample.agmv"):
            if os.path.exists(f):
                os.remove(f)
        kind, rec = case.get("kind", "same"), {}
        if kind == "same":
            A.encode_frames("one.agmv", x, **enc, **knobs)
            rec["one_stats"] = A.stabilise_stats()
            wr = A.Writer("two.agmv", h, w, ring_frames=case.get("ring"), **enc, **knobs)
            feed(wr.analyse, x, case["analyse"], case.get("analyse_n", n), False)
            feed(wr.write, x, case["write"], n, case.get("reuse", False))
            rec["stats"] = wr.stats()
            rec["written"] = wr.close()
            rec["two_stats"] = A.stabilise_stats()
            one, two = open("one.agmv", "rb").read(), open("two.agmv", "rb").read()
            rec.update(same=one == two, head=[list(one[4:8]), list(two[4:8]), list(one[18:22]), list(two[18:22])], bytes=[len(one), len(two)])
            if case.get("analyse_n"):                   # a sample's palette: the header's palette bytes are the one-shot call's for the sample
                A.encode_frames("sample.agmv", x[:case["analyse_n"]].contiguous(), **enc, **knobs)
                pals = 768 * (2 if enc.get("opt", 3) in (1, 3, 5, 7, 8) else 1)
                sample = open("sample.agmv", "rb").read()[@HEADER@:@HEADER@ + pals]
                pal = np.frombuffer(two[@HEADER@:@HEADER@ + pals], np.uint8).reshape(-1, 3).astype(np.int64)
                colours = torch.from_numpy(np.unique(pal[:, 0] << 16 | pal[:, 1] << 8 | pal[:, 2])).cuda()
                frames, info = A.decode_frames("two.agmv")
                rec.update(palette=two[@HEADER@:@HEADER@ + pals] == sample and len(sample) == pals, decoded=int(frames.shape[0]), frames=int(info.number_of_frames),
                           in_palette=bool(torch.isin(frames.to(torch.int64), colours).all()))
        elif kind == "too_few":                         # fewer written frames than the first group reads: -2 and no file
            wr = A.Writer("two.agmv", h, w, **enc)
            wr.analyse(x)
            if case["write_n"]:
                wr.write(x[:case["write_n"]])
            rec["exists_before"] = os.path.exists("two.agmv")
            rec["raised"] = raised(wr.close)
            rec["exists"] = os.path.exists("two.agmv")
            rec["one_shot"] = raised(lambda: A.encode_frames("one.agmv", x[:max(case["write_n"], 1)].contiguous(), **enc)) if case["write_n"] else None
        elif kind == "order":                           # the calls out of order, of nothing and on a closed writer
            wr = A.Writer("two.agmv", h, w, **enc)
            L, hd = wr._L, wr._h
            rec["write_first"] = [raised(lambda: wr.write(x[:4])), L.AGMV_WriterWriteDev(hd, x.data_ptr(), 4)]
            rec["nothing"] = [L.AGMV_WriterAnalyseDev(hd, None, 0), L.AGMV_WriterWriteDev(hd, None, 0), L.AGMV_WriterAnalyseDev(hd, None, 3)]
            rec["untouched"] = wr.stats()
            wr.analyse(x)
            rec["null_write"] = L.AGMV_WriterWriteDev(hd, None, 3)
            wr.write(x[:5])
            rec["analyse_late"] = [raised(lambda: wr.analyse(x[:4])), L.AGMV_WriterAnalyseDev(hd, x.data_ptr(), 4)]
            rec["wrong_size"] = raised(lambda: wr.write(x[:, :-4].contiguous()))
            wr.write(x[5:])
            rec["written"] = wr.close()
            rec["closed"] = [raised(lambda: wr.write(x[:1])), raised(lambda: wr.analyse(x[:1])), raised(wr.stats), wr.close()]
            A.encode_frames("one.agmv", x, **enc)
            rec["same"] = open("one.agmv", "rb").read() == open("two.agmv", "rb").read()
            with A.Writer("two.agmv", h, w, **enc) as wr:  # ... and the with block closes
                wr.analyse(x)
                wr.write(x)
            rec["with_same"] = open("one.agmv", "rb").read() == open("two.agmv", "rb").read()
        out.append(rec)
    print(json.dumps({"cases": out}))
""").replace("@HEADER@", str(HEADER))

ENVS = {"host": {}, "lzss_device": {"AGMV_LZ_DEVICE": "1"}, "lz77_device": {"AGMV_LZ77_DEVICE": "1"}}


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("writer_clips")
    made = {}
    for name, (w, h, t) in {"64x48": (64, 48, 80), "128x96": (128, 96, 37), "240x160": (240, 160, 37)}.items():
        made[name] = str(d / (name + ".npy"))
        np.save(made[name], MC.synth_clip(w, h, t))
    return made


def run_child(cwd, clips, cases, env=None):
    env = dict({"AGMV_BATCH_FRAMES": str(BATCH), "AGMV_LZ_DEVICE": None, "AGMV_LZ77_DEVICE": None, "AGMV_PALETTE_REFINE": None, "AGMV_DITHER": None,
                "AGMV_STABILISE": None}, **(env or {}))
    recs = K.run_child(cwd, CHILD, {"clips": clips, "cases": cases}, env, prelude="")["cases"]
    assert len(recs) == len(cases)
    return recs


def case(n=37, clip="64x48", schedule=FULL, opt=3, compression=1, **kw):
    enc = dict(dict(opt=opt, quality=3, compression=compression, schedule=schedule, fps=24), **kw.pop("enc", {}))
    return dict(dict(clip=clip, n=n, enc=enc, analyse=ANALYSES, write=WRITES), **kw)


def same(recs, cases):
    for c, r in zip(cases, recs):
        assert r["same"], (c, r)


@pytest.mark.parametrize("env", sorted(ENVS))
def test_full_in_pieces_is_the_one_shot_file(tmp_path, clips, env):
    """37 frames: 5 batches of 8, write sizes that cut GOPs and batches, analyse sizes that differ from them; 512- and 256-colour palettes,
    LZSS and LZ77, the LZ stage on the host and (each in a process of its own) on the GPU"""
    compressions = {"host": (1, 2), "lzss_device": (1,), "lz77_device": (2,)}[env]
    cases = [case(opt=opt, compression=c) for opt in (1, 2, 3) for c in compressions]
    recs = run_child(tmp_path, clips, cases, ENVS[env])
    same(recs, cases)
    for r in recs:
        st = r["stats"]
        assert r["written"] == 37 and st["analysed"] == st["taken"] == 37 and st["writes"] == len(WRITES) and st["batches"] == 37 // BATCH, r      # (statistics from before the close, which hands over the last, short batch)
        assert st["ring_frames"] == 4 * BATCH and st["written"] <= 37, r


def test_each_layout_once(tmp_path, clips):
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    norm = dict(mean=mean, std=std)
    cases = [case(fmt="rgb24"), case(fmt="rgb8p", opt=2), case(fmt="nv12", compression=2), case(fmt="i420", layout_kw=dict(yuv="bt709", full_range=True),
                                                                                                   enc=dict(yuv="bt709", full_range=True)),
             case(fmt="f16", layout_kw=norm, enc=norm), case(clip="128x96", enc=dict(size=[48, 64], scale="area")),
             case(clip="128x96", fmt="nv12", enc=dict(size=[48, 64], scale="nearest")), case(clip="240x160", opt=5), case(clip="240x160", opt=7, fmt="nv12"),
             case(clip="240x160", opt=6, fmt="f32", layout_kw=norm, enc=norm, compression=2)]
    recs = run_child(tmp_path, clips, cases)
    same(recs, cases)
    assert all(r["written"] == 37 for r in recs), recs


def test_stabilise_dither_and_refinement_see_the_one_shot_batches(tmp_path, clips):
    knobs = dict(stabilise=8, dither=6, palette_refine=4)
    cases = [case(n=45, knobs=knobs), case(n=45, opt=2, compression=2, knobs=knobs), case(n=42, schedule=PDIFS, knobs=knobs)]
    recs = run_child(tmp_path, clips, cases)
    same(recs, cases)
    for r in recs:
        assert r["one_stats"] == r["two_stats"] and r["one_stats"][0] > 0, r


@pytest.mark.parametrize("opt,compression,first", [(3, 1, 41), (1, 2, 42)], ids=["light", "heavy"])
def test_pdifs_without_the_clips_end(tmp_path, clips, opt, compression, first):
    """six consecutive lengths around group boundaries (groups start every 4 frames for a light opt, every 2 for a heavy one, and the last
    ones depend on the 5 frames behind them): the chunks, the patched frame count at offset 4 and the patched rate at offset 18"""
    cases = [case(n=n, schedule=PDIFS, opt=opt, compression=compression) for n in range(first, first + 6)]
    recs = run_child(tmp_path, clips, cases)
    same(recs, cases)
    heavy = opt == 1
    for c, r in zip(cases, recs):
        n = c["n"]
        groups = 1 + (n - 6) // (2 if heavy else 4)
        assert r["written"] == (groups if heavy else 3 * groups) and r["head"][0] == r["head"][1] and r["head"][2] == r["head"][3], (n, r)
        assert int.from_bytes(bytes(r["head"][1]), "little") == r["written"], (n, r)
        assert r["stats"]["taken"] == n and r["stats"]["batches"] == r["written"] // BATCH, (n, r)      # (before the close)
    assert len({r["written"] for r in recs}) > 1                 # (the lengths do cross a boundary)


def test_one_buffer_reused_for_every_write(tmp_path, clips):
    cases = [case(reuse=True), case(n=43, schedule=PDIFS, opt=1, reuse=True), case(fmt="nv12", reuse=True)]
    same(run_child(tmp_path, clips, cases), cases)


def test_ring_pressure(tmp_path, clips):
    """the smallest ring -- a request of 1 is raised to it: one batch's sources, and for PDIFS two per frame and the hold-back of 6 -- under one
    write of a clip at least three times as long"""
    cases = [case(n=40, ring=1, write=[40]), case(n=41, ring=1, write=[41], compression=2), case(n=80, ring=1, write=[80], schedule=PDIFS),
             case(n=80, ring=1, write=[80], schedule=PDIFS, opt=1, compression=2), case(n=45, ring=13, write=[45])]
    recs = run_child(tmp_path, clips, cases)
    same(recs, cases)
    for c, r, ring in zip(cases, recs, (BATCH, BATCH, 2 * BATCH + 6, 2 * BATCH + 6, 13)):
        assert r["stats"]["ring_frames"] == ring and r["stats"]["waits"] > 0 and r["stats"]["writes"] == 1 and c["n"] >= 3 * ring, (c, r)


def test_a_samples_palette(tmp_path, clips):
    """analyse the first 8 frames, write all 40: a valid file with the one-shot call's palette of the 8"""
    cases = [case(n=40, analyse_n=8), case(n=40, analyse_n=8, opt=2, compression=2)]
    recs = run_child(tmp_path, clips, cases)
    for r in recs:
        assert r["palette"] and r["decoded"] == r["frames"] == r["written"] == 40 and r["in_palette"], r
        assert r["stats"]["analysed"] == 8 and r["stats"]["taken"] == 40, r


def test_a_close_with_too_few_frames_leaves_no_file(tmp_path, clips):
    cases = [case(n=8, kind="too_few", write_n=0), case(n=8, kind="too_few", write_n=3, schedule=PDIFS), case(n=8, kind="too_few", write_n=1, schedule=PDIFS, opt=1)]
    recs = run_child(tmp_path, clips, cases)
    for c, r in zip(cases, recs):
        assert r["raised"] and "(-2)" in r["raised"] and not r["exists"] and r["exists_before"] == bool(c["write_n"]), (c, r)
        assert not c["write_n"] or "(-2)" in r["one_shot"], (c, r)             # the one-shot call's code for that many frames


def test_calls_out_of_order_of_nothing_and_on_a_closed_writer(tmp_path, clips):
    r = run_child(tmp_path, clips, [case(n=21, kind="order")])[0]
    assert "no palette" in r["write_first"][0] and r["write_first"][1] == -6 and r["nothing"] == [0, 0, -1] and r["null_write"] == -1, r
    assert all(v == 0 for k, v in r["untouched"].items() if k != "ring_frames"), r
    assert "frozen" in r["analyse_late"][0] and r["analyse_late"][1] == -6 and "takes frames of 64x48" in r["wrong_size"], r
    assert r["written"] == 21 and r["same"] and r["with_same"], r
    assert all(m and "closed" in m for m in r["closed"][:3]) and r["closed"][3] is None, r
