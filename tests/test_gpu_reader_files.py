"""Reader sessions on whole files: libagmv_amd.Reader (AGMV_OpenReaderDev ... of include/agmv_reader.h) against the one-shot decode.

The comparator is never the reader's own output: every read of n frames at position p must equal frames p, p + step, ... of
libagmv_amd.decode_frames(path, <the same sink arguments>) of the same file, decoded in the same child by the path without a reader
(which the file tests hold to the reference); the comparison runs on the device, and the parent asserts its verdicts and the
reader's statistics, which show what ran: how many frames went through the LZ stage and the GPU stage, which checkpoint a seek
started from, whether a read was run again from frame 0.  Every read gets a destination of its own, and the one before is poisoned
and dropped: the reader may hold nothing of the caller's.  The clip is the 24 frames of 64 x 48 of tests/test_gpu_view_files.py;
AGMV_BATCH_FRAMES=8 and 4 make reads cross batches.  lz_cap of that clip is 64 * 48 * 33 / 16 + 4096 bytes.  Child processes as in
tests/test_gpu_view_files.py.  Needs an MI355X."""
import textwrap

import children as K
import numpy as np
import pytest

import damage_cases as D
import memseq_cases as MC

pytestmark = pytest.mark.gpu

W, H0, T = 64, 48, 24
LZ_CAP = W * H0 * 33 // 16 + 4096

# job: clip (npy of the XRGB32 clip to encode, or none), compression, opt, craft ([a, b]: chunk a replaced by the bytes of chunk b), path,
# ops: [[reader, "open", path or none, kw], [reader, "read", n], [reader, "seek", f], [reader, "close"], [reader, "read_closed"],
# ["-", "decode", path or none, kw], ["-", "encode", path, {opt, compression}] (the job's clip)].  Answers one JSON line: per op a record.
CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    path = job.get("path")
    if job.get("clip"):
        libagmv_amd.encode_frames(path, torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda(), schedule=libagmv_amd.SCHEDULE_FULL,
                                  compression=job.get("compression", 1), opt=job.get("opt", 3))
    if job.get("craft"):
        data, at = open(path, "rb").read(), []
        p = data.find(b"AGFC")
        while p >= 0:
            at.append(p)
            p = data.find(b"AGFC", p + 16 + int.from_bytes(data[p + 12:p + 16], "little"))
        at.append(len(data))
        a, b = job["craft"]
        path = "crafted.agmv"
        open(path, "wb").write(data[:at[a]] + data[at[b]:at[b + 1]] + data[at[a + 1]:])

    def sink(kw):
        k = {n: (tuple(v) if isinstance(v, list) else v) for n, v in kw.items() if n not in ("step", "index_bytes")}
        return k

    fulls, readers, out = {}, {}, []

    def full_of(p, kw):
        key = json.dumps([p, sink(kw)], sort_keys=True)
        if key not in fulls:
            fulls[key] = libagmv_amd.decode_frames(p, **sink(kw))[0]
        return fulls[key]

    for op in job["ops"]:
        name, what, rec = op[0], op[1], {}
        if what == "open":
            p, kw = op[2] or path, op[3]
            full = full_of(p, kw)
            r = libagmv_amd.Reader(p, **{n: (tuple(v) if isinstance(v, list) else v) for n, v in kw.items()})
            readers[name] = {"r": r, "full": full, "step": kw.get("step", 1), "prev": None}
            rec = {"len": len(r), "full": int(full.shape[0]), "tell": r.tell(), "stats": r.stats(), "frames": int(r.info.number_of_frames)}
        elif what == "read":
            s = readers[name]
            r, p = s["r"], s["r"].tell()
            want = s["full"][p::s["step"]][:op[2]]
            got = r.read(op[2])
            same = got.shape == want.shape and got.dtype == want.dtype and bool((got.view(torch.uint8) == want.contiguous().view(torch.uint8)).all())
            rec = {"ok": same, "n": int(got.shape[0]), "want": int(want.shape[0]), "at": p, "tell": r.tell(), "stats": r.stats()}
            if s["prev"] is not None:
                s["prev"].view(torch.uint8).fill_(0xA5)
                torch.cuda.synchronize()
            s["prev"] = got
        elif what == "seek":
            readers[name]["r"].seek(op[2])
            rec = {"tell": readers[name]["r"].tell(), "stats": readers[name]["r"].stats()}
        elif what == "close":
            readers[name]["r"].close()
        elif what == "read_closed":
            r = readers[name]["r"]
            for call in (lambda: r.read(1), lambda: r.tell(), lambda: r.seek(0), lambda: r.stats(), lambda: list(r.batches(2))):
                try:
                    call()
                    rec.setdefault("raised", []).append(None)
                except ValueError as e:
                    rec.setdefault("raised", []).append(str(e))
            r.close()
        elif what == "encode":
            libagmv_amd.encode_frames(op[2], torch.from_numpy(np.load(job["clip_npy"]).view(np.int32)).cuda(), schedule=libagmv_amd.SCHEDULE_FULL, **op[3])
        elif what == "decode":
            p, kw = op[2] or path, op[3]
            got = libagmv_amd.decode_frames(p, **sink(kw))[0]
            want = full_of(p, kw)
            L = libagmv_amd.seq.load_library()
            vs = libagmv_amd.abi.AGMV_VIEW_STATS()
            L.AGMV_GetViewStats(vs)
            rec = {"ok": got.shape == want.shape and bool((got.view(torch.uint8) == want.view(torch.uint8)).all()), "deblock": libagmv_amd.deblock_stats(),
                   "view": [vs.lz_frames, vs.gpu_frames, vs.delivered, vs.restarts]}
        out.append(rec)
    print(json.dumps({"ops": out}))
""")


def run_child(cwd, job, env=None):
    return K.run_child(cwd, CHILD, job, dict({"AGMV_BATCH_FRAMES": "8", "AGMV_LZ_DECODE_DEVICE": None}, **(env or {})), prelude="")["ops"]


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    p = tmp_path_factory.mktemp("reader_clip") / "clip.npy"
    np.save(p, MC.synth_clip(W, H0, T))
    return str(p)


def reads_ok(recs, what=""):
    for k, r in enumerate(recs):
        if "ok" in r:
            assert r["ok"] and r.get("n") == r.get("want"), (what, k, r)             # (a one-shot decode's record has neither)


def sequential(sizes, kw=None, name="r"):
    """the ops of one reader that walks the file in reads of each of `sizes`, a reader per size, one after the other"""
    ops = []
    for k, n in enumerate(sizes):
        r = "%s%d" % (name, k)
        ops += [[r, "open", None, kw or {}]] + [[r, "read", n]] * (T // n + 2) + [[r, "close"]]
    return ops


LZ = {"host": None, "device": {"AGMV_LZ_DECODE_DEVICE": "1"}}


@pytest.mark.parametrize("lz", sorted(LZ))
@pytest.mark.parametrize("compression", [1, 2], ids=["lzss", "lz77"])
@pytest.mark.parametrize("opt", [1, 2, 3])
def test_sequential_reads_of_any_size_send_every_frame_through_each_stage_once(tmp_path, clip, opt, compression, lz):
    sizes = (1, 3, 5, 8, 9, 25)
    ops = sequential(sizes)
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "opt": opt, "compression": compression, "ops": ops}, LZ[lz])
    reads_ok(recs, (opt, compression, lz))
    at = 0
    for n in sizes:
        mine = recs[at:at + T // n + 4]
        at += len(mine)
        assert mine[0]["len"] == mine[0]["full"] == T and mine[0]["tell"] == 0 and mine[0]["stats"]["lz_frames"] == 0
        reads = mine[1:-1]
        assert [r["n"] for r in reads] == [min(n, T - k * n) if k * n < T else 0 for k in range(len(reads))]
        assert [r["tell"] for r in reads] == [min((k + 1) * n, T) for k in range(len(reads))]
        st = reads[-1]["stats"]
        assert st["lz_frames"] == st["gpu_frames"] == st["delivered"] == T and st["restarts"] == 0 and st["seeks"] == 0, (n, st)
        assert st["reads"] == sum(1 for r in reads if r["n"]) and st["interval"] == 4 and st["checkpoints"] == 5, (n, st)
        for k, r in enumerate(reads):                             # ... and never more than the read needed: no frame runs ahead into the statistics
            assert r["stats"]["lz_frames"] == r["stats"]["gpu_frames"] == r["tell"], (n, k, r)


def test_batches_of_four(tmp_path, clip):
    ops = sequential((3, 5, 9, 25))
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "ops": ops}, {"AGMV_BATCH_FRAMES": "4"})
    reads_ok(recs)
    finals = [recs[k - 1]["stats"] for k, op in enumerate(ops) if op[1] == "close"]
    assert len(finals) == 4 and all(st["lz_frames"] == st["gpu_frames"] == st["delivered"] == T and st["restarts"] == 0 for st in finals), finals


SINKS = [dict(fmt="rgb24"), dict(fmt="nv12", size=[30, 40], scale="bilinear"), dict(fmt="nv12", yuv="bt709", full_range=True, size=[24, 32], scale="area"),
         dict(fmt="i420", size=[14, 20], scale="area", crop=[4, 4, 30, 40]), dict(fmt="f16", mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]),
         dict(fmt="bf16", size=[28, 20], crop=[8, 12, 20, 28], step=3), dict(fmt="rgb8p", crop=[3, 5, 14, 20], step=3), dict(fmt="xrgb32", crop=[3, 1, 7, 5], step=2),
         dict(fmt="xrgb32", deblock=16), dict(fmt="rgb24", deblock=16, step=2, crop=[4, 8, 12, 16])]


def test_every_sink_reads_what_the_one_shot_decode_of_that_sink_gives(tmp_path, clip):
    ops = []
    for k, kw in enumerate(SINKS):
        r = "s%d" % k
        ops += [[r, "open", None, kw]] + [[r, "read", 5]] * 6 + [[r, "close"]]
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "ops": ops})
    reads_ok(recs)
    for k, kw in enumerate(SINKS):
        mine, step = recs[8 * k:8 * k + 8], kw.get("step", 1)
        assert sum(r["n"] for r in mine[1:7]) == len(range(0, T, step)), (kw, mine)
        st = mine[6]["stats"]
        last = (len(range(0, T, step)) - 1) * step
        assert st["lz_frames"] == st["gpu_frames"] == last + 1 and st["restarts"] == 0, (kw, st)     # the stride skips no frame of either stage


def seek_ops(index_bytes):
    kw = {"index_bytes": index_bytes}
    ops = [["a", "open", None, kw], ["a", "seek", 13], ["a", "read", 6], ["a", "close"],                   # 0 .. 3
           ["b", "open", None, kw]] + [["b", "read", 7]] * 4                                               # 4 .. 8: a full pass
    for f in (0, 5, 12, 20):                                                                               # 9 ..: backward seeks, 3 frames each
        ops += [["b", "seek", f], ["b", "read", 3]]
    ops += [["b", "seek", 11], ["b", "seek", 11], ["b", "read", 2],                                        # 17 .. 19: a seek to where the reader stands
            ["b", "seek", 24], ["b", "read", 4], ["b", "seek", 1000], ["b", "read", 4], ["b", "seek", 2], ["b", "read", 1], ["b", "close"]]
    return ops


@pytest.mark.parametrize("lz", sorted(LZ))
def test_seeks_start_the_lz_stage_at_the_nearest_checkpoint(tmp_path, clip, lz):
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "ops": seek_ops(6 * LZ_CAP)}, LZ[lz])
    reads_ok(recs)
    a = recs[2]
    assert (a["at"], a["n"], a["tell"]) == (13, 6, 19)
    assert a["stats"]["lz_frames"] == 19 and a["stats"]["gpu_frames"] == 7 and a["stats"]["restarts"] == 0 and a["stats"]["seeks"] == 1       # LZ 0 .. 18, GPU 12 .. 18
    st = recs[8]["stats"]
    assert st["lz_frames"] == st["gpu_frames"] == T and st["interval"] == 4 and st["checkpoints"] == 5
    lz_frames, gpu_frames = T, T
    for k, f in enumerate((0, 5, 12, 20)):
        seek, read = recs[9 + 2 * k], recs[10 + 2 * k]
        assert seek["tell"] == f and seek["stats"]["lz_frames"] == lz_frames               # (the work is the next read's)
        c = f & ~3                                                                         # every checkpoint is recorded: the one at g0
        lz_frames, gpu_frames = lz_frames + f + 3 - c, gpu_frames + f + 3 - c
        assert read["at"] == f and read["n"] == 3 and read["tell"] == f + 3
        assert read["stats"]["lz_frames"] == lz_frames and read["stats"]["gpu_frames"] == gpu_frames and read["stats"]["restarts"] == 0, (f, read)
    first, second, read = recs[17:20]
    assert first["stats"]["seeks"] == 5 and second["stats"]["seeks"] == 6 and second["tell"] == 11
    assert {k: v for k, v in second["stats"].items() if k != "seeks"} == {k: v for k, v in first["stats"].items() if k != "seeks"}
    assert read["stats"]["lz_frames"] == lz_frames + 11 + 2 - 8
    for k in (21, 23):
        assert recs[k]["n"] == 0 and recs[k]["stats"]["lz_frames"] == read["stats"]["lz_frames"], recs[k]
    assert recs[20]["tell"] == 24 and recs[22]["tell"] == 1000 and recs[23]["tell"] == 1000
    assert recs[25]["n"] == 1 and recs[25]["at"] == 2 and recs[25]["stats"]["checkpoints"] == 5


def test_an_index_of_one_buffer_starts_the_lz_stage_at_frame_0(tmp_path, clip):
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "ops": seek_ops(LZ_CAP)})
    reads_ok(recs)
    st = recs[8]["stats"]
    assert st["interval"] == 24 and st["checkpoints"] == 0 and st["lz_frames"] == T
    lz_frames = T
    for k, f in enumerate((0, 5, 12, 20)):
        lz_frames += f + 3
        assert recs[10 + 2 * k]["stats"]["lz_frames"] == lz_frames, (f, recs[10 + 2 * k])
    assert recs[16]["stats"]["gpu_frames"] == T + 3 + 4 + 3 + 3                          # the GPU stage still starts at the GOP


@pytest.mark.parametrize("lz", sorted(LZ))
def test_a_gop_that_depends_on_the_frames_before_it_is_read_again_from_frame_0(tmp_path, clip, lz):
    """chunk 16 replaced by the bytes of chunk 17: a P-frame's stream, COPY blocks included, stands where an I-frame is read (the craft of
    tests/test_gpu_view_files.py), so GOP 4 decoded from the fresh state is not the file's decode.  A read that runs INTO that GOP from
    a seek to 13 carries the decoder's state and needs no restart; a seek to 17 starts the GPU stage at 16 and must be run again."""
    ops = [["a", "open", None, {}], ["a", "seek", 13], ["a", "read", 6], ["a", "close"],
           ["b", "open", None, {}], ["b", "seek", 17], ["b", "read", 4], ["b", "read", 9], ["b", "seek", 18], ["b", "read", 2], ["b", "close"],
           ["-", "decode", None, {"frames": [17, 21, 1]}]]
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "craft": [16, 17], "ops": ops}, LZ[lz])
    reads_ok(recs)
    assert recs[11]["view"][3] == 1, "premise: the one-shot view from frame 17 of the crafted file restarts"
    assert recs[2]["n"] == 6 and recs[2]["stats"]["restarts"] == 0 and recs[2]["stats"]["gpu_frames"] == 7
    b = recs[6]
    assert b["n"] == 4 and b["stats"]["restarts"] == 1 and b["tell"] == 21
    assert b["stats"]["gpu_frames"] >= 21 and b["stats"]["lz_frames"] >= 21 + 21          # the run given up, then frames 0 .. 20 through both stages
    assert recs[7]["n"] == 3 and recs[7]["stats"]["restarts"] == 1                        # ... and on from there, sequentially
    assert recs[9]["n"] == 2 and recs[9]["stats"]["restarts"] == 2


DAMAGED = ("cut_normal_m512", "cut_fill_copy_m256", "flags_m512", "garbage_m256", "stale_a_m512", "stale_b_m256", "quirk_4x24_m512", "pframe_at_i_m512",
           "truncated_i_m256", "empty_first_m512", "empty_later_m256", "fields_lzss_m512", "fields_lz77_m256", "mix_4x4_v2", "mix_128x96_v4")


def test_damaged_files_read_in_fives_with_a_seek_back_into_the_damage(tmp_path):
    """the corpus of tests/damage_cases.py (the files of tests/test_gpu_damage_files.py, which holds their full decode to the
    reference's pixels), one file of every kind of damage: truncated streams, cut chunks, chunks that are not where their header says"""
    ops, names = [], []
    for c in D.cases():
        if c["name"] not in DAMAGED:
            continue
        p = str(tmp_path / (c["name"] + ".agmv"))
        open(p, "wb").write(D.file_image(c))
        r = c["name"]
        names.append(r)
        ops += [[r, "open", p, {"index_bytes": 1 << 20}], [r, "read", 5], [r, "read", 5], [r, "seek", 3], [r, "read", 5], [r, "read", 5], [r, "read", 5],
                [r, "read", 5], [r, "read", 5], [r, "close"]]
    recs = run_child(tmp_path, {"ops": ops}, {"AGMV_BATCH_FRAMES": "4"})
    assert sorted(names) == sorted(DAMAGED)
    for k, r in enumerate(names):
        mine = recs[10 * k:10 * k + 10]
        reads_ok(mine, r)
        assert mine[0]["full"] >= 3 and mine[8]["n"] == 0 and mine[8]["tell"] == max(mine[0]["full"], 3), (r, mine)


def test_two_readers_and_one_shot_decodes_do_not_disturb_each_other(tmp_path, clip):
    """two files with different palettes (OPT I, two palettes; OPT II, one), their reads interleaved with each other and with one-shot
    decodes of either file, one of them deblocked and one a view: every read and every decode is right, the one-shot statistics are
    those of the one-shot calls alone, and each reader's counters are its own"""
    one, two = str(tmp_path / "one.agmv"), str(tmp_path / "two.agmv")
    ops = [["-", "encode", one, {"opt": 1}], ["-", "encode", two, {"opt": 2, "compression": 2}], ["x", "open", one, {"deblock": 16}], ["y", "open", two, {"fmt": "rgb24", "step": 2}],
           ["x", "read", 5], ["y", "read", 3], ["-", "decode", two, {}], ["x", "read", 5], ["-", "decode", one, {"deblock": 16}], ["y", "read", 3],
           ["-", "decode", one, {"frames": [13, 21, 1]}], ["x", "seek", 2], ["y", "read", 3], ["x", "read", 9], ["-", "decode", two, {"fmt": "rgb24"}],
           ["y", "read", 9], ["x", "read", 30], ["x", "close"], ["y", "read", 1], ["y", "close"]]
    recs = run_child(tmp_path, {"clip_npy": clip, "ops": ops})[2:]
    reads_ok(recs)
    assert recs[4]["deblock"]["strength"] == 0 and recs[6]["deblock"] == dict(recs[6]["deblock"], strength=16, frames=T)
    assert recs[6]["deblock"]["weak"] + recs[6]["deblock"]["strong"] > 0
    assert recs[8]["view"] == [21, 9, 8, 0] and recs[8]["deblock"]["strength"] == 0
    assert recs[12]["view"] == [21, 9, 8, 0] and recs[12]["deblock"]["strength"] == 0     # (still the last view call's: no reader writes them)
    x, y = recs[14]["stats"], recs[16]["stats"]
    assert (x["reads"], x["seeks"], x["restarts"], x["delivered"]) == (4, 1, 0, 5 + 5 + 9 + 13)
    assert x["lz_frames"] == 10 + 11 + 13 and x["gpu_frames"] == 10 + 11 + 13            # 0 .. 9; from checkpoint 0 (g0 = 0) 0 .. 10; 11 .. 23
    assert (y["reads"], y["seeks"], y["delivered"], y["lz_frames"], y["gpu_frames"]) == (4, 0, 12, 23, 23)


def test_a_closed_reader_raises_and_a_reader_is_a_context_manager(tmp_path, clip):
    ops = [["a", "open", None, {}], ["a", "read", 2], ["a", "close"], ["a", "read_closed"], ["b", "open", None, {}], ["b", "read", 30], ["b", "close"]]
    recs = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "ops": ops})
    reads_ok(recs)
    assert len(recs[3]["raised"]) == 5 and all(m and "closed" in m for m in recs[3]["raised"]), recs[3]
    assert recs[5]["n"] == T and recs[5]["stats"]["lz_frames"] == T                       # a reader opened behind a closed one starts from nothing
