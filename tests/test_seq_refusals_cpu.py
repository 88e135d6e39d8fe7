"""What the file-level entry points refuse, and in which order: the return value of every refused call of a fixed argument matrix,
replayed against the built library and compared with tests/golden/seq_refusals.json (recorded from this library before its
sequence API was reshaped; `python tests/test_seq_refusals_cpu.py` records it again).  The matrix: per entry point a valid baseline,
every single violation the header documents, every pair of violations from two different return-code classes (the pairs pin the
order of the checks), the calls that only read the header, and a pending AGMV_SetAudioDev track followed by a second refused call
(-2 there shows that the first call consumed the track; -5 would show that it is still pending).  Every case holds at least one
violation that is refused before a device is opened: the pointers are never read, no file is created."""
import ctypes as C
import itertools
import json
import os

import hostlib as H

GOLDEN = os.path.join(H.ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "seq_refusals.json")
FAKE = 4096                                                      # never dereferenced
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))                        # mean, std

# ---- the entry points: (argument, baseline value) in the order of the C signature (libagmv_amd/abi.py has the types)
ENC = [("fps", 24), ("opt", 3), ("quality", 3), ("compression", 1), ("schedule", 2)]
CLIP = [("n", 8), ("w", 16), ("h", 16)]
TENSOR = [("type", 1), ("mean", UNIT[0]), ("std", UNIT[1])]
ENTRY = {
    "AGMV_EncodeFramesDev": [("filename", "out"), ("frames", FAKE)] + CLIP + ENC,
    "AGMV_EncodeFramesFmtDev": [("filename", "out"), ("frames", FAKE), ("fmt", 2)] + CLIP + ENC,
    "AGMV_EncodeFramesScaledDev": [("filename", "out"), ("frames", FAKE), ("fmt", 2), ("n", 8), ("sw", 32), ("sh", 32), ("w", 16),
                                   ("h", 16), ("filt", 2)] + ENC,
    "AGMV_EncodeFramesTensorDev": [("filename", "out"), ("frames", FAKE)] + TENSOR + CLIP + ENC,
    "AGMV_DecodeFramesDev": [("filename", "good"), ("frames", FAKE), ("cap", 4), ("info", None)],
    "AGMV_DecodeFramesFmtDev": [("filename", "good"), ("frames", FAKE), ("fmt", 2), ("cap", 4), ("info", None)],
    "AGMV_DecodeFramesScaledDev": [("filename", "good"), ("frames", FAKE), ("fmt", 2), ("w", 16), ("h", 16), ("filt", 1), ("cap", 4),
                                   ("info", None)],
    "AGMV_DecodeFramesTensorDev": [("filename", "good"), ("frames", FAKE)] + TENSOR + [("w", 16), ("h", 16), ("filt", 1), ("cap", 4),
                                                                                              ("info", None)],
    "AGMV_MeasureFramesDev": [("test", FAKE), ("ref", FAKE), ("fmt", 2), ("n", 2), ("w", 8), ("h", 8), ("quality", FAKE)],
    "AGMV_MeasureFileDev": [("filename", "good"), ("ref", FAKE), ("fmt", 2), ("n", "frames-of-good"), ("quality", FAKE), ("info", None)],
    "AGMV_DecodeAudioDev": [("filename", "good"), ("pcm", FAKE), ("fmt", 1), ("cap", 1 << 20), ("info", None)],
}

# ---- the violations: (return-code class, changes to the baseline).  Two of different classes whose changes do not touch the same
# argument make a pair.  "audio" is no argument: a track is pending when the call is made.
BAD_FMT = [("-1", dict(fmt=v)) for v in (0, 6, 2 | 0x100, 16 | 0x400)]
BAD_TENSOR = [("-1", dict(type=0)), ("-1", dict(type=4)), ("-1", dict(mean=None)), ("-1", dict(std=None)), ("-1", dict(std=(1.0, 0.0, 1.0))),
              ("-1", dict(mean=(0.0, 2.0 ** 33, 0.0)))]
BAD_ENC = ([("-1", dict(filename=None)), ("-1", dict(frames=None))] +
           [("-1", {k: v}) for k, v in (("opt", 0), ("opt", 9), ("quality", 0), ("quality", 4), ("compression", 0), ("compression", 3),
                                        ("schedule", 0), ("schedule", 4))] +
           [("-5", dict(audio=True, schedule=3))] +
           [("-2", dict(n=3)), ("-2", dict(n=1, opt=1)), ("-2", dict(n=0, schedule=1)), ("-2", dict(n=1 << 31))])
BAD_SIZE = [("-3", c) for c in (dict(w=0), dict(h=0), dict(w=18), dict(h=18), dict(w=1 << 15, h=1 << 14), dict(w=(1 << 32) + 16), dict(opt=5, w=1))]
BAD_SCALED_SIZE = [("-3", c) for c in (dict(w=0), dict(h=0), dict(w=18), dict(h=18), dict(w=(1 << 32) + 16), dict(sw=0), dict(sh=0), dict(opt=5), dict(opt=8),
                                       dict(sw=16, sh=16, w=32), dict(sw=16, sh=16, h=32), dict(sw=4097, sh=4096),
                                       dict(filt=1, sw=1 << 15, sh=1 << 14))]
# the files: "good" is a golden file, the others are it with a header field changed by hand (files() below)
BAD_FILE = [("-Error", dict(filename=None)), ("-Error", dict(filename="missing")), ("-Error", dict(filename="badfourcc")), ("-Error", dict(filename="w6"))]
NO_DST = [("0", dict(frames=None))]
BAD_TARGET = [("-4", c) for c in (dict(w=0), dict(h=0), dict(w=(1 << 28) + 4), dict(w=1 << 15, h=1 << 14))]
BAD_FILTER = [("-1", dict(filt=0)), ("-1", dict(filt=4))]
BAD_AREA = [("-4 of the file", dict(filt=2, w=4096)), ("-4 of the file", dict(filt=2, h=4096)), ("-4 of the file", dict(filt=2, filename="huge"))]
VIOLATIONS = {
    "AGMV_EncodeFramesDev": BAD_ENC + BAD_SIZE,
    "AGMV_EncodeFramesFmtDev": BAD_FMT + BAD_ENC + BAD_SIZE,
    "AGMV_EncodeFramesScaledDev": BAD_FMT + [("-1", dict(filt=0)), ("-1", dict(filt=3))] + BAD_ENC + BAD_SCALED_SIZE,
    "AGMV_EncodeFramesTensorDev": BAD_TENSOR + BAD_ENC + BAD_SIZE,
    "AGMV_DecodeFramesDev": BAD_FILE + NO_DST,
    "AGMV_DecodeFramesFmtDev": BAD_FMT + BAD_FILE + NO_DST,
    "AGMV_DecodeFramesScaledDev": BAD_FMT + BAD_FILTER + BAD_TARGET + BAD_FILE + NO_DST + BAD_AREA,
    "AGMV_DecodeFramesTensorDev": BAD_TENSOR + BAD_FILTER + BAD_TARGET + BAD_FILE + NO_DST + BAD_AREA + [("-Error", dict(w=0, h=0, filt=0, filename="missing"))],
    "AGMV_MeasureFramesDev": (BAD_FMT + [("-1", dict(test=None)), ("-1", dict(ref=None)), ("-1", dict(quality=None))] +
                              [("-3", c) for c in (dict(w=6), dict(h=6), dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 16), dict(w=(1 << 32) + 8), dict(n=1 << 31))] +
                              [("0", dict(n=0))]),
    "AGMV_MeasureFileDev": (BAD_FMT + [("-1", dict(ref=None))] + BAD_FILE + [("0", dict(quality=None))] +
                            [("-3", dict(n=1)), ("-3", dict(n=1 << 20)), ("-3", dict(filename="odd", fmt=16)), ("-3", dict(filename="odd", fmt=17 | 0x300))]),
    "AGMV_DecodeAudioDev": ([("-1", dict(fmt=0)), ("-1", dict(fmt=4))] + [v for v in BAD_FILE if v[1]["filename"] != "w6"] +
                            [("0", dict(pcm=None)), ("0", dict(filename="notrack"))] +
                            [("-1 of the file", c) for c in (dict(filename="track16", fmt=2), dict(filename="track8", fmt=1), dict(filename="track8", fmt=3),
                                                             dict(filename="track0ch"), dict(filename="track9ch", fmt=3))]),
}


def name_of(changes):
    return " ".join("%s=%s" % (k, changes[k]) for k in sorted(changes))


def cases():
    """(entry point, case name, changes) of the whole matrix, in a fixed order"""
    for entry, bad in VIOLATIONS.items():
        for _, c in bad:
            yield entry, name_of(c), c
        for (ka, a), (kb, b) in itertools.combinations(bad, 2):
            if ka != kb and not set(a) & set(b):
                yield entry, name_of(a) + " & " + name_of(b), dict(a, **b)


def files(tmp):
    """the names a `filename` of the matrix may hold, as paths: the golden file, and copies of it with a header field changed"""
    data = open(os.path.join(GOLDEN, "agmv_splash.agmv"), "rb").read()
    n, w, h, duration = (int.from_bytes(data[k:k + 4], "little") for k in (4, 8, 12, 22))
    assert n > 1 and w % 4 == 0 and h % 4 == 0 and w < 4096 and h < 4096 and duration != 0
    le = lambda v, size=4: v.to_bytes(size, "little")

    def track(channels, bits):                                   # total_audio_duration, sample_rate, audio_size, num_of_channels, bits_per_sample
        return data[:22] + le(1) + le(8000) + le(8000) + le(channels, 2) + le(bits, 2) + data[38:]
    made = {"badfourcc": b"AGMX" + data[4:], "w6": data[:8] + le(6) + data[12:], "odd": data[:8] + le(w - 1) + data[12:],
            "huge": data[:8] + le(8192) + le(4096) + data[16:], "track16": track(1, 16), "track8": track(1, 8), "track0ch": track(0, 16),
            "track9ch": track(9, 16), "notrack": data[:22] + le(0) + data[26:]}
    paths = {None: None, "good": os.path.join(GOLDEN, "agmv_splash.agmv").encode(), "missing": os.path.join(tmp, "missing.agmv").encode(),
             "out": os.path.join(tmp, "out", "x.agmv").encode()}
    os.mkdir(os.path.join(tmp, "out"))
    for name, content in made.items():
        paths[name] = os.path.join(tmp, name + ".agmv").encode()
        open(paths[name], "wb").write(content)
    return paths, n


def replay(tmp, verbose=False):
    """{entry point: {case name: return value}}; a case with a pending track is [its return value, that of the second refused call]"""
    L = H.lib()
    paths, nframes = files(tmp)
    got = {}
    for entry, name, changes in cases():
        f = getattr(L, entry)
        assert len(f.argtypes) == len(ENTRY[entry])

        def call(changes):
            args = []
            for (arg, base), t in zip(ENTRY[entry], f.argtypes):
                v = changes.get(arg, base)
                if arg == "filename":
                    v = paths[v]
                elif arg in ("mean", "std") and v is not None:
                    v = (C.c_float * 3)(*v)
                elif v == FAKE and issubclass(t, C._Pointer):       # (a structure pointer takes no plain address)
                    v = C.cast(v, t)
                elif v == "frames-of-good":
                    v = nframes
                args.append(v)
            return f(*args)
        if verbose:
            print(entry, name, flush=True)
        assert L.AGMV_SetAudioDev(None, 1, 0, 0, 0) == 0         # nothing pending
        if changes.get("audio"):
            assert L.AGMV_SetAudioDev(FAKE, 1, 48000, 48000, 2) == 0
            rc = [call(changes), call(dict(schedule=3, n=3))]
        else:
            rc = call(changes)
        assert name not in got.setdefault(entry, {}), (entry, name)
        got[entry][name] = rc
    assert not os.listdir(os.path.join(tmp, "out"))              # no encoder created its file
    return got


def test_every_refusal_of_the_matrix_returns_what_was_recorded(tmp_path):
    want = json.load(open(FIXTURE))
    got = replay(str(tmp_path))
    assert sorted(got) == sorted(want) == sorted(ENTRY)
    wrong = [(e, k, got[e].get(k), want[e].get(k)) for e in want for k in sorted(set(want[e]) | set(got[e])) if got[e].get(k) != want[e].get(k)]
    assert not wrong, wrong[:20]
    assert sum(len(v) for v in want.values()) > 1000


if __name__ == "__main__":
    import sys
    import tempfile
    sys.path.insert(0, H.ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        rec = replay(tmp, verbose=True)
    with open(FIXTURE, "w") as out:
        out.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (e, ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rec[e].items()))
                                    for e in rec) + "\n}\n")
    print("recorded %d cases" % sum(len(v) for v in rec.values()))
