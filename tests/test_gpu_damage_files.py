"""Every file-decode path against the REFERENCE's pixels on damaged files: the corpus of tests/damage_cases.py written to disk and
decoded by libagmv_amd.decode_frames (AGMV_DecodeFramesFmtDev: chunk locator, host or device LZ stage with the one persistent buffer,
the 16 stale bytes behind each row, batches, GOP ranges), by AGMV_DecodeAGMV's BMP export and by a view that starts at a GOP; the
pixel hashes are those the compiled reference left in tests/golden/golden_damage.json.  include/agmv.h documents no file of this
corpus that the drivers refuse and the reference decodes, so no case asserts a refusal.  Child processes as in
tests/test_gpu_view_files.py.  Needs an MI355X."""
import hashlib
import json
import os
import textwrap

import children as K
import numpy as np
import pytest

import damage_cases as D

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = (1, 4, 5, 8, 64)

# job: runs = [{path, env: {name: value or none}, frames: [start, stop, step] or none}].  Answers {"runs": [{n, sha: [...], stats}]}.
CHILD = textwrap.dedent("""
    import ctypes as C, hashlib, json, os, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import abi, seq
    L = seq.load_library()
    stats = abi.AGMV_VIEW_STATS()
    out = []
    for r in job["runs"]:
        for k, v in r["env"].items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        kw = {}
        if r.get("frames"):
            kw["frames"] = slice(*r["frames"])
        got, info = libagmv_amd.decode_frames(r["path"], **kw)
        L.AGMV_GetViewStats(C.byref(stats))
        px = got.cpu().numpy().view(np.uint32).reshape(len(got), -1)
        out.append({"n": len(px), "sha": [hashlib.sha256(np.ascontiguousarray(p).tobytes()).hexdigest() for p in px],
                    "stats": [stats.lz_frames, stats.gpu_frames, stats.delivered, stats.restarts]})
    print(json.dumps({"runs": out}))
""")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "golden_damage.json")))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path of the case's file"""
    d = tmp_path_factory.mktemp("damaged")
    out = {}
    for c in D.cases():
        out[c["name"]] = str(d / (c["name"] + ".agmv"))
        with open(out[c["name"]], "wb") as f:
            f.write(D.file_image(c))
    return out


def exported_pixels(d, k, w, h):
    raw = open(os.path.join(d, "quick_export_%d.bmp" % k), "rb").read()
    px = np.frombuffer(raw[54:], np.uint8).reshape(h, -1)[:, :w * 3].reshape(h, w, 3).astype(np.uint32)
    return px[..., 2] << 16 | px[..., 1] << 8 | px[..., 0]


def run(cwd, runs):
    return K.run_child(cwd, CHILD, {"runs": runs}, prelude="")["runs"]


@pytest.mark.parametrize("ranges", [None, "4"])
@pytest.mark.parametrize("lz", ["host", "device"])
def test_full_decode_of_every_damaged_file(tmp_path, golden, files, lz, ranges):
    """every case at AGMV_BATCH_FRAMES 1, 4, 5, 8 and 64: the frames the reference decoded, and as many"""
    env = {"AGMV_LZ_DECODE_DEVICE": "1" if lz == "device" else None, "AGMV_DEC_RANGE_FRAMES": ranges}
    runs = [{"name": n, "path": p, "env": dict(env, AGMV_BATCH_FRAMES=str(b))} for n, p in files.items() for b in BATCHES]
    for r, got in zip(runs, run(tmp_path, runs)):
        want = [f[2] for f in golden[r["name"]]["frames"] if f[0] == 0]
        assert got["n"] == len(want), "%s %s: %d frames delivered, the reference decoded %d" % (r["name"], r["env"], got["n"], len(want))
        bad = [t for t in range(len(want)) if got["sha"][t] != want[t]]
        assert not bad, "%s %s: frames %s differ from the reference's" % (r["name"], r["env"], bad)


@pytest.mark.parametrize("batch", [1, 8])
def test_bmp_export_of_stale_flags_and_disagreeing_fields(tmp_path, golden, files, batch):
    for name in sorted(n for n in files if n.startswith(("stale_", "fields_"))):
        d = tmp_path / name
        d.mkdir()
        r = K.decode_child(d, files[name], batch=batch)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        g = golden[name]
        for k, f in enumerate(g["frames"]):
            px = exported_pixels(str(d), k + 1, g["w"], g["h"]) & np.uint32(0xFFFFFF)
            assert hashlib.sha256(np.ascontiguousarray(px, np.uint32).tobytes()).hexdigest() == f[2], "%s batch %d: exported frame %d" % (name, batch, k)
        assert not os.path.exists(str(d / ("quick_export_%d.bmp" % (len(g["frames"]) + 1))))


@pytest.mark.parametrize("lz", ["host", "device"])
def test_a_view_from_frame_9_is_the_references_frames(tmp_path, golden, files, lz):
    """frames 9, 11, ... of the files whose GOP 2 depends on the frames before it: the reference's decode of them, after one restart;
    on the clean clip no restart"""
    env = {"AGMV_LZ_DECODE_DEVICE": "1" if lz == "device" else None, "AGMV_DEC_RANGE_FRAMES": None, "AGMV_BATCH_FRAMES": "8"}
    names = [k + m for m in ("m512", "m256") for k in ("pframe_at_i_", "truncated_i_", "clean_")]
    runs = [{"name": n, "path": files[n], "env": env, "frames": [9, None, 2]} for n in names]
    for r, got in zip(runs, run(tmp_path, runs)):
        want = [f[2] for f in golden[r["name"]]["frames"]][9::2]
        assert got["sha"] == want, "%s: the view is not the reference's frames 9, 11, ..." % r["name"]
        assert got["stats"][2] == len(want) and got["stats"][3] == (0 if r["name"].startswith("clean_") else 1), (r["name"], got["stats"])
