"""Records tests/golden/audio/ref_*.agmv: the files the compiled reference (oracle/_ref/libagmv_ref.so, built by oracle/Makefile where the
reference's source is present) writes for the clip, the tracks and the cases of tests/test_gpu_audio_files.py.  Its drivers run on
objects that hold the track through the setters and AGMV_SyncAudioTrack, one file per process (they free the caller's object and
take about 10 s each: the palette build sorts the whole histogram).  CPU only.

    python tests/golden/make_golden_audio.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

import numpy as np  # noqa: E402

import hostlib as H  # noqa: E402
import oracles as O  # noqa: E402
import test_gpu_audio_files as F  # noqa: E402

REF_CHILD = F.DRIVE + textwrap.dedent("""
    R = C.CDLL(job["ref"])
    if job["only"] < len(job["cases"]):
        name, schedule, opt, comp, track = job["cases"][job["only"]]
        drive(R, "ref_%s.agmv" % name, schedule, opt, comp, *tracks[track])
    else:
        drive(R, "ref_u8.agmv", 2, 3, 1, pcm8, job["long_rate"])
""")


def main():
    frames = F.clip()
    long_, short, pcm8, _ = F.tracks()
    job = {"T": F.T, "W": F.W, "H": F.HH, "cases": F.CASES, "long_rate": F.LONG[1], "short_rate": F.SHORT[1], "root": H.ROOT, "tests": TESTS, "ref": O.REF_SO}
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "fr"))
        for t in range(1, F.T + 1):
            H.write_bmp(os.path.join(d, "fr", "f%d.bmp" % t), frames[t - 1])
        for name, a in (("long", long_), ("short", short), ("pcm8", pcm8)):
            np.save(os.path.join(d, name + ".npy"), a)
        kids = [subprocess.Popen([sys.executable, "-c", REF_CHILD, json.dumps(dict(job, only=k))], cwd=d, stdout=subprocess.DEVNULL)
                for k in range(len(F.CASES) + 1)]
        assert [p.wait() for p in kids] == [0] * len(kids)
        os.makedirs(os.path.join(HERE, "audio"), exist_ok=True)
        for f in sorted(os.listdir(d)):
            if f.startswith("ref_") and f.endswith(".agmv"):
                shutil.copy(os.path.join(d, f), os.path.join(HERE, "audio", f))
                print(f, os.path.getsize(os.path.join(d, f)))


if __name__ == "__main__":
    main()
