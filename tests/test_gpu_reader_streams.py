"""A reader's read while the caller's own non-blocking stream is busy: the late arrival of tests/stream_cases.py -- a bounded delay on
a non-blocking torch stream, then fills of its decoy bytes SENT and EARLY -- around libagmv_amd.Reader.read(n, out=).  A read works
on streams of the reader's own and returns with the frames complete; Reader.read orders itself behind the caller's device work
first, as decode_frames' callers are ordered.  So: the destination holds EARLY, and on the busy stream, behind the delay, SENT is
copied over it (its "previous contents", still being written) and the reference clip -- the frames the read must deliver, a slice
of the one-shot decode of the same file -- is copied into place.  The read must come back with the caller's stream idle, its frames
equal to the reference clip, and nothing of the late SENT fill left in them; a second read into the same destination, then quiet,
must be right as well.  In a child process, like every test that runs the sequence drivers (tests/children.py has the reasons);
the child imports torch and the package alone.  Needs an MI355X."""
import textwrap

import children as K
import numpy as np
import pytest

import memseq_cases as MC

pytestmark = pytest.mark.gpu

W, H0, T = 64, 48, 24
SENT, EARLY, DELAY_MS = 0xA5, 0x5A, 30.0                        # (the values of tests/stream_cases.py, which a child cannot import: it loads the oracle)

CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    path = "clip.agmv"
    libagmv_amd.encode_frames(path, torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda(), schedule=libagmv_amd.SCHEDULE_FULL)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                # the delay, measured once with events (stream_cases.calibrate)
        torch.cuda._sleep(1000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(20000000)
        b.record()
    side.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.05, ms
    delay = int(20000000 * job["delay_ms"] / ms)
    res = []
    for kw in job["cases"]:
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in kw.items()}
        step = kw.get("step", 1)
        full = libagmv_amd.decode_frames(path, **{k: v for k, v in kw.items() if k != "step"})[0]
        first, n = 5, 6
        want = full[first::step][:n].contiguous()
        rec = {"want": int(want.shape[0]), "distinct": int(len(torch.unique(want.view(torch.uint8))))}
        with libagmv_amd.Reader(path, **kw) as r:
            r.seek(first)
            out = torch.full_like(want.view(torch.uint8), job["early"]).view(want.dtype)
            late = torch.full_like(want.view(torch.uint8), job["sent"]).view(want.dtype)
            ref = torch.zeros_like(want)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(delay)
                out.copy_(late, non_blocking=True)               # the destination's previous contents, still on their way
                ref.copy_(want, non_blocking=True)               # ... and the reference clip
                rec["busy_before"] = side.query() is False
                got = r.read(n, out=out)
                rec["idle_after"] = side.query() is True
            rec["same_buffer"] = got.data_ptr() == out.data_ptr() and got.shape == want.shape
            rec["ok"] = bool((out == ref).all())
            rec["tell"] = r.tell()
            again = r.read(n, out=out)                           # quiet now: the next frames into the same destination
            nxt = full[first + n * step::step][:n]
            rec["again"] = int(again.shape[0])
            rec["again_ok"] = again.shape == nxt.shape and bool((again == nxt).all())
        res.append(rec)
    print(json.dumps({"cases": res}))
""")


def test_a_read_while_the_callers_stream_is_busy(tmp_path):
    cases = [dict(fmt="xrgb32"), dict(fmt="rgb24", crop=[3, 5, 14, 20], step=2)]
    np.save(tmp_path / "clip.npy", MC.synth_clip(W, H0, T))
    res = K.run_child(tmp_path, CHILD, {"clip": str(tmp_path / "clip.npy"), "cases": cases, "sent": SENT, "early": EARLY, "delay_ms": DELAY_MS},
                      {"AGMV_BATCH_FRAMES": "8", "AGMV_LZ_DECODE_DEVICE": None}, prelude="")["cases"]
    for kw, r in zip(cases, res):
        assert r["want"] == 6 and r["distinct"] > 16, (kw, r)
        assert r["busy_before"], "premise: the stream is idle before the read (delay too short): %r" % (r,)
        assert r["idle_after"], "Reader.read returned while the caller's stream was still writing the destination: %r" % (r,)
        assert r["same_buffer"] and r["ok"], "the read's frames are not the reference clip (the late fill came after them, or the read was wrong): %r" % (r,)
        assert r["tell"] == 5 + 6 * kw.get("step", 1) and r["again"] > 0 and r["again_ok"], (kw, r)
