"""Writer sessions fed from a BUSY non-blocking stream: every piece handed to AGMV_WriterAnalyseDev / AGMV_WriterWriteDev is produced
late -- behind a bounded delay, the one of tests/stream_cases.py -- on a non-blocking torch stream, which the test synchronises just
before the call: the convention encode_frames documents, "the frames must be complete when called".  The one buffer all pieces travel
in is overwritten on that stream the moment the call returns, without another synchronisation, and the calls go to the library
directly, so nothing but the stream's own synchronisation orders the caller against the writer.  What is checked is the writer's own
ordering across calls: ingest, histogram and encode run on streams of the library's, and the file must still be, byte for byte, the
one-shot call's.  Once on a fresh session -- the first call of the library in its process, opened before the reference is encoded --
and once on a warm one.  In a child process, like every test that runs the sequence drivers (tests/children.py has the reasons); the
child imports torch and the package alone.  Needs an MI355X."""
import textwrap

import children as K
import numpy as np
import pytest

import memseq_cases as MC

pytestmark = pytest.mark.gpu

W, H, T = 64, 48, 37
ANALYSES, WRITES = [9, 4, 13, 11], [1, 2, 5, 3, 8, 11, 7]
DELAY_MS = 10.0

CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    x = torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda()
    top = max(job["analyses"] + job["writes"])
    decoy = torch.from_numpy(np.random.default_rng(5).integers(0, 1 << 24, size=(top,) + tuple(x.shape[1:]), dtype=np.int32)).cuda()
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
    torch.cuda.synchronize()

    def session(path, kw):
        wr = libagmv_amd.Writer(path, x.shape[1], x.shape[2], **kw)
        buf = torch.empty_like(x[:top])
        late = 0
        for call, sizes in ((wr._L.AGMV_WriterAnalyseDev, job["analyses"]), (wr._L.AGMV_WriterWriteDev, job["writes"])):
            p = 0
            for n in sizes:
                with torch.cuda.stream(side):
                    torch.cuda._sleep(delay)
                    buf[:n].copy_(x[p:p + n], non_blocking=True)
                late += side.query() is False                    # (the piece is still on its way)
                side.synchronize()                               # complete when called
                assert call(wr._h, buf.data_ptr(), n) == 0
                with torch.cuda.stream(side):
                    buf.copy_(decoy, non_blocking=True)          # the caller's again at once
                p += n
        st = wr.stats()
        written = wr.close()
        torch.cuda.synchronize()
        return {"bytes": open(path, "rb").read(), "written": written, "stats": st, "late": late}

    res = []
    for kw in job["cases"]:
        fresh = session("fresh.agmv", kw) if not res else None   # the library's first call in this process
        libagmv_amd.encode_frames("one.agmv", x, **kw)
        one = open("one.agmv", "rb").read()
        warm = session("warm.agmv", kw)
        rec = {"warm": warm["bytes"] == one, "written": warm["written"], "stats": warm["stats"], "late": warm["late"], "size": len(one)}
        if fresh:
            rec.update(fresh=fresh["bytes"] == one, fresh_written=fresh["written"])
        res.append(rec)
    print(json.dumps({"cases": res}))
""")


def test_pieces_from_a_busy_stream_fresh_and_warm(tmp_path):
    assert sum(ANALYSES) == sum(WRITES) == T
    cases = [dict(schedule=1), dict(schedule=2, opt=1, compression=2)]
    np.save(tmp_path / "clip.npy", MC.synth_clip(W, H, T))
    env = {"AGMV_BATCH_FRAMES": "8", "AGMV_LZ_DEVICE": None, "AGMV_LZ77_DEVICE": None, "AGMV_PALETTE_REFINE": None, "AGMV_DITHER": None, "AGMV_STABILISE": None}
    res = K.run_child(tmp_path, CHILD, {"clip": str(tmp_path / "clip.npy"), "cases": cases, "analyses": ANALYSES, "writes": WRITES, "delay_ms": DELAY_MS},
                      env, prelude="")["cases"]
    assert res[0]["fresh"] and res[0]["fresh_written"] == T, "the fresh writer's file differs from the one-shot call's: %r" % (res[0],)
    for kw, r in zip(cases, res):
        assert r["late"] == len(ANALYSES) + len(WRITES), "premise: a piece was complete before its synchronisation (delay too short): %r" % (r,)
        assert r["warm"] and r["size"] > 1000, "the warm writer's file differs from the one-shot call's: %r %r" % (kw, r)
        assert r["stats"]["analysed"] == r["stats"]["taken"] == T, (kw, r)
    assert res[0]["written"] == T and res[1]["written"] == 1 + (T - 6) // 2, res
