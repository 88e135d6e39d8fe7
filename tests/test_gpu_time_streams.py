"""agmv_hip_time_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module text),
unchanged, with cases for the new entry point, run warm and on a fresh context, as tests/test_gpu_view_source_streams.py does for the
view.  The source clip is a device input and arrives behind the delay, so a launch that is not ordered on the caller's stream reads
the decoy or the early fill.  A byte layout and both YUV layouts, each through a wide window (16-byte loads and stores) and a narrow
one at an odd offset (element by element), a batch that starts behind frame 0 of the result.  The expectation is the numpy statement
(tests/time_cases.py), never a GPU call.  The cases are built here and are not registered in stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import stream_cases as SC
import scale_cases as L
import time_cases as TC
import view_source_cases as VS
import yuv_cases as Y

pytestmark = pytest.mark.gpu

N, SH, SW = 11, 12, 48
FIRST, STEP, VIEW_LEN = 1, 2, 5                                                  # frames 1, 3, 5, 7, 9
RATE, J0, COUNT = (3, 2, TC.AREA), 1, 2                                          # frames 1 and 2 of the 3 of R: taps 1 .. 2 and 3 .. 4 of V
WINDOWS = {"wide": (16, 0, 32, 12), "narrow": (1, 3, 21, 7)}
FORMATS = {"rgb24": L.P.RGB24, "nv12": Y.NV12, "i420-bt709": Y.I420 | Y.BT709}
CASES = sorted((f, w) for f in FORMATS for w in WINDOWS)


@functools.lru_cache(maxsize=None)
def time_case(layout, name):
    fmt, (x, y, w, h) = FORMATS[layout], WINDOWS[name]
    sets = []
    for seed in (570, 571):
        src = VS.raw_clip(fmt, N, SH, SW, seed)
        v = VS.view(fmt, src, SW, SH, FIRST, VIEW_LEN, STEP, x, y, w, h)
        sets.append(({"src": src}, {"dst": TC.resample(v, RATE[0], RATE[1], RATE[2], J0, COUNT)}))
    assert SC.differs(sets[0][1]["dst"], sets[1][1]["dst"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_time_frames_async(hip.ctx, fmt, SC.ptr(b["src"]), SW, SH, N, FIRST, STEP, VIEW_LEN, x, y, w, h, RATE[0], RATE[1], RATE[2], J0, COUNT,
                                                 SC.ptr(b["dst"]), hip._stream()))
    return SC.Case("time_frames-%s-%s" % (layout, name), sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"dst": ((COUNT, h, w), np.uint32)}, call)


@pytest.fixture(scope="module")
def delay():
    import torch
    from libagmv_amd import hip
    hip.load_library()
    assert torch.cuda.is_available()
    return SC.calibrate()


@pytest.fixture(scope="module")
def side(delay):
    import torch
    return SC.pick_stream(delay, [torch.cuda.default_stream()])


@pytest.mark.parametrize("state", ["warm", "fresh"])
@pytest.mark.parametrize("layout,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_late_input(layout, name, state, delay, side):
    import torch
    from libagmv_amd import AgmvHip
    case = time_case(layout, name)
    hip = AgmvHip(0)
    try:
        if state == "warm":
            run, exp = SC.run_quiet(case, hip)
            torch.cuda.synchronize()
            assert run.verdict(exp) is None, run.verdict(exp)
        SC.run_late(case, hip, delay, side, fresh=state == "fresh")
        hip.check()
    finally:
        torch.cuda.synchronize()
        hip.close()


def test_the_wrapper_takes_a_stream(delay, side):
    """AgmvHip.time_frames(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = time_case("nv12", "wide")
    x, y, w, h = WINDOWS["wide"]
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.time_frames("nv12", run.b["src"].reshape(-1), SW, SH, N, FIRST, STEP, VIEW_LEN, x, y, w, h, RATE[:2], j0=J0, count=COUNT,
                        out=run.b["dst"].reshape(-1).view(torch.int32), stream=side)
        assert side.query() is False, "time_frames returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
