"""agmv_hip_view_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module
text) with cases for the new entry point, run warm and on a fresh context.  The source clip is a device input and arrives behind the
delay, so a copy that is not ordered on the caller's stream reads the decoy or the early fill.  A wide window (16-byte loads and
stores) and a narrow one (word by word).  The expectation is the numpy statement (tests/view_cases.py), never a GPU call.  The cases
are built here and are not registered in stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import stream_cases as SC
import view_cases as V

pytestmark = pytest.mark.gpu

N, SH, SW = 9, 12, 20
FIRST, STEP, COUNT = 1, 3, 3
WINDOWS = {"wide": (4, 0, 8, 12), "narrow": (1, 3, 5, 7)}


@functools.lru_cache(maxsize=None)
def view_case(name):
    x, y, w, h = WINDOWS[name]
    sets = []
    for seed in (270, 271):
        src = V.clip(N, SH, SW, seed)
        sets.append(({"src": src}, {"dst": V.view(src, FIRST, COUNT, STEP, x, y, w, h)}))
    assert SC.differs(sets[0][1]["dst"], sets[1][1]["dst"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_view_frames_async(hip.ctx, SC.ptr(b["src"]), SW, SH, FIRST, STEP, COUNT, x, y, w, h, SC.ptr(b["dst"]), hip._stream()))
    return SC.Case("view_frames-" + name, sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"dst": ((COUNT, h, w), np.uint32)}, call)


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
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_late_input(name, state, delay, side):
    import torch
    from libagmv_amd import AgmvHip
    case = view_case(name)
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
    """AgmvHip.view_frames_async(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = view_case("wide")
    x, y, w, h = WINDOWS["wide"]
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.view_frames_async(run.b["src"].reshape(-1).view(torch.int32), SW, SH, FIRST, STEP, COUNT, x, y, w, h, out=run.b["dst"].reshape(-1).view(torch.int32),
                              stream=side)
        assert side.query() is False, "view_frames_async returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
