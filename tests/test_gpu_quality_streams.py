"""agmv_hip_measure_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module
text) with cases for the new entry point, run warm and on a fresh context.  Both clips are device inputs and arrive behind the
delay; the result array holds the harness's early fill until its late fill arrives there too, so the call's own clearing must
be ordered on the caller's stream like its kernel: a memset on another stream is painted over, or adds to the fill.  The
expectation is the numpy statement (tests/quality_cases.py), never a GPU call.  The cases are built here and are not registered
in stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import pixfmt_cases as P
import quality_cases as Q
import stream_cases as SC
import yuv_cases as Y

pytestmark = pytest.mark.gpu

N, WW, HH = 3, 48, 20                            # whole groups of 16, two block rows of windows
FMTS = {"rgb24": P.RGB24, "nv12-bt709": Y.NV12 | Y.BT709}


@functools.lru_cache(maxsize=None)
def measure_case(name):
    fmt = FMTS[name]
    sets = []
    for seed in (170, 171):
        test = Q.noise(seed, N, HH, WW) | np.uint32(0x7E000000)            # bits >= 24 set
        raw, ref = Q.reference_clip(fmt, Q.perturbed(test, seed + 10, 5 + seed % 2 * 20))
        sets.append(({"test": test, "ref": raw}, {"q": Q.entries(Q.measure(test, ref))}))
    assert SC.differs(sets[0][1]["q"], sets[1][1]["q"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_measure_frames_async(hip.ctx, SC.ptr(b["test"]), fmt, SC.ptr(b["ref"]), WW, HH, N, SC.ptr(b["q"]), hip._stream()))
    return SC.Case("measure_frames-" + name, sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"q": ((N, 12), np.uint64)}, call)


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
@pytest.mark.parametrize("name", sorted(FMTS))
def test_late_input(name, state, delay, side):
    import torch
    from libagmv_amd import AgmvHip
    case = measure_case(name)
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
    """AgmvHip.measure_frames(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = measure_case("rgb24")
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.measure_frames(run.b["test"].reshape(-1), "rgb24", run.b["ref"].reshape(-1), WW, HH, N, out=run.b["q"], stream=side)
        assert side.query() is False, "measure_frames returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
