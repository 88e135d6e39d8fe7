"""agmv_hip_deblock_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module
text) with one case for the new entry point, run warm and on a fresh context.  The source clip and the counters are the call's device
inputs, the destination and the counters its outputs; the counters are changed in place: the decoy lies in the inputs until the
real words arrive behind the delay, so a launch on another stream deblocks the decoy or is painted over, and a host synchronisation
trips the harness's second query.  The expectation is the numpy statement (tests/deblock_cases.py), never a GPU call.  The case is
built here and is not registered in stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import deblock_cases as K
import stream_cases as SC

pytestmark = pytest.mark.gpu

N, HH, WW, STRENGTH = 3, 12, 260, 16                        # 66 x 4 cells: five waves, all nine kinds of cell


@functools.lru_cache(maxsize=None)
def deblock_case():
    sets = []
    for seed, start in ((170, (1000, 7)), (171, (5, 900))):
        pix = K.staircase_clip(N, HH, WW, seed)
        want, weak, strong = K.deblock(pix, STRENGTH)
        assert weak and strong
        sets.append(({"pix": pix, "counts": np.array(start, np.uint64)}, {"out": want, "counts": np.array([start[0] + weak, start[1] + strong], np.uint64)}))
    assert SC.differs(sets[0][1]["out"], sets[1][1]["out"]) and SC.differs(sets[0][1]["counts"], sets[1][1]["counts"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_deblock_frames_async(hip.ctx, STRENGTH, SC.ptr(b["pix"]), WW, HH, N, SC.ptr(b["out"]), SC.ptr(b["counts"]), hip._stream()))
    return SC.Case("deblock_frames", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"out": ((N, HH, WW), np.uint32)}, call, inplace=("counts",))


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
def test_late_input(state, delay, side):
    import torch
    from libagmv_amd import AgmvHip
    case = deblock_case()
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
    """AgmvHip.deblock_frames(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = deblock_case()
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.deblock_frames(run.b["pix"].reshape(-1), WW, HH, STRENGTH, out=run.b["out"].reshape(-1), counts=run.b["counts"], stream=side)
        assert side.query() is False, "deblock_frames returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
