"""agmv_hip_stabilise_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module
text) with one case for the new entry point, run warm and on a fresh context.  The clip and the counter are the call's device
arguments and both are changed in place: the decoy lies in them until the real words arrive behind the delay, so a launch on another
stream stabilises the decoy or is painted over, and a host synchronisation trips the harness's second query.  The expectation is
the numpy statement (tests/stabilise_cases.py), never a GPU call.  The case is built here and is not registered in
stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import stabilise_cases as S
import stream_cases as SC

pytestmark = pytest.mark.gpu

N, HH, WW, STRENGTH, FIRST_FC = 7, 8, 260, 8, 2             # a leading part, a whole GOP and a trailing one; 130 blocks: three waves


@functools.lru_cache(maxsize=None)
def stabilise_case():
    sets = []
    for seed, start in ((170, 1000), (171, 5)):
        pix = S.random_clip(N, HH, WW, STRENGTH, seed)
        want, examined, replaced = S.stabilise(pix, STRENGTH, FIRST_FC)
        assert 0 < replaced < examined
        sets.append(({"pix": pix, "count": np.array([start], np.uint64)}, {"pix": want, "count": np.array([start + replaced], np.uint64)}))
    assert SC.differs(sets[0][1]["pix"], sets[1][1]["pix"]) and SC.differs(sets[0][1]["count"], sets[1][1]["count"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_stabilise_frames_async(hip.ctx, STRENGTH, SC.ptr(b["pix"]), WW, HH, N, FIRST_FC, SC.ptr(b["count"]), hip._stream()))
    return SC.Case("stabilise_frames", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {}, call, inplace=("pix", "count"))


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
    case = stabilise_case()
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
    """AgmvHip.stabilise_frames(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = stabilise_case()
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.stabilise_frames(run.b["pix"].reshape(-1), WW, HH, STRENGTH, FIRST_FC, run.b["count"], stream=side)
        assert side.query() is False, "stabilise_frames returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
