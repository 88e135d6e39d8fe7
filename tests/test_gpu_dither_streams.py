"""agmv_hip_dither_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module
text) with one case for the new entry point, run warm and on a fresh context.  The clip is the call's only device input and is
dithered in place: the decoy lies in it until the real pixels arrive behind the delay, so a launch on another stream dithers the
decoy or is painted over, and a host synchronisation trips the harness's second query.  The expectation is the numpy statement
(tests/dither_cases.py) with the brute-force nearest entry, never a GPU call.  The case is built here and is not registered in
stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import dither_cases as D
import stream_cases as SC

pytestmark = pytest.mark.gpu

N, HH, WW, STRENGTH = 3, 7, 33, 32                # w no multiple of 4, w * h no multiple of 16: the frames' origins matter


@functools.lru_cache(maxsize=None)
def dither_case():
    pal = D.pal512_of(*SC.palettes())
    near = D.brute_nearest(pal, True)
    sets = []
    for seed in (160, 161):
        rng = np.random.default_rng(seed)
        pix = rng.integers(0, 1 << 24, (N, HH, WW)).astype(np.uint32)
        pix[0, 0, :8] = pal[rng.integers(0, 512, 8)] | np.uint32(0x7E000000)       # exact hits, bits >= 24 set
        sets.append(({"pix": pix}, {"pix": D.dither(pix, pal, True, STRENGTH, near)}))
    assert SC.differs(sets[0][1]["pix"], sets[1][1]["pix"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_dither_frames_async(hip.ctx, STRENGTH, SC.ptr(b["pix"]), WW, HH, N, hip._stream()))
    return SC.Case("dither_frames-512", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {}, call, inplace=("pix",), setup=SC.set_palette(True))


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
    case = dither_case()
    hip = AgmvHip(0)
    try:
        case.setup(hip)
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
    """AgmvHip.dither_frames(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = dither_case()
    hip = AgmvHip(0)
    try:
        case.setup(hip)
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.dither_frames(run.b["pix"].reshape(-1), WW, HH, STRENGTH, stream=side)
        assert side.query() is False, "dither_frames returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
