"""agmv_hip_scale_frames_async on a busy non-blocking stream: the late-input harness of tests/stream_cases.py (see its module
text) with cases for the new entry point, run warm and on a fresh context.  The source clip arrives behind the delay and the
target holds the harness's early fill until its late fill arrives there too, so the one launch must be ordered on the caller's
stream and nothing may wait for it.  The expectation is the numpy statement (tests/upscale_cases.py), never a GPU call.  The cases
are built here and are not registered in stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import pixfmt_cases as P
import scale_cases as SCL
import stream_cases as SC
import upscale_cases as U
import yuv_cases as Y

pytestmark = pytest.mark.gpu

N, SW, SH, DW, DH = 3, 20, 12, 48, 34            # whole groups of 16, even rows, a non-integer ratio
FMTS = {"rgb24": P.RGB24, "nv12-bt709": Y.NV12 | Y.BT709}


@functools.lru_cache(maxsize=None)
def scale_case(name):
    fmt = FMTS[name]
    sets = []
    for seed in (190, 191):
        pix = np.random.default_rng(seed).integers(0, 1 << 32, (N, SH, SW), dtype=np.uint32)       # bits >= 24 set at random
        out = np.asarray(SCL.from_packed(fmt, U.scale_bilinear(pix, DW, DH))).view(np.uint8).reshape(N, -1)
        sets.append(({"src": pix}, {"dst": out}))
    assert SC.differs(sets[0][1]["dst"], sets[1][1]["dst"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_scale_frames_async(hip.ctx, U.BILINEAR, SC.ptr(b["src"]), SW, SH, N, fmt, DW, DH, SC.ptr(b["dst"]), hip._stream()))
    return SC.Case("scale_frames-" + name, sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"dst": (sets[0][1]["dst"].shape, np.uint8)}, call)


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
    case = scale_case(name)
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
    """AgmvHip.scale_frames_async(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = scale_case("rgb24")
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.scale_frames_async(U.BILINEAR, run.b["src"].reshape(-1), SW, SH, N, "rgb24", DW, DH, out=run.b["dst"], stream=side)
        assert side.query() is False, "scale_frames_async returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
