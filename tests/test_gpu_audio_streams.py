"""agmv_hip_audio_compand_async and agmv_hip_audio_expand_async on a busy non-blocking stream: the late-input harness of
tests/stream_cases.py (see its module text), run warm and on a fresh context.  The PCM (or the codes) is the call's only device
input: the decoy lies in it until the real samples arrive behind the delay, so a launch on another stream converts the decoy or is
painted over, and a host synchronisation trips the harness's second query.  The expectations are the numpy statement
(tests/audio_cases.py), never a GPU call.  Floats travel as their bits.  The cases are built here and are not registered in
stream_cases.CASES.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import audio_cases as A
import stream_cases as SC

pytestmark = pytest.mark.gpu

N, CH = 1028, 2                                   # 2056 samples: whole 16-sample units and a tail; planes of a multiple of 4 samples


def pcm_sets(fmt):
    """two sets of inputs in the layout fmt and the codes of each"""
    sets = []
    for seed in (170, 171):
        rng = np.random.default_rng(seed)
        if fmt == A.PCM_S16:
            x = rng.integers(0, 65536, (N, CH)).astype(np.uint16)
            sets.append((x, A.compand(x)))
        elif fmt == A.PCM_U8:
            x = rng.integers(0, 256, (N, CH)).astype(np.uint8)
            sets.append((x, x.copy()))
        else:
            x = rng.uniform(-1.05, 1.05, (CH, N)).astype(np.float32)
            sets.append((x.view(np.uint32), np.ascontiguousarray(A.compand(A.from_f32(x)).T)))
    return sets


def code_sets(fmt):
    """two sets of codes and what each expands to in the layout fmt"""
    sets = []
    for seed in (180, 181):
        c = np.random.default_rng(seed).integers(0, 256, (N, CH)).astype(np.uint8)
        out = {A.PCM_S16: lambda: A.expand(c), A.PCM_U8: lambda: c.copy(), A.PCM_F32P: lambda: np.ascontiguousarray(A.to_f32(A.expand(c)).T).view(np.uint32)}[fmt]()
        sets.append((c, out))
    return sets


@functools.lru_cache(maxsize=None)
def audio_case(direction, fmt):
    name = "audio_%s-%s" % (direction, {A.PCM_S16: "s16", A.PCM_U8: "u8", A.PCM_F32P: "f32p"}[fmt])
    if direction == "compand":
        (r, er), (d, ed) = pcm_sets(fmt)

        def call(hip, b, side):
            hip._ck(hip.L.agmv_hip_audio_compand_async(hip.ctx, fmt, SC.ptr(b["pcm"]), CH, N, SC.ptr(b["codes"]), hip._stream()))
        case = SC.Case(name, {"pcm": r}, {"pcm": d}, {"codes": er}, {"codes": ed}, {"codes": (er.shape, er.dtype)}, call)
    else:
        (r, er), (d, ed) = code_sets(fmt)

        def call(hip, b, side):
            hip._ck(hip.L.agmv_hip_audio_expand_async(hip.ctx, fmt, SC.ptr(b["codes"]), CH, N, SC.ptr(b["pcm"]), hip._stream()))
        case = SC.Case(name, {"codes": r}, {"codes": d}, {"pcm": er}, {"pcm": ed}, {"pcm": (er.shape, er.dtype)}, call)
    assert SC.differs(case.exp_real[case.compared()[0]], case.exp_decoy[case.compared()[0]])
    return case


CASES = [(d, f) for d in ("compand", "expand") for f in (A.PCM_S16, A.PCM_U8, A.PCM_F32P)]


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
@pytest.mark.parametrize("direction,fmt", CASES, ids=["%s-%d" % c for c in CASES])
def test_late_input(direction, fmt, state, delay, side):
    import torch
    from libagmv_amd import AgmvHip
    case = audio_case(direction, fmt)
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


def test_the_wrappers_take_a_stream(delay, side):
    """AgmvHip.audio_compand(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = audio_case("compand", A.PCM_S16)
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.audio_compand("s16", run.b["pcm"], codes=run.b["codes"], stream=side)
        assert side.query() is False, "audio_compand returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
