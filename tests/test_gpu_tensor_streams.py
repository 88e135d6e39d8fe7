"""agmv_hip_tensor_from_xrgb_async and agmv_hip_tensor_to_xrgb_async on a busy non-blocking stream: the late-input harness of
tests/stream_cases.py (see its module text) with cases for the two entry points, run warm and on a fresh context.  The source
clip -- and for the sink the table too -- arrives behind the delay and the target holds the harness's early fill until its late
fill arrives there too, so the one launch must be ordered on the caller's stream and nothing may wait for it.  The expectation is
the numpy statement (tests/tensor_cases.py, tests/upscale_cases.py), never a GPU call.  The cases are built here and are not
registered in stream_cases.CASES.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import stream_cases as SC
import tensor_cases as TC
import upscale_cases as U

pytestmark = pytest.mark.gpu

N, SW, SH, DW, DH = 3, 20, 12, 48, 34            # whole groups of 16, a non-integer ratio
NORMS = ("imagenet", "half")                     # the real set's and the decoy's: the table is a device input like the clip


@functools.lru_cache(maxsize=None)
def sink_case(t):
    sets = []
    for seed, norm in zip((290, 291), NORMS):
        pix = np.random.default_rng(seed).integers(0, 1 << 32, (N, SH, SW), dtype=np.uint32)       # bits >= 24 set at random
        tab = TC.table(t, *TC.NORMS[norm])
        sets.append(({"src": pix, "table": tab}, {"dst": TC.from_packed(tab, U.scale_bilinear(pix, DW, DH))}))
    assert SC.differs(sets[0][1]["dst"], sets[1][1]["dst"])

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_tensor_from_xrgb_async(hip.ctx, t, SC.ptr(b["src"]), SW, SH, N, U.BILINEAR, DW, DH, SC.ptr(b["table"]), SC.ptr(b["dst"]),
                                                      hip._stream()))
    return SC.Case("tensor_from_xrgb-" + TC.NAMES[t], sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"dst": (sets[0][1]["dst"].shape, TC.BITS[t])}, call)


@functools.lru_cache(maxsize=None)
def source_case(t):
    mean, std = TC.NORMS["imagenet"]
    a, b = TC.coefficients(mean, std)
    ab = (C.c_float * 6)(*a.tolist(), *b.tolist())
    sets = []
    for seed in (292, 293):
        pix = np.random.default_rng(seed).integers(0, 1 << 24, (N, DH, DW), dtype=np.uint32)
        bits = TC.from_packed(TC.table(t, mean, std), pix)                                         # a clip whose reading is its pixels
        out = TC.to_packed(t, bits, mean, std)
        assert (out == pix).all()
        sets.append(({"src": bits}, {"dst": out}))

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_tensor_to_xrgb_async(hip.ctx, t, SC.ptr(b["src"]), DW * DH, N, ab, SC.ptr(b["dst"]), hip._stream()))
    return SC.Case("tensor_to_xrgb-" + TC.NAMES[t], sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"dst": ((N, DH, DW), np.uint32)}, call)


CASES = {"sink-f16": lambda: sink_case(TC.F16), "sink-f32": lambda: sink_case(TC.F32), "source-bf16": lambda: source_case(TC.BF16),
         "source-f32": lambda: source_case(TC.F32)}


def test_the_cases_tell_the_real_inputs_from_the_decoy():
    """(on the CPU's terms, as tests/test_stream_cases_cpu.py asks of the registered cases)"""
    for name in sorted(CASES):
        c = CASES[name]()
        for k in c.compared():
            assert SC.differs(c.exp_real[k], c.exp_decoy[k]), name
            for fill in (SC.SENT, SC.EARLY):
                assert SC.differs(c.exp_real[k], SC.sent(c.exp_real[k].shape, c.exp_real[k].dtype, fill)), name
        for k in c.real:
            assert (c.real[k] != c.decoy[k]).any(), name


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
@pytest.mark.parametrize("name", sorted(CASES))
def test_late_input(name, state, delay, side):
    import torch
    from libagmv_amd import AgmvHip
    case = CASES[name]()
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
    """AgmvHip.tensor_from_xrgb_async(..., stream=side) from the null stream: the same late-input run with the stream passed, not current"""
    import torch
    from libagmv_amd import AgmvHip
    case = sink_case(TC.F16)
    hip = AgmvHip(0)
    try:
        run = SC.Late(case)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            run.arrive(delay)
        assert side.query() is False, "premise: the stream is idle before the call (delay too short)"
        hip.tensor_from_xrgb_async("f16", run.b["src"].reshape(-1), SW, SH, N, run.b["table"], run.b["dst"], U.BILINEAR, DW, DH, stream=side)
        assert side.query() is False, "tensor_from_xrgb_async returned with the caller's stream idle"
        with torch.cuda.stream(side):
            run.leave()
        side.synchronize()
        assert run.verdict() is None, run.verdict()
    finally:
        torch.cuda.synchronize()
        hip.close()
