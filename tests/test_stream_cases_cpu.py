"""The cases of the late-input harness (tests/stream_cases.py) checked on the CPU: a decoy that gives the same bytes as the real
inputs proves nothing, and a decoy, or a mixture of decoy and real arguments, that is no valid input would turn a wrong-stream
bug into a GPU fault instead of wrong bytes."""
import numpy as np
import pytest

import stream_cases as SC

NAMES = sorted(SC.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_decoy_gives_other_bytes_in_every_output(name):
    c = SC.build(name)
    assert set(c.compared()) <= set(c.exp_real) and set(c.compared()) <= set(c.exp_decoy)
    assert c.compared(), "a case without an output"
    for k in c.compared():
        e, m = SC.parts(c.exp_real[k])
        shape, dtype = c.outputs[k] if k in c.outputs else (c.real[k].shape, c.real[k].dtype)
        assert e.shape == tuple(shape) and e.dtype == dtype, k
        assert m is None or (m.shape == e.shape and m.any()), k
        if k in c.host_determined:                    # a function of the host arguments alone, which stay fixed: shown, not assumed
            assert (e == c.host_determined[k]).all() and (SC.parts(c.exp_decoy[k])[0] == c.host_determined[k]).all(), k
            continue
        assert SC.differs(c.exp_real[k], c.exp_decoy[k]), "%s: %s is the same for the real and the decoy inputs" % (name, k)
        if k in c.inplace:                            # an in-place argument the call leaves as it is proves nothing either
            assert SC.differs(c.exp_real[k], c.real[k]), "%s: %s is not changed by the call" % (name, k)
    for k in c.real:
        assert (c.real[k] != c.decoy[k]).any(), "%s: input %s of the decoy is the real one" % (name, k)
    for k in c.returns:                               # every host value a case returns has an expectation, for both sets
        for exp in (c.exp_real, c.exp_decoy):
            assert k in exp and isinstance(exp[k], (bool, int, SC.Between)), "%s: no expectation for the returned %s" % (name, k)
        if not isinstance(c.exp_real[k], SC.Between):  # an exact one tells the real inputs from the decoy, like an output array
            assert c.exp_real[k] != c.exp_decoy[k], "%s: %s is the same for the real and the decoy inputs" % (name, k)
    assert set(c.exp_real) == set(c.compared()) | set(c.returns) == set(c.exp_decoy), "%s: an expectation nothing is compared with" % name


@pytest.mark.parametrize("name", NAMES)
def test_expectation_is_not_the_fill(name):
    """an output that stays as the harness filled it would pass for a call that never ran"""
    c = SC.build(name)
    for k in c.outputs:
        e, m = SC.parts(c.exp_real[k])
        for fill in (SC.SENT, SC.EARLY):
            assert SC.differs((e, m), SC.sent(e.shape, e.dtype, fill)), "%s: %s expects nothing but 0x%02x" % (name, k, fill)


@pytest.mark.parametrize("name", NAMES)
def test_every_mixture_of_decoy_and_real_is_in_bounds(name):
    c = SC.build(name)
    n = 0
    for inp in c.mixtures():
        c.bounds(inp)
        n += 1
    assert n == 1 << len(c.real)


def test_only_one_output_is_host_determined():
    """the one array no decoy can change: `used` of an LZ77 decode with the sizes in host memory (agmv_lz_decode_mem fetches csize
    bytes whatever they hold, so used = min(csize, avail))"""
    assert {n: sorted(SC.build(n).host_determined) for n in NAMES if SC.build(n).host_determined} == {"lz_decode_sized-pair": ["used3"]}


def test_bounds_checks_can_fail():
    """the bounds checks are live: an argument out of range is refused"""
    for name, key, value in (("gather", "index", 68 * 36), ("pack_frames", "sizes", SC.PK_STRIDE + 1), ("lzss_frames", "sizes", SC.LZ_STRIDE + 1),
                             ("decode_bitstreams-512", "bpos", SC._dec_stride(True) - 15), ("lz_decode+commit-lzss", "off", SC.LZD_SRC)):
        c = SC.build(name)
        inp = {k: v.copy() for k, v in c.real.items()}
        inp[key].reshape(-1)[0] = value
        with pytest.raises(AssertionError):
            c.bounds(inp)


def test_header_entry_points_have_a_case():
    """every *_dev entry point of include/agmv_hip.h is named by the table of tests/test_gpu_streams.py"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "agmv_hip.h")).read()
    table = open(os.path.join(root, "tests", "test_gpu_streams.py")).read().split('"""')[1]
    want = set(re.findall(r"\b(agmv_hip_\w+_dev)\(", header))
    want |= {"agmv_hip_stream_create", "agmv_hip_stream_destroy", "agmv_hip_stream_sync", "agmv_hip_event_create", "agmv_hip_event_destroy",
             "agmv_hip_event_record", "agmv_hip_stream_wait_event", "agmv_hip_host_alloc", "agmv_hip_host_free", "agmv_hip_memcpy_async",
             "agmv_hip_memset_async", "agmv_hip_set_palette", "agmv_hip_check", "agmv_hip_decode_prior_dependent", "agmv_hip_parse_fallback_frames",
             "agmv_hip_lz77_reparsed_segments", "agmv_hip_lz_decode_fallback_frames"}
    assert len(want) > 45
    missing = sorted(n for n in want if n not in table)
    assert not missing, "no late-input case is listed for %s" % ", ".join(missing)
