"""Every device entry point of include/agmv_hip.h on a BUSY non-blocking stream (the late-input harness of tests/stream_cases.py):
the drivers run one hipStreamNonBlocking stream per worker, the kernel-level suite runs everything on an idle null stream, where a
launch on the wrong stream or a missing wait cannot fail.  Here the inputs of a call arrive late on the caller's stream, behind a
bounded delay, and the outputs are snapshotted on that stream alone.

Entry point -> case (tests/stream_cases.py; every case runs warm and on a fresh context).  A new entry point gets a row here
and a case there; tests/test_stream_cases_cpu.py checks that no *_dev entry point of the header is missing from this table.

  agmv_hip_quantise_dev                                  quantise-{512,256}
  agmv_hip_set_palette                                   set_palette+quantise-{512,256}; test_shared_palette_table_is_awaited (lut_share / built)
  agmv_hip_encode_frames_dev                             encode-{512,256}-fc{0,6} (fc6: the ient_both copy-back)
  agmv_hip_encode_entries_dev                            encode_entries-{512,256}-fc{0,6}
  agmv_hip_parse_frames_dev, agmv_hip_decode_frames_dev  parse+decode-{512,256}
  agmv_hip_parse_decode_frames_dev                       parse_decode-{512,256}-slices{1,3} (3: the parser's own stream, ev_fork / ev_slice)
  agmv_hip_decode_bitstreams_dev                         decode_bitstreams-{512,256}
  agmv_hip_decode_prior_dependent, agmv_hip_parse_fallback_frames, agmv_hip_check        decode_stats-512
  agmv_hip_pack_frames_dev, agmv_hip_unpack_frames_dev   pack_frames, unpack_frames
  agmv_hip_lzss_frames_dev                               lzss_frames
  agmv_hip_lz77_peek_dev, agmv_hip_lz77_frames_dev, agmv_hip_lz77_reparsed_segments      lz77_peek+frames
  agmv_hip_lz_decode_frames_dev, agmv_hip_lz_decode_commit_dev, agmv_hip_lz_decode_fallback_frames   lz_decode+commit-{lzss,lz77}
  agmv_hip_lz_decode_frames_sized_dev                    lz_decode_sized-pair (h_stage / ev_up); test_driver_handoff_through_the_c_abi
  agmv_hip_synth_dev, agmv_hip_interp_dev, agmv_hip_histogram_dev, agmv_hip_similarity_dev, agmv_hip_gather_dev
                                                         synth, interp, histogram, similarity, gather
  agmv_hip_pixels_to_xrgb_dev, agmv_hip_pixels_from_xrgb_dev, agmv_hip_gather_fmt_dev, agmv_hip_histogram_fmt_dev,
  agmv_hip_similarity_fmt_dev                            pixels_to_xrgb-rgb24, pixels_from_xrgb-rgba32, gather_fmt-rgb8p, histogram_fmt-rgb24,
                                                         similarity_fmt-rgba32
  agmv_hip_yuv_to_xrgb_dev, agmv_hip_yuv_from_xrgb_dev, agmv_hip_yuv_gather_dev, agmv_hip_yuv_histogram_dev,
  agmv_hip_yuv_similarity_dev                            yuv_to_xrgb-nv12, yuv_from_xrgb-i420, yuv_gather-nv12, yuv_histogram-i420, yuv_similarity-nv12
  agmv_hip_scale_area_dev                                scale_area-{xrgb32,nv12-bt601}-{64x48-to-32x24,7x5-to-3x2}
  agmv_hip_palette_refine_dev                            palette_refine-early_stop, palette_refine-k_1
  agmv_hip_stream_create, agmv_hip_stream_destroy, agmv_hip_stream_sync, agmv_hip_event_create, agmv_hip_event_destroy,
  agmv_hip_event_record, agmv_hip_stream_wait_event, agmv_hip_host_alloc, agmv_hip_host_free, agmv_hip_memcpy_async,
  agmv_hip_memset_async                                  test_driver_handoff_through_the_c_abi

The contract sentences of the header: test_one_context_two_streams_encode, test_two_contexts_on_two_streams.
"""
import ctypes as C

import numpy as np
import pytest

import stream_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def delay():
    """the calibrated delay in cycles of torch.cuda._sleep (printed: run with -s to see it)"""
    import torch
    from libagmv_amd import hip
    hip.load_library()
    assert torch.cuda.is_available()
    return SC.calibrate()


@pytest.fixture(scope="module")
def side(delay):
    """the delayed stream: non-blocking, and on another hardware queue than the null stream (so that a launch on stream 0 does
    not wait for the delay as well)"""
    import torch
    return SC.pick_stream(delay, [torch.cuda.default_stream()])


@pytest.fixture(scope="module")
def second(delay, side):
    """a second stream that runs beside both"""
    import torch
    return SC.pick_stream(delay, [torch.cuda.default_stream(), side])


@pytest.fixture
def contexts():
    """contexts that are closed whatever the test does"""
    from libagmv_amd import AgmvHip
    made = []

    def make():
        made.append(AgmvHip(0))
        return made[-1]
    yield make
    import torch
    torch.cuda.synchronize()
    for c in made:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# the two controls: torch alone, no library code
# ---------------------------------------------------------------------------------------------------------------------
def _copy_case(other):
    """out.copy_(inp) on the caller's stream, or on `other`"""
    import torch
    rng = np.random.default_rng(1)
    real, decoy = ({"inp": rng.integers(0, 256, 5000, dtype=np.uint8)} for _ in range(2))
    wrong_stream = other is not None

    def call(hip, b, side):
        if wrong_stream:
            with torch.cuda.stream(other):
                b["out"].copy_(b["inp"], non_blocking=True)
        else:
            b["out"].copy_(b["inp"], non_blocking=True)
    return SC.Case("control", real, decoy, {"out": real["inp"]}, {"out": decoy["inp"]}, {"out": ((5000,), np.uint8)}, call)


def test_control_correct_caller_passes(delay, side):
    SC.run_late(_copy_case(None), None, delay, side)


@pytest.mark.parametrize("which", ["null", "second"])
def test_control_wrong_stream_is_reported(which, delay, side, second):
    """a caller that copies on ANOTHER stream than the delayed one (the null stream, a stream of its own) reads the decoy, and the
    late fill paints over what it wrote"""
    import torch
    with pytest.raises(AssertionError, match=r"control: out\(\d+,\) is 0xa5"):
        SC.run_late(_copy_case(torch.cuda.default_stream() if which == "null" else second), None, delay, side)


def test_control_host_synchronisation_is_reported(delay, side):
    """a caller that waits for its stream trips the second premise"""
    import torch
    c = _copy_case(None)
    inner = c.call

    def call(hip, b, side):
        inner(hip, b, side)
        torch.cuda.current_stream().synchronize()
    c.call = call
    with pytest.raises(AssertionError, match="caller's stream idle"):
        SC.run_late(c, None, delay, side)


# ---------------------------------------------------------------------------------------------------------------------
# every case, warm and fresh
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["warm", "fresh"])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_late_input(name, state, delay, side, contexts, monkeypatch):
    """warm: after one quiet call of the same shape on the context (nothing allocates); fresh: the first call on a new context
    (work areas, events and first-use memsets happen behind the delay)"""
    import torch
    case = SC.build(name)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    hip = contexts()
    case.setup(hip)
    if state == "warm":
        SC.run_quiet(case, hip)
        torch.cuda.synchronize()
    SC.run_late(case, hip, delay, side, fresh=state == "fresh")
    hip.check()


# ---------------------------------------------------------------------------------------------------------------------
# the sentences of "Notes on a context"
# ---------------------------------------------------------------------------------------------------------------------
def test_shared_palette_table_is_awaited(side, second, contexts):
    """contexts with the same palette share one table: the second context finds it while the first one's build is still running
    on ANOTHER stream, and its quantise must wait for that build (the `built` event on the caller's stream).
    No delay can be put before the build: agmv_hip_set_palette waits for its stream and launches the build kernels in the same
    call.  The premise is therefore the build itself: 2^24 colours against 512 entries (2.1 ms) against the
    two host calls that follow it here (tens of microseconds).  It is asserted: a build that ends first fails the test, it does
    not pass it."""
    import torch
    import oracles as O
    p0, p1 = SC.palettes(2)                                            # a palette no other test sets: the table is built here
    pix = np.random.default_rng(7).integers(0, 1 << 24, 4099, dtype=np.uint32)
    exp = np.zeros(pix.size, np.uint16)
    O.oracle().orc_quantise(p0, p1, 1, pix, pix.size, exp)
    a, b = contexts(), contexts()
    d_pix = SC.to_dev(pix)
    outs = [SC.to_dev(SC.sent((4099,), np.uint16)) for _ in range(2)]
    torch.cuda.synchronize()
    sa, sb = side, second
    building = torch.cuda.Event()
    with torch.cuda.stream(sa):
        a.set_palette(p0, p1, True)
        building.record()
    with torch.cuda.stream(sb):
        b.set_palette(p0, p1, True)
        b._ck(b.L.agmv_hip_quantise_dev(b.ctx, d_pix.data_ptr(), 4099, outs[1].data_ptr(), b._stream()))
        assert building.query() is False, "premise: the first context's table was complete before the second context used it"
        snap_b = outs[1].clone()
    with torch.cuda.stream(sa):
        a._ck(a.L.agmv_hip_quantise_dev(a.ctx, d_pix.data_ptr(), 4099, outs[0].data_ptr(), a._stream()))
        snap_a = outs[0].clone()
    sa.synchronize()
    sb.synchronize()
    assert (SC.to_host(snap_b, np.uint16) == exp).all(), "the second context quantised with a table that was not complete"
    assert (SC.to_host(snap_a, np.uint16) == exp).all()


def test_one_context_two_streams_encode(delay, side, second, contexts):
    """"a second encode is ordered behind the first (on another stream it waits for it through an event)": batch A on the
    delayed stream, batch B (another clip, inside a GOP) on a second stream straight after; both as the oracle encodes them"""
    import torch
    ca, cb = SC.build("encode-512-fc0"), SC.build("encode-512-fc6")
    hip = contexts()
    ca.setup(hip)
    for c in (ca, cb):
        SC.run_quiet(c, hip)
    torch.cuda.synchronize()
    ra, rb = SC.Late(ca), SC.Late(cb, "real")
    a_seen_from_b = {k: torch.empty_like(ra.snap[k]) for k in ca.outputs}   # (its in-place argument gets the decoy back on s1)
    torch.cuda.synchronize()
    s1, s2 = side, second
    with torch.cuda.stream(s1):
        ra.arrive(delay)
        assert s1.query() is False, "premise: the first stream is idle before the call"
        ca.call(hip, ra.b, SC.Probe(s1))
        assert s1.query() is False, "premise: the first stream is idle when the call returns"
        ra.leave()
    with torch.cuda.stream(s2):
        cb.call(hip, rb.b, SC.Probe())
        assert s1.query() is False, "premise: the first encode was over before the second was enqueued"
        rb.leave(restore=False)
        for k, v in a_seen_from_b.items():                             # ordered behind the first: its outputs are complete HERE
            v.copy_(ra.b[k], non_blocking=True)
    s2.synchronize()
    s1.synchronize()
    assert ra.verdict() is None, ra.verdict()
    assert rb.verdict(cb.exp_real) is None, rb.verdict(cb.exp_real)
    ra.snap = a_seen_from_b
    assert ra.verdict() is None, "the second stream did not wait for the first encode: " + ra.verdict()
    hip.check()


STAGES = ["encode", "decode_bitstreams", "lz77", "lz_decode", "palette_refine"]


def _stage_case(stage, pal):
    if stage == "encode":
        return SC._encode(True, 6, False, pal)
    if stage == "decode_bitstreams":
        return SC._decode("decode_bitstreams", True, None, pal)
    return SC.build({"lz77": "lz77_peek+frames", "lz_decode": "lz_decode+commit-lzss", "palette_refine": "palette_refine-early_stop"}[stage])


@pytest.mark.parametrize("stage,palettes", [(s, p) for s in STAGES for p in (("same", "different") if s in ("encode", "decode_bitstreams") else ("none",))])
def test_two_contexts_on_two_streams(stage, palettes, side, second, contexts):
    """"use one context per concurrent encoder / decoder": two contexts, each on its own stream, three rounds interleaved; context 0
    runs the real inputs of the case and context 1 the decoy, and each result equals its reference, as it does serially.  The two
    stages that read the palette run with the same one in both contexts (one shared table) and with different ones; the other
    three take none"""
    import torch
    cases = [_stage_case(stage, 0), _stage_case(stage, 1 if palettes == "different" else 0)]
    ctx = [contexts(), contexts()]
    for w in (0, 1):
        if palettes != "none":
            SC.set_palette(True, 1 if w and palettes == "different" else 0)(ctx[w])
    torch.cuda.synchronize()
    streams = [side, second]
    runs = []
    for rnd in range(3):
        for w in (0, 1):
            with torch.cuda.stream(streams[w]):
                runs.append((rnd, w) + SC.run_quiet(cases[w], ctx[w], "decoy" if w else "real"))
    torch.cuda.synchronize()
    for rnd, w, run, exp in runs:
        bad = run.verdict(exp)
        assert bad is None, "round %d, context %d: %s" % (rnd, w, bad)
    for c in ctx:
        c.check()


def test_driver_handoff_through_the_c_abi(delay, contexts):
    """the sequence decoder's handoff, with nothing but the C-ABI helpers: inputs go up from agmv_hip_host_alloc memory with
    agmv_hip_memcpy_async on stream A (which is busy), the LZ stage and its commit run on A, an event hands the rows to stream B,
    which reconstructs the pixels and brings them down.  The pixels are the oracle decoder's."""
    import torch
    import hostlib as HL
    import lz_decode_cases as LZD
    import oracles as O
    import streams as T
    W, H, n = SC.W, SC.H, 9
    p0, p1 = SC.palettes()
    frames = T.clip(np.random.default_rng(77), W, H, n)
    bits = T.encode(W, H, True, p0, p1, frames)
    fr = []
    for x in bits:
        p, cs = HL.lzss(x)
        fr.append(LZD.Frame(p.tobytes(), len(x), cs, avail=len(p) + len(LZD.GUARD)))
    src, off, avail = LZD.image(fr)
    usize, csize = (np.array([getattr(f, k) for f in fr], np.uint32) for k in ("usize", "csize"))
    avail, off = avail.astype(np.uint32), off.astype(np.uint64)
    cap = W * H * 3 + 64                                               # the oracle decoder's persistent buffer
    before, rows, bpos, used, _ = LZD.host_batch(1, fr, cap)
    dec = O.OracleDecoder(W, H, True, p0, p1)
    exp = np.stack([dec.decode(rows[f, :bpos[f]]) for f in range(n)])
    dec.close()

    hip = contexts()
    hip.set_palette(p0, p1, True)
    L, ctx = hip.L, hip.ctx
    d_src, d_off = torch.zeros(len(src), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    d_bits = torch.full((n, cap), 0x11, dtype=torch.uint8, device="cuda")
    d_persist = torch.full((cap,), 0x22, dtype=torch.uint8, device="cuda")
    d_bpos, d_used = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_pix = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    # a quiet run first, so that the busy one allocates nothing
    hip.lz_decode_frames_dev(1, d_src, d_off, avail, usize, csize, n, cap, bits=d_bits, bpos=d_bpos, used=d_used)
    hip.lz_decode_commit_dev(d_bits, d_bpos, n, d_persist)
    hip.decode_bitstreams_dev(d_bits, torch.zeros(n, dtype=torch.int32, device="cuda"), n, W, H, out=d_pix)
    torch.cuda.synchronize()

    sa, sb, ev = L.agmv_hip_stream_create(ctx), L.agmv_hip_stream_create(ctx), L.agmv_hip_event_create(ctx)
    h_src, h_off, h_pix = L.agmv_hip_host_alloc(len(src)), L.agmv_hip_host_alloc(8 * n), L.agmv_hip_host_alloc(4 * n * W * H)
    try:
        assert sa and sb and ev and h_src and h_off and h_pix, hip.L.agmv_hip_last_error()
        C.memmove(h_src, src.ctypes.data, len(src))
        C.memmove(h_off, off.ctypes.data, 8 * n)
        C.memset(h_pix, 0x33, 4 * n * W * H)
        ta = torch.cuda.ExternalStream(sa)
        with torch.cuda.stream(ta):
            torch.cuda._sleep(delay)
        ck = hip._ck
        ck(L.agmv_hip_memcpy_async(ctx, d_src.data_ptr(), h_src, len(src), 0, sa))
        ck(L.agmv_hip_memcpy_async(ctx, d_off.data_ptr(), h_off, 8 * n, 0, sa))
        ck(L.agmv_hip_memset_async(ctx, d_bits.data_ptr(), 0, n * cap, sa))
        ck(L.agmv_hip_memset_async(ctx, d_persist.data_ptr(), 0, cap, sa))         # the fresh decoder's buffer
        ck(L.agmv_hip_memset_async(ctx, d_pix.data_ptr(), SC.SENT, 4 * n * W * H, sb))
        assert ta.query() is False, "premise: stream A is idle before the LZ stage"
        u32p = lambda a: a.ctypes.data_as(C.c_void_p)
        ck(L.agmv_hip_lz_decode_frames_sized_dev(ctx, 1, d_src.data_ptr(), d_off.data_ptr(), u32p(avail), u32p(usize), u32p(csize), n, d_bits.data_ptr(),
                                                 cap, cap, d_bpos.data_ptr(), d_used.data_ptr(), sa))
        ck(L.agmv_hip_lz_decode_commit_dev(ctx, d_bits.data_ptr(), cap, d_bpos.data_ptr(), n, d_persist.data_ptr(), cap, sa))
        assert ta.query() is False, "premise: stream A is idle when the LZ stage returns (it promises no stream synchronisation)"
        ck(L.agmv_hip_event_record(ctx, ev, sa))
        ck(L.agmv_hip_stream_wait_event(ctx, sb, ev))
        ck(L.agmv_hip_decode_bitstreams_dev(ctx, d_bits.data_ptr(), cap, d_bpos.data_ptr(), n, W, H, 0, None, d_pix.data_ptr(), None, None, sb))
        ck(L.agmv_hip_memcpy_async(ctx, h_pix, d_pix.data_ptr(), 4 * n * W * H, 1, sb))
        assert ta.query() is False, "premise: stream A is idle when everything is enqueued"
        ck(L.agmv_hip_stream_sync(ctx, sb))
        assert ta.query() is True, "stream B ended before stream A, whose event it waits for"
        got = np.ctypeslib.as_array(C.cast(h_pix, C.POINTER(C.c_uint32)), (n, W * H)).copy()
        assert (SC.to_host(d_bpos, np.uint32) == bpos).all() and (SC.to_host(d_used, np.uint32) == used).all()
        assert (got == exp).all(), "frames %s differ from the oracle decoder's" % np.flatnonzero((got != exp).any(axis=1))
        hip.check()
    finally:
        torch.cuda.synchronize()
        for s in (sa, sb):
            if s:
                L.agmv_hip_stream_destroy(ctx, s)
        if ev:
            L.agmv_hip_event_destroy(ctx, ev)
        for h in (h_src, h_off, h_pix):
            if h:
                L.agmv_hip_host_free(h)
