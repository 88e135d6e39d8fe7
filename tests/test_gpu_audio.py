"""agmv_hip_audio_compand_async / agmv_hip_audio_expand_async against the numpy statement of tests/audio_cases.py: every sample
value and every code, the three layouts at sample counts around the kernels' 16-sample unit, 1 to 6 channels, pointers one element
off their 16-byte boundary (the scalar head), tracks longer than one pass of the capped grid (both loops of every kernel go round a
second time), canary bytes on both sides of every output, the float rule's edge values, the round trip and the refusals.  Expected values never come from the GPU.  Needs an MI355X."""
import itertools

import numpy as np
import pytest

import audio_cases as A

pytestmark = pytest.mark.gpu

PAD, CANARY = 32, 0xA5                             # elements of the output's type on either side; torch's allocations are 16-byte aligned
OUT_DTYPE = {A.PCM_S16: np.uint16, A.PCM_U8: np.uint8, A.PCM_F32P: np.uint32}      # (floats are compared as their bits)
COUNTS_F32P = A.COUNTS + (1028, 4100)              # samples_per_channel % 4 == 0: the planes can be read 16 bytes at a time


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    torch.cuda.synchronize()
    h.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}[a.dtype]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def launch(hip, expanding, fmt, src, channels, n, off=0, out_off=None):
    """src: the flat input as uint16 / uint8 / uint32 (float bits) for a compand, uint8 codes for an expand.  The input pointer is
    moved `off` elements off its base, the output pointer out_off elements (None: as many).  -> (rc, flat output, the canaries
    are intact)"""
    import torch
    out_dtype = OUT_DTYPE[fmt] if expanding else np.uint8
    total = n * channels
    out_off = off if out_off is None else out_off
    d_in = dev(np.concatenate([np.zeros(off, src.dtype), src]))
    host = np.full(PAD + out_off + total + PAD, CANARY, np.uint8).repeat(np.dtype(out_dtype).itemsize).view(out_dtype)
    d_out = dev(host)
    fn = hip.L.agmv_hip_audio_expand_async if expanding else hip.L.agmv_hip_audio_compand_async
    rc = fn(hip.ctx, fmt, d_in[off:].data_ptr(), channels, n, d_out[PAD + out_off:].data_ptr(), hip._stream())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(out_dtype)
    lo, hi = got[:PAD + out_off], got[PAD + out_off + total:]
    intact = bool((lo.view(np.uint8) == CANARY).all() and (hi.view(np.uint8) == CANARY).all())
    return rc, got[PAD + out_off:PAD + out_off + total].copy(), intact


def test_compand_every_sample_value(hip):
    s = np.arange(65536, dtype=np.uint16)
    rc, got, intact = launch(hip, False, A.PCM_S16, s, 1, 65536)
    assert rc == 0 and intact and (got == A.compand(s)).all(), np.flatnonzero(got != A.compand(s))[:8]


def test_expand_every_code(hip):
    c = np.arange(256, dtype=np.uint8)
    rc, got, intact = launch(hip, True, A.PCM_S16, c, 1, 256)
    assert rc == 0 and intact and (got == A.expand(c)).all()
    rc, got, intact = launch(hip, True, A.PCM_F32P, c, 1, 256)
    assert rc == 0 and intact and (got == A.to_f32(A.expand(c)).view(np.uint32)).all()


def pcm_of(fmt, n, channels, seed):
    """(the flat device input, the track's uint16 / uint8 in track order [n, channels]) of a seeded clip in the layout fmt"""
    rng = np.random.default_rng(seed)
    if fmt == A.PCM_U8:
        x = rng.integers(0, 256, (n, channels)).astype(np.uint8)
        return x.reshape(-1), x
    if fmt == A.PCM_S16:
        x = rng.integers(0, 65536, (n, channels)).astype(np.uint16)
        k = min(4, x.size)
        x.reshape(-1)[:k] = (0, 65535, 65281, 255)[:k]
        return x.reshape(-1), x
    x = rng.uniform(-1.05, 1.05, (channels, n)).astype(np.float32)
    return x.reshape(-1).view(np.uint32), A.from_f32(x).T.copy()


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("channels", A.CHANNELS)
@pytest.mark.parametrize("fmt", (A.PCM_S16, A.PCM_U8, A.PCM_F32P), ids=("s16", "u8", "f32p"))
def test_edges_and_layouts(hip, fmt, channels, off):
    for n in (COUNTS_F32P if fmt == A.PCM_F32P else A.COUNTS):
        src, track = pcm_of(fmt, n, channels, 100 * n + channels)
        codes = track.reshape(-1) if fmt == A.PCM_U8 else A.compand(track).reshape(-1)
        rc, got, intact = launch(hip, False, fmt, src, channels, n, off)
        assert rc == 0 and intact, (n, "compand wrote outside its output" if rc == 0 else hip.L.agmv_hip_last_error())
        assert (got == codes).all(), (n, np.flatnonzero(got != codes)[:8])
        # and back, from seeded codes of their own
        c = np.random.default_rng(n + 7).integers(0, 256, (n, channels)).astype(np.uint8)
        want = {A.PCM_S16: lambda: A.expand(c).reshape(-1), A.PCM_U8: lambda: c.reshape(-1),
                A.PCM_F32P: lambda: A.to_f32(A.expand(c)).T.copy().reshape(-1).view(np.uint32)}[fmt]()
        rc, got, intact = launch(hip, True, fmt, c.reshape(-1), channels, n, off)
        assert rc == 0 and intact, (n, "expand wrote outside its output" if rc == 0 else hip.L.agmv_hip_last_error())
        assert (got == want).all(), (n, np.flatnonzero(got != want)[:8])


# (channels, elements the planes are moved by, bytes the codes are moved by, the head that brings both to 16-byte boundaries):
# different phases that one head satisfies, so the planar kernels run a non-zero head, the body and a tail with several channels
PHASES = ((2, 1, 2, 7), (3, 3, 13, 1), (4, 2, 8, 2), (6, 1, 14, 3))


@pytest.mark.parametrize("channels,plane_off,code_off,head", PHASES)
def test_planar_head_and_body_with_several_channels(hip, channels, plane_off, code_off, head):
    assert (4 * (plane_off + head)) % 16 == 0 and (code_off + head * channels) % 16 == 0 and 0 < head < 16
    assert not any((4 * (plane_off + h)) % 16 == 0 and (code_off + h * channels) % 16 == 0 for h in range(head))
    for n in (64, 1028, 4100):                                                     # n % 4 == 0: every plane keeps the phase of the first
        src, track = pcm_of(A.PCM_F32P, n, channels, 7 * n + channels)
        rc, got, intact = launch(hip, False, A.PCM_F32P, src, channels, n, plane_off, code_off)
        want = A.compand(track).reshape(-1)
        assert rc == 0 and intact and (got == want).all(), (n, np.flatnonzero(got != want)[:8])
        c = np.random.default_rng(n + channels).integers(0, 256, (n, channels)).astype(np.uint8)
        rc, got, intact = launch(hip, True, A.PCM_F32P, c.reshape(-1), channels, n, code_off, plane_off)
        want = A.to_f32(A.expand(c)).T.copy().reshape(-1).view(np.uint32)
        assert rc == 0 and intact and (got == want).all(), (n, np.flatnonzero(got != want)[:8])


# ---- tracks longer than one pass of the capped grid: the second trip of the unit loop and of the edge loop ----
AUD_MAX_BLOCKS, AUD_T = 2048, 256                  # the kernels' grid cap and workgroup size, restated
CAP = AUD_MAX_BLOCKS * AUD_T                       # lanes of the largest grid: a loop of more iterations goes round a second time
LONG = 16 * CAP + 16 * 300 + 5                     # samples: 300 units past the cap, and a tail


def cut(n, pcm_off, pcm_step, plane_bytes, planes, code_off, code_step):
    """(head, units) of a track of n samples per channel by the kernels' rule, restated: the smallest head below 16 that brings the
    codes and every plane to a 16-byte boundary (offsets in bytes from one), else the whole track is head"""
    for h in range(16):
        if h + 16 <= n and (code_off + h * code_step) % 16 == 0 and all((pcm_off + c * plane_bytes + h * pcm_step) % 16 == 0 for c in range(planes)):
            return h, (n - h) // 16
    return n, 0


def every_code(track):
    """A.compand through its table over all 65536 sample values"""
    return A.compand(np.arange(65536, dtype=np.uint16))[track]


def both_ways(hip, fmt, channels, n, pcm_off, code_off, seed):
    """a compand and an expand of n samples per channel with the PCM pointer pcm_off elements and the codes code_off bytes off a
    16-byte boundary, against the statement, canaries included"""
    src, track = pcm_of(fmt, n, channels, seed)
    rc, got, intact = launch(hip, False, fmt, src, channels, n, pcm_off, code_off)
    want = every_code(track).reshape(-1)
    assert rc == 0 and intact, "compand wrote outside its output" if rc == 0 else hip.L.agmv_hip_last_error()
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    c = np.random.default_rng(seed + 1).integers(0, 256, (n, channels)).astype(np.uint8)
    rc, got, intact = launch(hip, True, fmt, c.reshape(-1), channels, n, code_off, pcm_off)
    samples = A.expand(np.arange(256, dtype=np.uint8))                              # A.expand through its table over all 256 codes
    want = samples[c].reshape(-1) if fmt == A.PCM_S16 else A.to_f32(samples)[c].T.copy().reshape(-1).view(np.uint32)
    assert rc == 0 and intact, "expand wrote outside its output" if rc == 0 else hip.L.agmv_hip_last_error()
    assert (got == want).all(), np.flatnonzero(got != want)[:8]


def test_the_edge_loop_goes_round_twice_s16(hip):
    """600 001 mono samples, the PCM pointer one sample off its boundary and the codes on theirs: no head serves both, so the whole
    track goes one sample per lane, more samples than the capped grid has lanes"""
    n = 600001
    assert cut(n, 2, 2, 0, 1, 0, 1) == (n, 0) and n > CAP
    both_ways(hip, A.PCM_S16, 1, n, 1, 0, 41)


def test_the_edge_loop_goes_round_twice_f32p(hip):
    """3 planes of 200 001 samples: n % 4 != 0, the planes cannot all lie on 16-byte boundaries, the whole track is head"""
    n, ch = 200001, 3
    assert cut(n, 0, 4, 4 * n, ch, 0, ch) == (n, 0) and n * ch > CAP
    both_ways(hip, A.PCM_F32P, ch, n, 0, 0, 43)


@pytest.mark.parametrize("off,head", ((0, 0), (1, 15)))
def test_the_unit_loop_goes_round_twice_s16(hip, off, head):
    """mono, both pointers `off` elements off their boundaries: a head of 0 or of 15 samples, more units than the grid has lanes, a tail"""
    h, units = cut(LONG, 2 * off, 2, 0, 1, off, 1)
    assert h == head and units > CAP and 0 < LONG - h - 16 * units < 16
    both_ways(hip, A.PCM_S16, 1, LONG, off, off, 45 + off)


def test_the_unit_loop_goes_round_twice_f32p(hip):
    """2 planes in the first phase of PHASES: head 7, more units than the grid has lanes, a tail of 5.  The planes keep one phase
    only where n % 4 == 0, so the count is LONG + 7"""
    channels, plane_off, code_off, head = PHASES[0]
    n = LONG + 7
    assert (channels, head) == (2, 7) and n % 4 == 0
    h, units = cut(n, 4 * plane_off, 4, 4 * n, channels, code_off, channels)
    assert h == head and units > CAP and n - h - 16 * units == 5
    both_ways(hip, A.PCM_F32P, channels, n, plane_off, code_off, 47)


def test_float_rule(hip):
    x = A.float_cases()
    x = np.concatenate([x, np.zeros(-len(x) % 4, np.float32)])                    # whole 16-byte groups: the vector body runs
    want = A.compand(A.from_f32(x))
    assert A.from_f32(np.float32(np.nan)) == 0 and A.from_f32(np.float32(np.inf)) == 32767 and A.from_f32(np.float32(-7)) == np.uint16(-32767 & 0xFFFF)
    for off in (0, 1):                                                             # body and scalar path
        rc, got, intact = launch(hip, False, A.PCM_F32P, x.view(np.uint32), 1, len(x), off)
        assert rc == 0 and intact and (got == want).all(), (off, x[np.flatnonzero(got != want)[:8]])
    two = x[:len(x) // 8 * 8].reshape(2, -1)                                       # two planes of a multiple of 4 samples
    rc, got, intact = launch(hip, False, A.PCM_F32P, two.reshape(-1).view(np.uint32), 2, two.shape[1])
    assert rc == 0 and intact and (got.reshape(-1, 2) == A.compand(A.from_f32(two)).T).all()


@pytest.mark.parametrize("channels", (1, 2, 5))
def test_round_trip(hip, channels):
    n = 4100
    src, track = pcm_of(A.PCM_S16, n, channels, 31)
    rc, codes, _ = launch(hip, False, A.PCM_S16, src, channels, n)
    rc2, back, _ = launch(hip, True, A.PCM_S16, codes, channels, n)
    assert rc == 0 and rc2 == 0 and (back == A.expand(A.compand(track)).reshape(-1)).all()
    assert int(np.abs(back.astype(np.int64) - src.astype(np.int64)).max()) <= 256
    srcf, trackf = pcm_of(A.PCM_F32P, n, channels, 32)
    rc, codes, _ = launch(hip, False, A.PCM_F32P, srcf, channels, n)
    rc2, back, _ = launch(hip, True, A.PCM_F32P, codes, channels, n)
    assert rc == 0 and rc2 == 0 and (back == A.to_f32(A.expand(A.compand(trackf))).T.copy().reshape(-1).view(np.uint32)).all()


def test_wrappers(hip):
    import torch
    pcm = A.tone(3000, 2)
    d = torch.from_numpy(pcm).cuda()
    codes = hip.audio_compand("s16", d)
    back = hip.audio_expand("s16", codes)
    planar = hip.audio_expand("f32p", codes)
    torch.cuda.synchronize()
    want = A.compand(pcm.view(np.uint16))
    assert (codes.cpu().numpy() == want).all() and (back.cpu().numpy().view(np.uint16) == A.expand(want)).all()
    assert planar.shape == (2, 3000) and (planar.cpu().numpy() == A.to_f32(A.expand(want)).T).all()
    f = torch.from_numpy(A.to_f32(pcm.view(np.uint16)).T.copy()).cuda()
    assert (hip.audio_compand("f32p", f).cpu().numpy() == A.compand(A.from_f32(f.cpu().numpy())).T).all()
    with pytest.raises(ValueError):
        hip.audio_compand("s16", f)


def test_refusals_write_nothing(hip):
    import torch
    n = 64
    d_in, d_out = dev(np.zeros(8 * n, np.uint32)), dev(np.full(8 * n * 4, CANARY, np.uint8))
    L, s = hip.L, hip._stream()
    bad = [(0, 2, d_in.data_ptr(), d_out.data_ptr()), (4, 2, d_in.data_ptr(), d_out.data_ptr()),          # no AGMV_PCMFMT
           (A.PCM_S16, 0, d_in.data_ptr(), d_out.data_ptr()), (A.PCM_U8, 0, d_in.data_ptr(), d_out.data_ptr()),   # zero channels
           (A.PCM_F32P, 9, d_in.data_ptr(), d_out.data_ptr()),                                           # more than 8 planes
           (A.PCM_S16, 2, None, d_out.data_ptr()), (A.PCM_S16, 2, d_in.data_ptr(), None),                # NULL
           (A.PCM_S16, 2, d_in.data_ptr() + 1, d_out.data_ptr()), (A.PCM_F32P, 2, d_in.data_ptr() + 2, d_out.data_ptr())]   # a sample astride its alignment
    for (fmt, ch, pcm, codes), fn in itertools.product(bad, (L.agmv_hip_audio_compand_async, L.agmv_hip_audio_expand_async)):
        rc = fn(hip.ctx, fmt, pcm, ch, n, codes, s) if fn is L.agmv_hip_audio_compand_async else fn(hip.ctx, fmt, codes, ch, n, pcm, s)
        assert rc < 0 and L.agmv_hip_last_error(), (fmt, ch)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == CANARY).all() and not d_in.cpu().numpy().any()
    assert L.agmv_hip_audio_compand_async(hip.ctx, A.PCM_S16, d_in.data_ptr(), 2, 0, d_out.data_ptr(), s) == 0      # nothing to do is no error
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == CANARY).all()
