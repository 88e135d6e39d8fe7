"""agmv_hip_tensor_from_xrgb_async and agmv_hip_tensor_to_xrgb_async (include/agmv_hip.h, "normalised float tensor clips"): the
decoder's sink as a table look-up, with and without a scale, and the encoder's source by the reading rule, against the numpy
statement of tests/tensor_cases.py (and tests/upscale_cases.py for the scale).  Everything is compared as bit patterns; no
expectation comes from the GPU.  A lane of the sink forms 16 target pixels of a row and stores them per plane with 16-byte stores
where the width is a multiple of 16 and the planes lie on 16-byte boundaries; a lane of the source owns 8 pixels and loads them
with 16-byte loads where the planes allow; every other clip goes element by element, to the same result: the shapes and the
bases one element off a boundary hold both paths and their edges.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import tensor_cases as TC
import upscale_cases as U
from test_gpu_upscale import BANDS

pytestmark = pytest.mark.gpu

GUARD = 64                                       # bytes on either side of the target
N = 3
IMAGENET = TC.NORMS["imagenet"]
IDS = [TC.NAMES[t] for t in TC.TYPES]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    return torch


@pytest.fixture(scope="module")
def hip(torch):
    from libagmv_amd import AgmvHip
    h = AgmvHip(0)
    yield h
    h.close()


def source(sw, sh, seed, n=N):
    """random pixels with bits >= 24 set: they are no pixels"""
    return np.random.default_rng(seed).integers(0, 1 << 32, (n, sh, sw), dtype=np.uint32) | np.uint32(0x80000000)


def dev(torch, a):
    """an ndarray's bytes as a device tensor"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def sink(torch, hip, t, pix, tab, filt=0, dw=None, dh=None, off=0):
    """-> (the target's bit patterns [n, 3, dh, dw]; whether the guard bytes on either side kept their value).  off: elements"""
    n, sh, sw = pix.shape
    dw, dh = dw or sw, dh or sh
    es = np.dtype(TC.BITS[t]).itemsize
    lo = GUARD + off * es
    nb = n * 3 * dw * dh * es
    buf = torch.full((lo + nb + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    src, d_tab = dev(torch, pix), dev(torch, tab)
    assert buf.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0 and d_tab.data_ptr() % 16 == 0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = hip.L.agmv_hip_tensor_from_xrgb_async(hip.ctx, t, src.data_ptr(), sw, sh, n, filt, dw, dh, d_tab.data_ptr(), buf.data_ptr() + lo, s)
    assert rc == 0, hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[lo:lo + nb].view(TC.BITS[t]).reshape(n, 3, dh, dw), bool((host[:lo] == 0x5A).all() and (host[lo + nb:] == 0x5A).all())


# ---- the sink without a scale ----------------------------------------------------------------------------------------
PLAIN = [(16, 4), (48, 8), (20, 12), (4, 4)]     # one group of 16; three; a width that is no multiple of 16; less than one group


@pytest.mark.parametrize("t", TC.TYPES, ids=IDS)
@pytest.mark.parametrize("wh", PLAIN, ids=["%dx%d" % s for s in PLAIN])
def test_the_sink_is_the_table_applied(torch, hip, wh, t):
    """3 frames; the target on a 16-byte boundary and one element off it: the same elements, nothing else written"""
    w, h = wh
    pix = source(w, h, 100 * w + t)
    tab = TC.table(t, *IMAGENET)
    exp = TC.from_packed(tab, pix)
    for off in (0, 1):
        got, guards = sink(torch, hip, t, pix, tab, off=off)
        assert (got == exp).all(), (wh, off, np.argwhere(got != exp)[:4])
        assert guards, (wh, off, "guard bytes written")


@pytest.mark.parametrize("t", TC.TYPES, ids=IDS)
def test_the_kernel_gathers_and_computes_nothing(torch, hip, t):
    """a table of random bit patterns, NaN patterns of every kind and both infinities included, comes out as it is"""
    rng = np.random.default_rng(40 + t)
    tab = rng.integers(0, 1 << 32, (3, 256), dtype=np.uint64).astype(TC.BITS[t])
    special = [0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000] if t == TC.F32 else \
              [0x7E00, 0x7C01, 0xFFFF, 0x7C00, 0xFC00, 0x0001, 0x8000, 0x7FC0, 0x7F81, 0x7F80, 0xFF80]
    for c in range(3):
        tab[c, 5 * c:5 * c + len(special)] = special
    for w, h in ((48, 8), (20, 12)):
        pix = source(w, h, 7 * w)
        pix[0, 0, :16] = np.arange(16, dtype=np.uint32) * 0x010101 | 0xFF000000       # the special entries are reached
        got, guards = sink(torch, hip, t, pix, tab)
        assert (got == TC.from_packed(tab, pix)).all() and guards


# ---- the sink with a scale -------------------------------------------------------------------------------------------
SCALED = U.SHAPES + BANDS


@pytest.mark.parametrize("t", (TC.F16, TC.F32), ids=["f16", "f32"])
@pytest.mark.parametrize("filt", (U.NEAREST, U.BILINEAR), ids=["nearest", "bilinear"])
@pytest.mark.parametrize("shape", SCALED, ids=[U.shape_id(s) for s in SCALED])
def test_the_scaled_sink_is_the_table_applied_to_the_scaled_clip(torch, hip, shape, filt, t):
    sw, sh, dw, dh = shape
    pix = source(sw, sh, 1000 * t + dw + dh)
    tab = TC.table(t, *IMAGENET)
    exp = TC.from_packed(tab, U.scale(filt, pix, dw, dh))
    for off in (0, 1):
        got, guards = sink(torch, hip, t, pix, tab, filt, dw, dh, off)
        assert (got == exp).all(), (shape, off, np.argwhere(got != exp)[:4])
        assert guards, (shape, off, "guard bytes written")


# the taps divided in 64 bits (U.WIDE_INDEX): the band kernel with 4-byte and 2-byte elements, and the per-pixel one
WIDE_INDEX = [((70001, 1, 40000, 2), U.BILINEAR, TC.F32), ((70001, 1, 40000, 2), U.BILINEAR, TC.F16), ((70001, 1, 40001, 3), U.NEAREST, TC.BF16)]


@pytest.mark.parametrize("shape,filt,t", WIDE_INDEX, ids=["%s-%s-%s" % (U.shape_id(s), U.FILTER_NAMES[f], TC.NAMES[t]) for s, f, t in WIDE_INDEX])
def test_the_scaled_sink_with_taps_divided_in_64_bits(torch, hip, shape, filt, t):
    sw, sh, dw, dh = shape
    assert U.axes_small(shape) == (False, True) and dict(U.WIDE_INDEX)[shape] == (False, True)
    pix = source(sw, sh, 1000 * t + dw + dh)
    tab = TC.table(t, *IMAGENET)
    exp = TC.from_packed(tab, U.scale(filt, pix, dw, dh))
    got, guards = sink(torch, hip, t, pix, tab, filt, dw, dh)
    assert (got == exp).all(), (shape, np.argwhere(got != exp)[:4])
    assert guards, (shape, "guard bytes written")


def test_the_sink_wrapper_on_many_blocks(torch, hip):
    """AgmvHip.tensor_from_xrgb_async on 2 frames of 320 x 240 -> 224 x 224 F16 and 640 x 360 BF16: many blocks per frame"""
    pix = source(320, 240, 5, n=2)
    src = torch.from_numpy(pix.view(np.int32)).cuda()
    for name, dtype, (dw, dh), filt in (("f16", torch.float16, (224, 224), U.BILINEAR), ("bf16", torch.bfloat16, (640, 360), U.NEAREST)):
        tab = TC.table(TC.TYPES[("f32", "f16", "bf16").index(name)], *IMAGENET)
        out = torch.empty((2, 3, dh, dw), dtype=dtype, device="cuda")
        hip.tensor_from_xrgb_async(name, src, 320, 240, 2, dev(torch, tab), out, filt, dw, dh)
        torch.cuda.synchronize()
        got = out.view(torch.int16).cpu().numpy().view(np.uint16)
        assert (got == TC.from_packed(tab, U.scale(filt, pix, dw, dh))).all()


# ---- the source --------------------------------------------------------------------------------------------------------
def read(torch, hip, t, bits, mean, std, off=0):
    """bits [n, 3, npx] -> uint32 [n, npx] through the kernel; the source starts `off` elements behind a 16-byte boundary"""
    n, _, npx = bits.shape
    es = bits.dtype.itemsize
    buf = torch.zeros(16 + off * es + bits.nbytes, dtype=torch.uint8, device="cuda")
    buf[16 + off * es:] = dev(torch, bits)
    out = torch.full((GUARD + n * npx * 4 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    a, b = TC.coefficients(mean, std)
    ab = (C.c_float * 6)(*a.tolist(), *b.tolist())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = hip.L.agmv_hip_tensor_to_xrgb_async(hip.ctx, t, buf.data_ptr() + 16 + off * es, npx, n, ab, out.data_ptr() + GUARD, s)
    assert rc == 0, hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:GUARD] == 0x5A).all() and (host[-GUARD:] == 0x5A).all(), "guard bytes written"
    return host[GUARD:-GUARD].view(np.uint32).reshape(n, npx)


def check_source(torch, hip, t, bits, norms=("identity", "imagenet")):
    for norm in norms:
        mean, std = TC.NORMS[norm]
        exp = TC.to_packed(t, bits[:, :, None, :], mean, std)[:, 0]
        for off in (0, 1):
            got = read(torch, hip, t, bits, mean, std, off)
            bad = np.argwhere(got != exp)
            assert not len(bad), (norm, off, bad[:4], [hex(int(bits[i, 0, k])) for i, k in bad[:4]], got[got != exp][:4], exp[got != exp][:4])


@pytest.mark.parametrize("t", (TC.F16, TC.BF16), ids=["f16", "bf16"])
def test_the_source_over_all_65536_bit_patterns(torch, hip, t):
    """one frame of 256 x 256 per type: every pattern in every channel, each channel in another order"""
    every = np.arange(65536, dtype=np.uint16)
    rng = np.random.default_rng(t)
    bits = np.stack([every, every[::-1], rng.permutation(every)])[None]
    check_source(torch, hip, t, bits)


def f32_inputs():
    rng = np.random.default_rng(32)
    parts = [TC.widen(TC.F32, TC.table(TC.F32, *TC.NORMS[n])).reshape(-1) for n in sorted(TC.NORMS)]            # the table values of four normalisations
    ties = np.arange(256, dtype=np.float32) + np.float32(0.5)
    parts += [ties, ties / np.float32(255), -ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(300))]
    parts.append(np.array([0.0, -0.0, np.inf, -np.inf, 3e38, -3e38, 1.0, -1.0, 255.0, 256.0], np.float32))
    special = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,                 # NaNs, quiet and signalling
                        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00800000, 0x80800000], np.uint32)      # subnormals and the smallest normals
    x = np.concatenate([np.concatenate(parts).view(np.uint32), special, rng.integers(0, 0x00800000, 512, dtype=np.uint32),
                        rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint32)])
    return x


def test_the_source_on_float32(torch, hip):
    x = f32_inputs()
    x = x[:len(x) // 8 * 8]                                          # planes of a multiple of 4 elements: the 16-byte loads
    rng = np.random.default_rng(33)
    bits = np.stack([x, x[::-1], rng.permutation(x)])[None]
    assert bits.shape[2] % 8 == 0 and bits.shape[2] > 1 << 20
    check_source(torch, hip, TC.F32, bits)


@pytest.mark.parametrize("t", TC.TYPES, ids=IDS)
def test_the_source_on_frames_that_are_no_multiple_of_four_elements(torch, hip, t):
    """3 frames of 2051 pixels (a full block of 2048 and a partial group), of 12 (16-byte planes for F32 only) and of 5"""
    rng = np.random.default_rng(50 + t)
    for npx in (2051, 12, 5):
        if t == TC.F32:
            vals = rng.uniform(-0.2, 1.2, (N, 3, npx)).astype(np.float32)
            vals.reshape(-1)[::7] = f32_inputs()[:len(vals.reshape(-1)[::7])].view(np.float32)
            bits = vals.view(np.uint32)
        else:
            bits = rng.integers(0, 1 << 16, (N, 3, npx), dtype=np.uint16)
        check_source(torch, hip, t, bits, norms=("imagenet",))


def test_the_source_wrapper_reads_what_the_sink_wrote(torch, hip):
    """both wrappers on torch tensors of the three dtypes: 2 frames of 64 x 48 come back as they were (bits >= 24 cleared)"""
    pix = source(64, 48, 9, n=2)
    src = torch.from_numpy(pix.view(np.int32)).cuda()
    for name, dtype in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        mean, std = TC.NORMS["imagenet"]
        out = torch.empty((2, 3, 48, 64), dtype=dtype, device="cuda")
        from libagmv_amd import hip as H
        hip.tensor_from_xrgb_async(name, src, 64, 48, 2, dev(torch, H.tensor_table(name, mean, std)), out)
        a, b = TC.coefficients(mean, std)
        back = hip.tensor_to_xrgb_async(name, out, 64 * 48, 2, a.tolist() + b.tolist())
        torch.cuda.synchronize()
        assert (back.cpu().numpy().view(np.uint32).reshape(2, 48, 64) == pix & 0xFFFFFF).all(), name


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_no_frames_and_refusals_launch_nothing(torch, hip):
    src = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
    tab = torch.zeros(768, dtype=torch.int32, device="cuda")
    dst = torch.full((12 * 64 * 64,), 0x5A, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sink_call, src_call = hip.L.agmv_hip_tensor_from_xrgb_async, hip.L.agmv_hip_tensor_to_xrgb_async

    def to_tensor(ctx=hip.ctx, t=TC.F16, src=src.data_ptr(), sw=16, sh=16, n=1, filt=U.BILINEAR, dw=32, dh=32, tab=tab.data_ptr(), dst=dst.data_ptr()):
        return sink_call(ctx, t, src, sw, sh, n, filt, dw, dh, tab, dst, s)
    bad = [dict(t=0), dict(t=4), dict(t=16), dict(filt=U.AREA), dict(filt=U.AREA, dw=8, dh=8), dict(filt=2, dw=16, dh=16), dict(filt=4), dict(filt=-1),
           dict(filt=0), dict(filt=0, dw=16),                                                                     # filter 0 does not scale
           dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(dw=1 << 15, dh=(1 << 13) + 1), dict(sw=1 << 15, sh=(1 << 13) + 1),
           dict(src=None), dict(tab=None), dict(dst=None), dict(dst=dst.data_ptr() + 1), dict(t=TC.F32, dst=dst.data_ptr() + 2), dict(src=src.data_ptr() + 2)]
    for change in bad:
        assert to_tensor(**change) != 0, change
        assert hip.L.agmv_hip_last_error()
    assert to_tensor(ctx=None) != 0 and b"NULL context" in hip.L.agmv_hip_last_error()
    for filt, dw in ((0, 16), (U.NEAREST, 32), (U.BILINEAR, 32)):
        assert to_tensor(n=0, filt=filt, dw=dw, dh=dw) == 0                                                     # no frames: nothing to do

    ab = (C.c_float * 6)(255, 255, 255, 0, 0, 0)
    out = torch.full((64 * 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")

    def to_xrgb(ctx=hip.ctx, t=TC.F16, src=dst.data_ptr(), npx=64, n=1, ab=ab, out=out.data_ptr()):
        return src_call(ctx, t, src, npx, n, ab, out, s)
    for change in (dict(t=0), dict(t=4), dict(npx=0), dict(npx=(1 << 28) + 1), dict(src=None), dict(ab=None), dict(out=None), dict(src=dst.data_ptr() + 1),
                   dict(t=TC.F32, src=dst.data_ptr() + 2), dict(out=out.data_ptr() + 2)):
        assert to_xrgb(**change) != 0, change
        assert hip.L.agmv_hip_last_error()
    assert to_xrgb(ctx=None) != 0 and b"NULL context" in hip.L.agmv_hip_last_error()
    assert to_xrgb(n=0) == 0
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all()) and bool((out == 0x5A5A5A5A).all())
    with pytest.raises(RuntimeError, match="area"):
        hip.tensor_from_xrgb_async("f16", src, 16, 16, 1, tab, dst, U.AREA, 8, 8)
    with pytest.raises(ValueError, match="fmt"):
        hip.tensor_from_xrgb_async("f64", src, 16, 16, 1, tab, dst)
