"""The late-input harness and its cases (tests/test_gpu_streams.py on the GPU, tests/test_stream_cases_cpu.py on the CPU).

A case is ONE call (or one short sequence of calls) of the device entry points of include/agmv_hip.h with
  real    the device-resident inputs of the call, name -> ndarray;
  decoy   other VALID inputs of the same shapes and dtypes;
  exp     for either set the expected outputs, name -> ndarray or (ndarray, mask): the mask marks what the header defines
          (without one the whole array is compared, so bytes the call must leave alone are expected to hold SENT).
The expectations come from the references the suite already has (the oracle encoder / decoder, the brute-force LZ of the oracle,
the host LZ decode, the numpy statements of the layouts, the scale rule and the palette refinement), never from a GPU call.

run_late() holds the DECOY in the device buffers and lets the real inputs arrive late, on a busy non-blocking stream:
  1. decoy in the inputs, EARLY (0x5A) in the outputs, device synchronised;
  2. on a torch.cuda.Stream() (non-blocking; one that shares no hardware queue with the null stream, pick_stream()): a bounded
     delay (torch.cuda._sleep, calibrated by calibrate()), then copies of the real inputs over the decoy and SENT (0xA5) over
     the outputs, from device tensors prepared before step 1;
  3. the stream must still be busy (query() is False); the library call is made with that stream current;
  4. for a call the header calls asynchronous without qualification the stream must still be busy when it returns;
  5. device-to-device snapshots of every output and in-place argument, then the decoy again over the inputs;
  6. synchronise; the snapshots must equal the expectation for the REAL inputs.
A step of the library that runs on another stream reads the decoy, or has its output painted over by the late SENT fill; work
still running when the caller's stream says it is done misses the snapshot or reads the decoy copied back; a host
synchronisation the header does not promise trips the second query().
"""
import functools

import numpy as np

import lz77_cases as L77
import lz_decode_cases as LZD
import lzss_cases as LZS
import oracles as O
import palette_cases as PC
import pixfmt_cases as PF
import scale_cases as SC
import streams as T
import synth as S
import yuv_cases as Y

SENT, EARLY = 0xA5, 0x5A
W, H = 64, 48                                   # the codec cases: 192 blocks, three rows of 64-block tiles
NBLK = (W // 4) * (H // 4)
W2, H2 = 68, 36                                 # the helper kernels: 2448 pixels, no multiple of 256
NONE = 0xFFFFFFFF                               # a gather index without a source pixel


def sent(shape, dtype, fill=SENT):
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = fill
    return a


@functools.lru_cache(maxsize=None)
def palettes(which=0):
    """two sets of 512 DISTINCT colours: an entry plane painted with its colours quantises back to itself"""
    p0, p1 = S.random_palettes(5 + which)
    assert len(np.unique(np.concatenate([p0, p1]))) == 512 and len(np.unique(p0)) == 256
    return p0, p1


def hip_library():
    """libagmv_hip.so for its host-only functions (they need no GPU), built on demand like the host library of tests/hostlib.py"""
    import hostlib
    from libagmv_amd import hip
    hostlib.lib()
    return hip.load_library()


def max_usize(mode512):
    """agmv_hip_max_usize"""
    return int(hip_library().agmv_hip_max_usize(W, H, int(mode512)))


class Between:
    """the expectation of a returned count for which the suite has no reference: what its definition bounds it by"""

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def holds(self, v):
        return self.lo <= v <= self.hi

    def __repr__(self):
        return "%d .. %d" % (self.lo, self.hi)


class Case:
    """see the module docstring.  call(hip, b, side) makes the library call(s) on torch's current stream with b: name -> device
    tensor (inputs, outputs, scratch) and returns the host values named in `returns`, name -> value, each of which is compared
    with exp[name] (a value, or Between).  setup(hip) runs quietly before (the palette).  asynchronous: assertion 4 applies.
    bounds(inp) asserts on the CPU that a set of inputs (any mixture of real and decoy) is valid.  host_determined: name -> array
    for an output that is a function of the HOST arguments alone, which stay fixed: no decoy can change it."""

    def __init__(self, name, real, decoy, exp_real, exp_decoy, outputs, call, bounds=None, inplace=(), scratch=None, setup=None,
                 asynchronous=True, env=None, host_determined=None, returns=()):
        self.name, self.real, self.decoy, self.exp_real, self.exp_decoy = name, real, decoy, exp_real, exp_decoy
        self.outputs, self.call, self.bounds, self.inplace = outputs, call, bounds or (lambda inp: None), tuple(inplace)
        self.scratch, self.setup, self.asynchronous, self.env = scratch or {}, setup or (lambda hip: None), asynchronous, env or {}
        self.host_determined, self.returns = host_determined or {}, tuple(returns)
        assert set(real) == set(decoy) and all(real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype for k in real)

    def compared(self):
        """the names of the device arrays the GPU test compares"""
        return list(self.outputs) + list(self.inplace)

    def mixtures(self):
        """every choice of real or decoy per input (2^inputs sets; the cases have at most 7 inputs)"""
        names = sorted(self.real)
        for m in range(1 << len(names)):
            yield {k: (self.real if m >> i & 1 else self.decoy)[k] for i, k in enumerate(names)}


def parts(e):
    return e if isinstance(e, tuple) else (e, None)


def differs(a, b):
    """do two expectations differ where both are defined?"""
    (a, ma), (b, mb) = parts(a), parts(b)
    if not isinstance(a, np.ndarray):
        return a != b
    m = np.ones(a.shape, bool) if ma is None else ma
    if mb is not None:
        m = m & mb
    return bool(((a != b) & m).any())


# ---------------------------------------------------------------------------------------------------------------------
# the harness (GPU)
# ---------------------------------------------------------------------------------------------------------------------
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64,
           np.dtype(np.int32): np.int32, np.dtype(np.int64): np.int64}


def to_dev(a):
    """an ndarray as a device tensor of the same bytes (torch has no unsigned 16/32/64-bit types)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype]).copy()).cuda()


def to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


DELAY_MS = 30.0                                  # tens of milliseconds: far beyond any enqueue, short enough for the suite


def calibrate(target_ms=DELAY_MS):
    """cycles of torch.cuda._sleep that keep a stream busy for target_ms, measured once with events"""
    import torch
    s = torch.cuda.Stream()
    probe = 20_000_000
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)                      # (loads the kernel)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
    s.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.05, "torch.cuda._sleep(%d) took %.3f ms: it cannot serve as a delay" % (probe, ms)
    cycles = int(probe * target_ms / ms)
    print("late-input harness: torch.cuda._sleep(%d) is %.2f ms; the delay is %d cycles = %.1f ms" % (probe, ms, cycles, target_ms))
    return cycles


def runs_beside(stream, sleeper, delay):
    """does work on `stream` run while `sleeper` is busy?  The runtime maps its streams onto a few hardware queues, and two
    streams on one queue run in submission order: a launch on the wrong one of them would wait for the delay like a launch on
    the right one.  No timing: the marker on `stream` is awaited, and the sleeper must still be busy then (were the queue
    shared, the marker would have waited for the whole delay, with nothing behind it)."""
    import torch
    torch.cuda.synchronize()
    with torch.cuda.stream(sleeper):
        torch.cuda._sleep(delay)
    with torch.cuda.stream(stream):
        marker = torch.cuda.Event()
        marker.record()
    marker.synchronize()
    beside = sleeper.query() is False
    sleeper.synchronize()
    return beside


def pick_stream(delay, beside):
    """a non-blocking torch stream whose work runs beside that of every stream in `beside` (one delay per probe, at most 8 streams)"""
    import torch
    for _ in range(8):
        s = torch.cuda.Stream()
        if all(runs_beside(o, s, delay) for o in beside):
            return s
    raise AssertionError("no stream found that runs beside %r: the premise of the harness cannot be had" % (beside,))


class Late:
    """the buffers of one run: decoy in the inputs, EARLY in the outputs; the staging tensors; the snapshots"""

    def __init__(self, case, quiet=None):
        """quiet: "real" or "decoy" puts that set into the inputs and SENT into the outputs at once (a run without late arrival)"""
        import torch
        self.case = case
        self.stage_real = {k: to_dev(v) for k, v in case.real.items()}
        self.stage_decoy = {k: to_dev(v) for k, v in case.decoy.items()}
        self.b = {k: v.clone() for k, v in (self.stage_real if quiet == "real" else self.stage_decoy).items()}
        self.stage_sent = {}
        for group, fill in ((case.outputs, SENT if quiet else EARLY), (case.scratch, EARLY)):
            for k, (shape, dtype) in group.items():
                self.b[k] = to_dev(sent(shape, dtype, fill))
        for k, (shape, dtype) in case.outputs.items():
            self.stage_sent[k] = to_dev(sent(shape, dtype, SENT))
        self.snap = {k: torch.empty_like(self.b[k]) for k in case.compared()}
        self.ret = {}

    def arrive(self, delay):
        """step 2, on the current stream"""
        import torch
        torch.cuda._sleep(delay)
        for k, v in self.stage_real.items():
            self.b[k].copy_(v, non_blocking=True)
        for k, v in self.stage_sent.items():
            self.b[k].copy_(v, non_blocking=True)

    def leave(self, restore=True):
        """step 5, on the current stream"""
        for k, v in self.snap.items():
            v.copy_(self.b[k], non_blocking=True)
        if restore:
            for k, v in self.stage_decoy.items():
                self.b[k].copy_(v, non_blocking=True)

    def verdict(self, exp=None):
        """step 6 after the synchronisation: the first mismatch as text, or None"""
        exp = self.case.exp_real if exp is None else exp
        for k in self.snap:
            e, m = parts(exp[k])
            got = to_host(self.snap[k], e.dtype).reshape(e.shape)
            bad = got != e if m is None else (got != e) & m
            if bad.any():
                at = tuple(int(x[0]) for x in np.nonzero(bad))
                return "%s: %s%r is 0x%x, expected 0x%x (%d of %d differ)" % (self.case.name, k, at, int(got[at]), int(e[at]), int(bad.sum()), bad.size)
        if sorted(self.ret) != sorted(self.case.returns):
            return "%s: the call returned %r, the case names %r" % (self.case.name, sorted(self.ret), sorted(self.case.returns))
        for k, v in self.ret.items():
            if not (exp[k].holds(v) if isinstance(exp[k], Between) else v == exp[k]):
                return "%s: %s returned %r, expected %r" % (self.case.name, k, v, exp[k])
        return None


class Probe:
    """what a case may assert about the caller's stream in the middle of its calls; silent in a quiet run (side None), and for
    busy() on a fresh context, whose first-use allocations may synchronise"""

    def __init__(self, side=None, fresh=False):
        self.side, self.fresh = side, fresh

    def busy(self, what):
        if self.side is not None and not self.fresh:
            assert self.side.query() is False, "%s returned with the caller's stream idle (a host synchronisation, or the delay is too short)" % what

    def idle(self, what):
        if self.side is not None:
            assert self.side.query() is True, "%s returned while the caller's stream was busy" % what


def host_values(ret):
    """what a case's call returns: host values by name, or nothing that counts"""
    return ret if isinstance(ret, dict) else {}


def run_quiet(case, hip, which="decoy"):
    """the call on torch's current stream with one of the input sets already in place: (run, expectation); nothing is awaited"""
    run = Late(case, which)
    run.ret = host_values(case.call(hip, run.b, Probe()))
    run.leave(restore=False)
    return run, case.exp_real if which == "real" else case.exp_decoy


def run_late(case, hip, delay, side, fresh=False):
    """steps 1 to 6 for one case on one context, on the non-blocking stream `side` (pick_stream: one that runs beside the null
    stream); raises AssertionError with the premise or the mismatch"""
    import torch
    run = Late(case)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run.arrive(delay)
        assert side.query() is False, "%s: premise: the stream is idle before the call (delay too short)" % case.name
        run.ret = host_values(case.call(hip, run.b, Probe(side, fresh)))
        if case.asynchronous:
            Probe(side, fresh).busy(case.name)
        run.leave()
    side.synchronize()
    bad = run.verdict()
    assert bad is None, bad
    return run


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name):
    def reg(f):
        CASES[name] = functools.lru_cache(maxsize=None)(f)
        return f
    return reg


def build(name):
    return CASES[name]()


def set_palette(mode512, which=0):
    return lambda hip: hip.set_palette(*palettes(which), mode512)


def ptr(t):
    return t.data_ptr() if t is not None else None


# ---- palette table + quantise ---------------------------------------------------------------------------------------
def _quantise_set(seed, mode512):
    rng = np.random.default_rng(seed)
    p0, p1 = palettes()
    pix = rng.integers(0, 1 << 24, 4099, dtype=np.uint32)
    pix[:600] = np.concatenate([p0, p1])[rng.integers(0, 512, 600)]              # exact hits among them
    ent = np.zeros(pix.size, np.uint16)
    O.oracle().orc_quantise(p0, p1, int(mode512), pix, pix.size, ent)
    return {"pix": pix}, {"entries": ent}


def _quantise(mode512, with_set):
    """quantise_dev alone (the palette is set quietly before), and set_palette + quantise_dev on the busy stream: set_palette waits
    for its stream (the colours go up from the caller's memory), so only the first form sees the pixels arrive late"""
    real, er = _quantise_set(31, mode512)
    decoy, ed = _quantise_set(32, mode512)

    def call(hip, b, side):
        if with_set:
            hip.set_palette(*palettes(), mode512)              # (builds, or finds, the table)
        hip._ck(hip.L.agmv_hip_quantise_dev(hip.ctx, ptr(b["pix"]), b["pix"].numel(), ptr(b["entries"]), hip._stream()))
    return Case("%squantise-%d" % ("set_palette+" if with_set else "", 512 if mode512 else 256), real, decoy, er, ed, {"entries": ((4099,), np.uint16)},
                call, asynchronous=not with_set, setup=None if with_set else set_palette(mode512))


for _m in (True, False):
    for _s in (False, True):
        case("%squantise-%d" % ("set_palette+" if _s else "", 512 if _m else 256))(functools.partial(_quantise, _m, _s))


# ---- encode ----------------------------------------------------------------------------------------------------------
def _encode_set(seed, mode512, first_fc, as_entries, pal=0):
    """9 frames at frame_count first_fc ..; a batch inside a GOP (6) follows two lead frames whose I-frame gives the entry plane"""
    rng = np.random.default_rng(seed)
    p0, p1 = palettes(pal)
    frames = T.clip(rng, W, H, 9)
    stride = max_usize(mode512)
    if first_fc & 3:
        lead = T.clip(rng, W, H, first_fc & 3)
        enc = O.OracleEncoder(W, H, mode512, p0, p1, first_fc & ~3)
        _, ient = enc.encode(lead[0], want_entries=True)
        for f in lead[1:]:
            enc.encode(f)
    else:
        enc = O.OracleEncoder(W, H, mode512, p0, p1, first_fc)
        ient = (rng.integers(0, 2 if mode512 else 1, W * H) << 8 | rng.integers(0, 256, W * H)).astype(np.uint16)   # not read
    out, mask = sent((9, stride), np.uint8), np.zeros((9, stride), bool)
    sizes, ents, ient_after = np.zeros(9, np.uint32), [], None
    for f in range(9):
        o, e = enc.encode(frames[f], want_entries=True)
        out[f, :len(o)], mask[f, :len(o)], sizes[f] = o, True, len(o)
        ents.append(e)
        if (first_fc + f) & 3 == 0:
            ient_after = e
    inp = {"pix": np.stack(ents).astype(np.uint32).reshape(9, H, W) if as_entries else frames, "ientries": ient}
    return inp, {"out": (out, mask), "sizes": sizes, "ientries": ient_after}


@functools.lru_cache(maxsize=None)
def _encode(mode512, first_fc, as_entries, pal=0):
    name = "%s-%d-fc%d" % ("encode_entries" if as_entries else "encode", 512 if mode512 else 256, first_fc)
    real, er = _encode_set(41, mode512, first_fc, as_entries, pal)
    decoy, ed = _encode_set(42, mode512, first_fc, as_entries, pal)
    stride = max_usize(mode512)

    def call(hip, b, side):
        f = hip.L.agmv_hip_encode_entries_dev if as_entries else hip.L.agmv_hip_encode_frames_dev
        hip._ck(f(hip.ctx, ptr(b["pix"]), 9, W, H, first_fc, ptr(b["out"]), stride, ptr(b["sizes"]), ptr(b["ientries"]), hip._stream()))

    def bounds(inp):
        lim = 2 if mode512 else 1
        assert (inp["ientries"] >> 8 < lim).all()
        if as_entries:
            assert (inp["pix"] >> 8 < lim).all()
    return Case(name, real, decoy, er, ed, {"out": ((9, stride), np.uint8), "sizes": ((9,), np.uint32)}, call, bounds, inplace=("ientries",),
                setup=set_palette(mode512, pal))


for _m in (True, False):
    for _fc in (0, 6):
        for _e in (False, True):
            case("%s-%d-fc%d" % ("encode_entries" if _e else "encode", 512 if _m else 256, _fc))(functools.partial(_encode, _m, _fc, _e))


# ---- decode ----------------------------------------------------------------------------------------------------------
DEC_N, DEC_FC = 13, 0


def _dec_stride(mode512):
    return (max_usize(mode512) + 16 + 255) & ~255


@functools.lru_cache(maxsize=None)
def _decode_set(seed, mode512, pal=0):
    """13 oracle-encoded frames, frame 5 cut short (k_fixup has work: its tail keeps the frame before), from a given decoder state.
    decode_depends_on_prior is the oracle's: do the pixels change when every pixel of the prior state does?"""
    rng = np.random.default_rng(seed)
    p0, p1 = palettes(pal)
    frames = T.clip(rng, W, H, DEC_N)
    bits = T.encode(W, H, mode512, p0, p1, frames, DEC_FC)
    bits[5] = bits[5][:max(1, len(bits[5]) * 2 // 3)]
    if seed == 51:                                   # the real set: the first frame cut short too, so that its tail is the caller's `prev`
        bits[0] = bits[0][:max(1, len(bits[0]) // 2)]          # and the batch depends on the prior state (the decoy's does not)
    prev = rng.integers(0, 1 << 24, (H, W), dtype=np.uint32)
    previ = rng.integers(0, 1 << 24, (H, W), dtype=np.uint32)
    pix, pads, offs, nent = T.oracle_range(W, H, mode512, p0, p1, bits, DEC_FC, prev, previ)
    m = np.uint32(0xFFFFFF)
    other = T.oracle_range(W, H, mode512, p0, p1, bits, DEC_FC, prev ^ m, previ ^ m)[0]
    rows, bpos = T.slab(bits, pads, _dec_stride(mode512))
    inp = {"bits": rows, "bpos": bpos.astype(np.uint32), "prev": prev, "prev_iframe": previ}
    exp = {"pix": pix.reshape(DEC_N, H, W).astype(np.uint32), "nentered": nent.astype(np.uint32),
           "offsets": (offs.astype(np.uint32), np.arange(NBLK)[None, :] < nent[:, None]),
           "decode_depends_on_prior": bool((other != pix).any()),
           "parse_fallback_frames": Between(0, DEC_N)}            # a count of frames of the call; which of them, no reference says
    return inp, exp


def _dec_bounds(mode512):
    def bounds(inp):
        assert inp["bits"].shape[1] == _dec_stride(mode512) and (inp["bpos"].astype(np.int64) <= inp["bits"].shape[1] - 16).all()
    return bounds


def _stats(hip, side, *which):
    """the calls that synchronise the stream, on the busy stream with nothing behind them: the stream is idle when they return"""
    ret = {}
    for w in which:
        if w == "check":
            hip.check()
        else:
            ret[w] = getattr(hip, w)(W, H) if w == "decode_depends_on_prior" else getattr(hip, w)()
        side.idle(w)
    return ret


@functools.lru_cache(maxsize=None)
def _decode(kind, mode512, slices=None, pal=0):
    name = "%s-%d%s" % (kind, 512 if mode512 else 256, "-slices%d" % slices if slices else "")
    real, er = _decode_set(51, mode512, pal)
    decoy, ed = _decode_set(52, mode512, pal)
    outs = {"pix": ((DEC_N, H, W), np.uint32), "nentered": ((DEC_N,), np.uint32)}
    if kind != "decode_bitstreams":
        outs["offsets"] = ((DEC_N, NBLK), np.uint32)
    er, ed = ({k: e[k] for k in outs} for e in (er, ed))

    def call(hip, b, side):
        kw = dict(prev=b["prev"], prev_iframe=b["prev_iframe"])
        if kind == "parse+decode":
            hip.parse_dev(b["bits"], b["bpos"], DEC_N, W, H, offsets=b["offsets"], nentered=b["nentered"])
            hip.decode_dev(b["bits"], b["bpos"], b["offsets"], b["nentered"], DEC_N, W, H, DEC_FC, out=b["pix"], **kw)
        elif kind == "parse_decode":
            hip.parse_decode_dev(b["bits"], b["bpos"], DEC_N, W, H, DEC_FC, out=b["pix"], offsets=b["offsets"], nentered=b["nentered"], **kw)
        else:
            hip.decode_bitstreams_dev(b["bits"], b["bpos"], DEC_N, W, H, DEC_FC, out=b["pix"], nentered=b["nentered"], **kw)
    return Case(name, real, decoy, er, ed, outs, call, _dec_bounds(mode512), setup=set_palette(mode512, pal),
                env={"AGMV_DEC_SLICES": str(slices)} if slices else {})


def _decode_stats(mode512):
    """decode_bitstreams_dev, then the three calls that read a word back: they must wait for the caller's stream"""
    c = _decode("decode_bitstreams", mode512)
    inner, returns = c.call, ("decode_depends_on_prior", "parse_fallback_frames")
    er, ed = ({k: _decode_set(seed, mode512)[1][k] for k in tuple(c.outputs) + returns} for seed in (51, 52))

    def call(hip, b, side):
        inner(hip, b, side)
        return _stats(hip, side, "decode_depends_on_prior", "parse_fallback_frames", "check")
    return Case("decode_stats-%d" % (512 if mode512 else 256), c.real, c.decoy, er, ed, c.outputs, call, c.bounds, setup=c.setup,
                asynchronous=False, returns=returns)


for _m in (True, False):
    _n = 512 if _m else 256
    case("parse+decode-%d" % _n)(functools.partial(_decode, "parse+decode", _m))
    case("parse_decode-%d-slices1" % _n)(functools.partial(_decode, "parse_decode", _m, 1))
    case("parse_decode-%d-slices3" % _n)(functools.partial(_decode, "parse_decode", _m, 3))
    case("decode_bitstreams-%d" % _n)(functools.partial(_decode, "decode_bitstreams", _m))
case("decode_stats-512")(functools.partial(_decode_stats, True))


# ---- pack / unpack ---------------------------------------------------------------------------------------------------
PK_STRIDE, PK_MSG = 700, 2400


def _pack_set(seed):
    rng = np.random.default_rng(seed)
    sizes = np.array([[0, 1, 700, 333, 0, 257, 64], [5, 0, 699, 2, 512, 0, 31]][seed & 1], np.uint32)
    slab = rng.integers(0, 256, (7, PK_STRIDE), dtype=np.uint8)
    msg = sent(PK_MSG, np.uint8)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    msg[:int(offs[7])] = np.concatenate([slab[f, :sizes[f]] for f in range(7)])
    return slab, sizes, msg, offs


def _pack_bounds(inp):
    assert (inp["sizes"] <= PK_STRIDE).all() and int(inp["sizes"].sum()) <= PK_MSG


@case("pack_frames")
def _pack():
    sets = []
    for seed in (60, 61):
        slab, sizes, msg, offs = _pack_set(seed)
        sets.append(({"slab": slab, "sizes": sizes}, {"msg": msg, "offsets": offs}))

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_pack_frames_dev(hip.ctx, ptr(b["slab"]), PK_STRIDE, ptr(b["sizes"]), 7, ptr(b["msg"]), ptr(b["offsets"]), hip._stream()))
    return Case("pack_frames", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"msg": ((PK_MSG,), np.uint8), "offsets": ((8,), np.uint64)}, call, _pack_bounds)


@case("unpack_frames")
def _unpack():
    sets = []
    for seed in (60, 61):
        slab, sizes, msg, offs = _pack_set(seed)
        msg[int(offs[7]):] = np.random.default_rng(seed).integers(0, 256, PK_MSG - int(offs[7]), dtype=np.uint8)   # (what lies behind a message)
        rows = sent((7, PK_STRIDE), np.uint8)
        for f in range(7):
            rows[f, :sizes[f]] = slab[f, :sizes[f]]
        sets.append(({"msg": msg, "sizes": sizes}, {"slab": rows}))

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_unpack_frames_dev(hip.ctx, ptr(b["msg"]), ptr(b["sizes"]), 7, ptr(b["slab"]), PK_STRIDE, ptr(b["offsets"]), hip._stream()))
    return Case("unpack_frames", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"slab": ((7, PK_STRIDE), np.uint8)}, call, _pack_bounds,
                scratch={"offsets": ((8,), np.uint64)})


# ---- the encoder's LZ stages -----------------------------------------------------------------------------------------
LZ_STRIDE = 3 * L77.SEG + 80
LZ_PERSIST = 5000                               # shorter than two of the streams, longer than the others


def lz_streams(which):
    """5 pre-LZ streams: bitstream-like content of about 6 KB, zeros of 3 * SEG + 77, an empty one"""
    z = np.zeros(3 * L77.SEG + 77, np.uint8)
    if which == 0:
        return [L77.bitstream_like(1, n=6100), z, np.zeros(0, np.uint8), L77.bitstream_like(2, n=900), L77.bitstream_like(3, n=77)]
    return [L77.bitstream_like(4, n=1300), L77.bitstream_like(5, n=5900), L77.bitstream_like(6, n=40), np.zeros(0, np.uint8), z[:-7]]


def _lz_rows(streams):
    rows = np.full((5, LZ_STRIDE), 0xEE, np.uint8)                     # what lies behind a stream must never be read
    for f, x in enumerate(streams):
        rows[f, :len(x)] = x
    return rows, np.array([len(x) for x in streams], np.uint32)


def _lz_bounds(inp):
    assert (inp["sizes"] <= LZ_STRIDE).all()


def _payload_rows(payloads, ostride):
    out, cs = sent((5, ostride), np.uint8), np.zeros(5, np.uint32)
    for f, p in enumerate(payloads):
        out[f, :len(p)], cs[f] = p, len(p)
    return out, cs


@case("lzss_frames")
def _lzss():
    ostride = int(hip_library().agmv_hip_lzss_max_csize(LZ_STRIDE))
    sets = []
    for which in (0, 1):
        rows, sizes = _lz_rows(lz_streams(which))
        out, cs = _payload_rows([LZS.orc(x) for x in lz_streams(which)], ostride)
        sets.append(({"bits": rows, "sizes": sizes}, {"out": out, "csize": cs}))

    def call(hip, b, side):
        hip.lzss_frames_dev(b["bits"], b["sizes"], 5, out=b["out"], csize=b["csize"])
    return Case("lzss_frames", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"out": ((5, ostride), np.uint8), "csize": ((5,), np.uint32)}, call,
                _lz_bounds, asynchronous=False)


@case("lz77_peek+frames")
def _lz77():
    ostride = 4 * LZ_STRIDE
    sets = []
    for which in (0, 1):
        streams = lz_streams(which)
        rows, sizes = _lz_rows(streams)
        persist = np.random.default_rng(70 + which).integers(0, 256, LZ_PERSIST, dtype=np.uint8)
        after = persist.copy()
        peek = L77.prepare_batch_peek(rows, sizes, after)
        out, cs = _payload_rows([L77.orc77(x, int(peek[f])) for f, x in enumerate(streams)], ostride)
        segments = sum((len(x) + L77.SEG - 1) // L77.SEG for x in streams)   # a count of segments of the call; which of them, no reference says
        sets.append(({"bits": rows, "sizes": sizes, "persist": persist},
                     {"peek": peek, "out": out, "csize": cs, "persist": after, "lz77_reparsed_segments": Between(0, segments)}))

    def call(hip, b, side):
        hip.lz77_peek_dev(b["bits"], b["sizes"], 5, b["persist"], peek=b["peek"])
        side.busy("lz77_peek_dev")
        hip.lz77_frames_dev(b["bits"], b["sizes"], 5, peek=b["peek"], out=b["out"], csize=b["csize"])
        return _stats(hip, side, "lz77_reparsed_segments")
    return Case("lz77_peek+frames", sets[0][0], sets[1][0], sets[0][1], sets[1][1],
                {"peek": ((5,), np.uint8), "out": ((5, ostride), np.uint8), "csize": ((5,), np.uint32)}, call, _lz_bounds, inplace=("persist",),
                asynchronous=False, returns=("lz77_reparsed_segments",))


# ---- the decoder's LZ stage -------------------------------------------------------------------------------------------
LZD_CAP = 3 * L77.SEG + 77 + 16 + 3             # lim = cap - 16 just above the longest stream


def crafted_fallback(version, k):
    """frames that the header DEFINES as fallback frames (a match with offset > pos followed by further tokens), as
    tests/test_gpu_lz_decode.py crafts them: the damaged payloads whose count a reference can tell"""
    if version == 1:
        return LZD.lzss_frame([[("L", 1), ("L", 2), ("M", 9, 12), ("L", 3), ("M", 1, 5)], [("M", 4, 4), ("L", 6), ("M", 1, 15)]][k])
    return LZD.lz77_frame([[(0, 0, 1), (5, 9, 2), (1, 3, 4)], [(2, 2, 2), (0, 0, 5)]][k])


def _lzd_image(version, which, damaged=None, crafted=()):
    """the 5 streams compressed by the host library as a file image with explicit avail (payload + guard); payload `damaged` has
    random bytes put in, the frames at `crafted` are replaced by crafted_fallback frames"""
    import hostlib as HL
    frames = []
    for f, x in enumerate(lz_streams(which)):
        if f in crafted:
            fr = crafted_fallback(version, crafted.index(f))
            frames.append(LZD.Frame(fr.payload, fr.usize, fr.csize, avail=len(fr.payload) + len(LZD.GUARD)))
            continue
        p, cs = (HL.lzss if version == 1 else HL.lz77)(x)
        p = p.copy()
        if f == damaged and len(p) > 40:
            p[20:40] ^= np.random.default_rng(80 + which).integers(1, 256, 20, dtype=np.uint8)
        frames.append(LZD.Frame(p.tobytes(), len(x), cs, avail=len(p) + len(LZD.GUARD)))
    src, off, avail = LZD.image(frames)
    return src, off.astype(np.uint64), avail.astype(np.uint32), np.array([f.usize for f in frames], np.uint32), np.array([f.csize for f in frames], np.uint32)


LZD_SRC = 65536                                 # every image is padded to this length: off + avail of any mixture stays inside


def _lzd_expect(version, src, off, avail, usize, csize, persist=None):
    """host stage per frame into rows that hold SENT (nothing but data[0, bpos) is written), then the commit loop"""
    rows0, bpos, used = LZD.host_lz(version, src, off.astype(np.int64), avail, usize, csize, LZD_CAP, LZD_CAP)
    rows = sent((5, LZD_CAP), np.uint8)
    for f in range(5):
        rows[f, :bpos[f]] = rows0[f, :bpos[f]]
    exp = {"bits": rows, "bpos": bpos.astype(np.uint32), "used": used.astype(np.uint32)}
    if persist is not None:
        per = persist.copy()
        exp["bits"], exp["persist"] = LZD.commit(rows.copy(), bpos, per)
    return exp


def _lzd_pad(src):
    assert len(src) <= LZD_SRC
    return np.concatenate([src, np.zeros(LZD_SRC - len(src), np.uint8)])


def _lzd_bounds(inp, avail=None, csize=None, usize=None):
    a = inp["avail"] if avail is None else avail
    c = inp["csize"] if csize is None else csize
    u = inp["usize"] if usize is None else usize
    assert (u.astype(np.int64) <= LZD_CAP - 16).all()
    reach = inp["off"].astype(np.int64) + np.minimum(a.astype(np.int64), c.astype(np.int64) + 3)
    assert (reach <= inp["src"].size).all() and inp["src"].size == LZD_SRC


def _lzd(version):
    """lz_decode_frames_dev (the sizes arrive late) + lz_decode_commit_dev + the fallback count.  The damaged payloads are frames the
    header defines as fallback frames, one in the real set and two in the decoy; what the host library compressed never is one
    (tests/test_gpu_lz_decode.py), so the count is the number of crafted frames"""
    vname = "lzss" if version == 1 else "lz77"
    sets = []
    for which, crafted in ((0, (4,)), (1, (2, 3))):
        src, off, avail, usize, csize = _lzd_image(version, which, crafted=crafted)
        persist = np.random.default_rng(90 + which).integers(0, 256, LZD_CAP, dtype=np.uint8)
        inp = {"src": _lzd_pad(src), "off": off, "avail": avail, "usize": usize, "csize": csize, "persist": persist}
        exp = _lzd_expect(version, inp["src"], off, avail, usize, csize, persist)
        exp["lz_decode_fallback_frames"] = len(crafted)
        sets.append((inp, exp))

    def call(hip, b, side):
        hip.lz_decode_frames_dev(version, b["src"], b["off"], b["avail"], b["usize"], b["csize"], 5, LZD_CAP, bits=b["bits"], bpos=b["bpos"], used=b["used"])
        hip.lz_decode_commit_dev(b["bits"], b["bpos"], 5, b["persist"])
        return _stats(hip, side, "lz_decode_fallback_frames")
    return Case("lz_decode+commit-" + vname, sets[0][0], sets[1][0], sets[0][1], sets[1][1],
                {"bits": ((5, LZD_CAP), np.uint8), "bpos": ((5,), np.uint32), "used": ((5,), np.uint32)}, call, _lzd_bounds, inplace=("persist",),
                asynchronous=False, returns=("lz_decode_fallback_frames",))


case("lz_decode+commit-lzss")(functools.partial(_lzd, 1))
case("lz_decode+commit-lz77")(functools.partial(_lzd, 3))


@case("lz_decode_sized-pair")
def _lzd_sized():
    """two agmv_hip_lz_decode_frames_sized_dev calls back to back on the busy stream, an LZSS table and an LZ77 table: the second
    rewrites the pinned staging the first uploads from.  The sizes are host arguments and stay; the decoy is other payload bytes
    at shifted offsets (damaged streams, which the stage must survive in bounds).  The first call returns while the stream is
    busy; the second waits on the host for the first's upload (the rule in "Notes on a context")."""
    tabs = {1: _lzd_image(1, 0, damaged=1), 3: _lzd_image(3, 1, damaged=4)}
    real, decoy, er, ed = {}, {}, {}, {}
    for v, (src, off, avail, usize, csize) in tabs.items():
        src = _lzd_pad(src)
        rng = np.random.default_rng(100 + v)
        dsrc = np.where(rng.integers(0, 4, LZD_SRC) == 0, rng.integers(0, 256, LZD_SRC), src).astype(np.uint8)
        doff = off + rng.integers(1, 9, 5).astype(np.uint64)
        for f in (0, 1):                             # two payloads of zeros: tokens that emit nothing (LZSS) or one byte each (LZ77),
            dsrc[int(off[f]):int(off[f]) + int(avail[f]) + 8] = 0     # so that bpos and used differ too, with the same host sizes
        for inp, exp, s, o in ((real, er, src, off), (decoy, ed, dsrc, doff)):
            inp["src%d" % v], inp["off%d" % v] = s, o
            for k, a in _lzd_expect(v, s, o, avail, usize, csize).items():
                exp["%s%d" % (k, v)] = a

    def call(hip, b, side):
        for v, (_, _, avail, usize, csize) in tabs.items():
            hip.lz_decode_frames_dev(v, b["src%d" % v], b["off%d" % v], avail, usize, csize, 5, LZD_CAP, bits=b["bits%d" % v], bpos=b["bpos%d" % v],
                                     used=b["used%d" % v])
            if v == 1:
                side.busy("lz_decode_frames_sized_dev")

    def bounds(inp):
        for v, (_, _, avail, usize, csize) in tabs.items():
            _lzd_bounds({"src": inp["src%d" % v], "off": inp["off%d" % v]}, avail, csize, usize)
    outs = {}
    for v in tabs:
        outs.update({"bits%d" % v: ((5, LZD_CAP), np.uint8), "bpos%d" % v: ((5,), np.uint32), "used%d" % v: ((5,), np.uint32)})
    # LZ77 fetches csize bytes whatever they hold (agmv_lz_decode_mem: its loop runs over csize), so with the sizes in host memory
    # `used` is min(csize, avail): compared on the GPU, but no device input can change it
    return Case("lz_decode_sized-pair", real, decoy, er, ed, outs, call, bounds, asynchronous=False,
                host_determined={"used3": np.minimum(tabs[3][2], tabs[3][4])})


# ---- the helper kernels ----------------------------------------------------------------------------------------------
NPX2 = W2 * H2


def grey_counts(pix):
    """the integer behind AGMV_CompareFrameSimilarity for every adjacent pair of uint32 [n, npx]"""
    p = np.asarray(pix, np.uint32).reshape(len(pix), -1)
    g = (((p >> 16) & 255) + ((p >> 8) & 255) + (p & 255)) // 3
    return (g[:-1] == g[1:]).sum(axis=1).astype(np.uint32)


def helper_clip(seed, n=3, w=W2, h=H2):
    """n frames in which many pixels keep their grey from frame to frame (the counts are neither 0 nor all)"""
    rng = np.random.default_rng(seed)
    f = [rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)]
    for _ in range(n - 1):
        f.append(np.where(rng.integers(0, 3, (h, w)) == 0, rng.integers(0, 1 << 24, (h, w), dtype=np.uint32), f[-1]))
    return np.stack(f).astype(np.uint32)


def gather_index(seed, npx, n_out=1500):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, npx, n_out).astype(np.uint32)
    idx[rng.integers(0, n_out, 40)] = NONE
    idx[:2] = (npx - 1, 0)
    return idx


def gathered(pix, idx):
    p = np.asarray(pix, np.uint32).reshape(len(pix), -1)
    return np.where(idx[None, :] == NONE, 0, p[:, np.where(idx == NONE, 0, idx)]).astype(np.uint32)


def _index_bounds(npx):
    def bounds(inp):
        assert ((inp["index"] < npx) | (inp["index"] == NONE)).all()
    return bounds


@case("synth")
def _synth():
    """no device input: a launch on another stream is painted over by the late SENT fill of the harness"""
    exp = {"out": np.stack([S.synth_frame(W2, H2, t) for t in range(5, 8)])}

    def call(hip, b, side):
        hip.synth_dev(W2, H2, 5, 3, out=b["out"])
    return Case("synth", {}, {}, exp, {"out": sent((3, H2, W2), np.uint32)}, {"out": ((3, H2, W2), np.uint32)}, call)


@case("interp")
def _interp():
    sets = []
    for seed in (110, 111):
        a, b2 = helper_clip(seed, 2)
        out = np.zeros(NPX2, np.uint32)
        O.oracle().orc_interp_frame(out, np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(b2.reshape(-1)), NPX2)
        sets.append(({"f1": a, "f2": b2}, {"out": out.reshape(H2, W2)}))

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_interp_dev(hip.ctx, ptr(b["out"]), ptr(b["f1"]), ptr(b["f2"]), NPX2, hip._stream()))
    return Case("interp", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"out": ((H2, W2), np.uint32)}, call)


def _hist_before(seed):
    h = np.zeros(1 << 19, np.uint32)
    rng = np.random.default_rng(seed)
    h[rng.integers(0, 1 << 19, 300)] = rng.integers(1, 1000, 300)      # the histogram calls ADD to what is there
    return h


@case("histogram")
def _histogram():
    sets = []
    for seed in (120, 121):
        pix, before = helper_clip(seed), _hist_before(seed)
        sets.append(({"pix": pix, "hist": before}, {"hist": before + PC.histogram(pix, PC.MID)}))

    def call(hip, b, side):
        hip.histogram_dev(b["pix"], PC.MID, hist=b["hist"])
    return Case("histogram", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {}, call, inplace=("hist",))


@case("similarity")
def _similarity():
    sets = [({"pix": helper_clip(s)}, {"counts": grey_counts(helper_clip(s))}) for s in (130, 131)]

    def call(hip, b, side):
        hip.similarity_dev(b["pix"], counts=b["counts"])
    return Case("similarity", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"counts": ((2,), np.uint32)}, call)


@case("gather")
def _gather():
    sets = []
    for seed in (140, 141):
        pix, idx = helper_clip(seed).reshape(3, NPX2), gather_index(seed, NPX2)
        sets.append(({"src": pix, "index": idx}, {"dst": gathered(pix, idx)}))

    def call(hip, b, side):
        hip.gather_dev(b["src"], b["index"], out=b["dst"])
    return Case("gather", sets[0][0], sets[1][0], sets[0][1], sets[1][1], {"dst": ((3, 1500), np.uint32)}, call, _index_bounds(NPX2))


# ---- clips in the caller's layout: one layout per kernel template ------------------------------------------------------------
NPX = W * H
YFLAGS = Y.BT709                                 # (a flag set, so that the tables are not the defaults)


def _fmt_case(name, make, outputs, call, bounds=None, inplace=()):
    sets = [make(s) for s in (150, 151)]
    return Case(name, sets[0][0], sets[1][0], sets[0][1], sets[1][1], outputs, call, bounds, inplace=inplace)


@case("pixels_to_xrgb-rgb24")
def _to_xrgb():
    def make(seed):
        raw = PF.from_packed(PF.RGB24, helper_clip(seed, 3, W, H).reshape(3, NPX))
        return {"src": raw}, {"dst": PF.to_packed(PF.RGB24, raw, NPX)[0][:, :NPX - 5].copy()}
    return _fmt_case("pixels_to_xrgb-rgb24", make, {"dst": ((3, NPX - 5), np.uint32)},
                     lambda hip, b, side: hip.pixels_to_xrgb_dev("rgb24", b["src"], NPX, 3, NPX - 5, out=b["dst"]))


@case("pixels_from_xrgb-rgba32")
def _from_xrgb():
    def make(seed):
        pix = helper_clip(seed, 3, W, H).reshape(3, NPX) | np.uint32(0x5A000000)           # bits >= 24 are ignored
        return {"src": pix}, {"dst": PF.from_packed(PF.RGBA32, pix)}
    return _fmt_case("pixels_from_xrgb-rgba32", make, {"dst": ((3, 4 * NPX), np.uint8)},
                     lambda hip, b, side: hip.pixels_from_xrgb_dev("rgba32", b["src"], out=b["dst"]))


@case("gather_fmt-rgb8p")
def _gather_fmt():
    def make(seed):
        pix, idx = helper_clip(seed, 3, W, H).reshape(3, NPX), gather_index(seed, NPX)
        return {"src": PF.from_packed(PF.RGB8P, pix), "index": idx}, {"dst": gathered(pix, idx)}
    return _fmt_case("gather_fmt-rgb8p", make, {"dst": ((3, 1500), np.uint32)},
                     lambda hip, b, side: hip.gather_fmt_dev("rgb8p", b["src"], NPX, 3, b["index"], out=b["dst"]), _index_bounds(NPX))


@case("histogram_fmt-rgb24")
def _histogram_fmt():
    def make(seed):
        pix, before = helper_clip(seed, 3, W, H).reshape(3, NPX), _hist_before(seed)
        return {"src": PF.from_packed(PF.RGB24, pix), "hist": before}, {"hist": before + PC.histogram(pix[:, :NPX - 7], PC.HIGH)}
    return _fmt_case("histogram_fmt-rgb24", make, {},
                     lambda hip, b, side: hip.histogram_fmt_dev("rgb24", b["src"], NPX, 3, NPX - 7, PC.HIGH, hist=b["hist"]), inplace=("hist",))


@case("similarity_fmt-rgba32")
def _similarity_fmt():
    def make(seed):
        pix = helper_clip(seed, 3, W, H).reshape(3, NPX)
        return {"src": PF.from_packed(PF.RGBA32, pix)}, {"counts": grey_counts(pix)}
    return _fmt_case("similarity_fmt-rgba32", make, {"counts": ((2,), np.uint32)},
                     lambda hip, b, side: hip.similarity_fmt_dev("rgba32", b["src"], 3, NPX, counts=b["counts"]))


def _yuv_clip(fmt, seed):
    return Y.from_packed(fmt, helper_clip(seed, 3, W, H), W, H)


@case("yuv_to_xrgb-nv12")
def _yuv_to():
    fmt = Y.NV12 | YFLAGS

    def make(seed):
        raw = _yuv_clip(fmt, seed)
        return {"src": raw}, {"dst": Y.to_packed(fmt, raw, W, H).reshape(3, NPX)[:, :NPX - 5].copy()}
    return _fmt_case("yuv_to_xrgb-nv12", make, {"dst": ((3, NPX - 5), np.uint32)},
                     lambda hip, b, side: hip.yuv_to_xrgb_dev(fmt, b["src"], W, H, 3, NPX - 5, out=b["dst"]))


@case("yuv_from_xrgb-i420")
def _yuv_from():
    fmt = Y.I420 | YFLAGS

    def make(seed):
        pix = helper_clip(seed, 3, W, H).reshape(3, NPX) | np.uint32(0x5A000000)
        return {"src": pix}, {"dst": Y.from_packed(fmt, pix, W, H)}
    return _fmt_case("yuv_from_xrgb-i420", make, {"dst": ((3, Y.frame_bytes(fmt, W, H)), np.uint8)},
                     lambda hip, b, side: hip.yuv_from_xrgb_dev(fmt, b["src"], W, H, out=b["dst"]))


@case("yuv_gather-nv12")
def _yuv_gather():
    fmt = Y.NV12 | YFLAGS

    def make(seed):
        raw, idx = _yuv_clip(fmt, seed), gather_index(seed, NPX)
        return {"src": raw, "index": idx}, {"dst": gathered(Y.to_packed(fmt, raw, W, H), idx)}
    return _fmt_case("yuv_gather-nv12", make, {"dst": ((3, 1500), np.uint32)},
                     lambda hip, b, side: hip.yuv_gather_dev(fmt, b["src"], W, H, 3, b["index"], out=b["dst"]), _index_bounds(NPX))


@case("yuv_histogram-i420")
def _yuv_histogram():
    fmt = Y.I420 | YFLAGS

    def make(seed):
        raw, before = _yuv_clip(fmt, seed), _hist_before(seed)
        pix = Y.to_packed(fmt, raw, W, H).reshape(3, NPX)
        return {"src": raw, "hist": before}, {"hist": before + PC.histogram(pix[:, :NPX - 7], PC.LOW)}
    return _fmt_case("yuv_histogram-i420", make, {},
                     lambda hip, b, side: hip.yuv_histogram_dev(fmt, b["src"], W, H, 3, NPX - 7, PC.LOW, hist=b["hist"]), inplace=("hist",))


@case("yuv_similarity-nv12")
def _yuv_similarity():
    fmt = Y.NV12 | YFLAGS

    def make(seed):
        rng = np.random.default_rng(seed)
        raw = rng.integers(0, 256, (3, Y.frame_bytes(fmt, W, H)), dtype=np.uint8)
        raw[1:, :W * H] = np.where(rng.integers(0, 2, (2, W * H)) == 0, raw[:2, :W * H], raw[1:, :W * H])   # luma kept: greys often equal
        raw[1:, W * H:] = raw[0, W * H:]
        return {"src": raw}, {"counts": grey_counts(Y.to_packed(fmt, raw, W, H))}
    return _fmt_case("yuv_similarity-nv12", make, {"counts": ((2,), np.uint32)},
                     lambda hip, b, side: hip.yuv_similarity_dev(fmt, b["src"], W, H, 3, counts=b["counts"]))


# ---- scale -----------------------------------------------------------------------------------------------------------
def _scale(fmt, sw, sh, dw, dh):
    name = "scale_area-%s-%s" % (SC.fmt_name(fmt), SC.shape_id((sw, sh, dw, dh)))
    n = 3

    def make(seed):
        raw = SC.from_packed(fmt, helper_clip(seed, n, sw, sh))
        if fmt == PF.XRGB32:
            raw = np.ascontiguousarray(raw).view(np.uint32)
        return {"src": raw}, {"dst": SC.scale_area(SC.to_packed(fmt, np.ascontiguousarray(raw).view(np.uint8).reshape(n, -1), sw, sh), dw, dh)}
    return _fmt_case(name, make, {"dst": ((n, dh, dw), np.uint32)},
                     lambda hip, b, side: hip.scale_area_dev(fmt, b["src"], sw, sh, n, dw, dh, out=b["dst"]))


for _fmt in (PF.XRGB32, Y.NV12):
    for _shape in ((64, 48, 32, 24), (7, 5, 3, 2)):
        case("scale_area-%s-%s" % (SC.fmt_name(_fmt), SC.shape_id(_shape)))(functools.partial(_scale, _fmt, *_shape))


# ---- palette refinement ----------------------------------------------------------------------------------------------
def _refine(which):
    q, hist, pal, n_free, iters = PC.crafted()[which]

    def make(seed):
        if seed == 150:
            h, p = hist, pal
        else:                                        # the decoy: another cloud of bins, other centroids
            rng = np.random.default_rng(seed)
            h = np.zeros(1 << 19, np.uint32)
            h[rng.integers(0, PC.NCODES[q], 2500)] = rng.integers(1, 1 << 20, 2500)
            p = rng.integers(0, 1 << 24, len(pal)).astype(np.uint32)
            if len(pal) == 1:                        # one centroid reaches the mean in its first round: start the decoy there (0 rounds)
                p = PC.refine(h, q, p, n_free, iters)["pal"]
        run = PC.refine(h, q, p, n_free, iters)
        return {"hist": h, "pal": p}, {"pal": run["pal"], "rounds": np.array([run["rounds"]], np.uint32), "sse": np.array(run["sse"], np.uint64)}

    def call(hip, b, side):
        hip._ck(hip.L.agmv_hip_palette_refine_dev(hip.ctx, ptr(b["hist"]), q, ptr(b["pal"]), len(pal), n_free, iters, ptr(b["rounds"]), ptr(b["sse"]),
                                                  hip._stream()))
    return _fmt_case("palette_refine-" + which, make, {"rounds": ((1,), np.uint32), "sse": ((2,), np.uint64)}, call, inplace=("pal",))


case("palette_refine-early_stop")(functools.partial(_refine, "early_stop"))
case("palette_refine-k_1")(functools.partial(_refine, "k_1"))
