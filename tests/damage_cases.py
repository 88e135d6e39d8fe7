"""The corpus of DAMAGED .agmv files that pins the decoder to the reference where clean encoder output never goes: streams cut inside
blocks, bytes flipped to flag values, garbage between blocks, stale flags at data[bpos] of the persistent buffer, the last-block FILL
quirk under damage, P-frame streams at I-frame positions, empty payloads, usize / csize fields that disagree with the payload, and a
frame of "4E 4E ..." that the fast parser gives up on.  numpy and the oracle only, deterministic, and the reference is never read:
tests/golden/make_golden_damage.py decodes these files with the compiled reference and records what it makes of them
(tests/golden/golden_damage.json); tests/test_damage_cpu.py holds the oracle to that record, tests/test_gpu_damage.py the kernels and
tests/test_gpu_damage_files.py every file-decode path.

A case is a dict: name, w, h, version (1 LZSS/512 colours, 2 LZSS/256, 3 LZ77/512, 4 LZ77/256), p0, p1, frames; a frame is a dict:
stream (the pre-LZ bytes), payload (what the chunk holds), usize and csize (the fields the chunk gets), literal (the payload is the
literal-only encoding written here in numpy, whose length is known in closed form).  file_image(case) is the file.

The reference has no bounds of its own, so layout() walks the file the way the reference's reader does -- chunk scan, LZ stage in
plain Python, written from src/agmv_decode.c:171-218 and independent of the oracle's -- and asserts, before anything decodes the
file, that every frame's decoded length + 64 fits the decoder's buffer less 16 (w*h*3 + 64 bytes, the rule of the fuzz in
tests/test_gpu_hotpath.py) and that no payload holds the bytes "AGFC"."""
import ctypes as C

import numpy as np

import oracles as O
import synth as S

FILL, NORMAL, COPY = 0x4E, 0x2F, 0x5E
GUARD = b"\xff" * 8                        # behind every payload, src/agmv_encode.c:622-624
GEOMETRIES = [(4, 4), (4, 24), (20, 12), (68, 36), (64, 48), (1028, 4), (128, 96)]
RUN_GEOMETRY = (1280, 720)                 # 57 600 blocks: a 4E run of 115 201 bytes is 31 parser regions, more than the fast parser repairs


def mode512(version):
    return version in (1, 3)


def room(w, h):
    """the longest stream a frame of the corpus may decode to: decoded length + 64 <= w*h*3 + 64 - 16"""
    return w * h * 3 + 64 - 16 - 64


def u32(v):
    return int(v).to_bytes(4, "little")


# ------------------------------------------------------------------------------------------------ container
def header(num_frames, w, h, version, p0, p1, fps=24, total_audio_duration=0, sample_rate=0, audio_size=0, channels=0, bits_per_sample=16):
    def rgb(p):
        p = np.asarray(p, np.uint32)
        return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], 1).astype(np.uint8).tobytes()
    out = b"AGMV" + u32(num_frames) + u32(w) + u32(h) + bytes([1, version]) + u32(fps) + u32(total_audio_duration) + u32(sample_rate) + u32(audio_size)
    out += int(channels).to_bytes(2, "little") + int(bits_per_sample).to_bytes(2, "little") + rgb(p0)
    return out + (rgb(p1) if mode512(version) else b"")


def lzss_literal(stream):
    """every byte as '1' + 8 bits, LSB first (src/agmv_encode.c:147-152, src/agmv_utils.c:86-112): (bytes, csize field)"""
    s = np.ascontiguousarray(stream, np.uint8)
    bits = np.ones((len(s), 9), np.uint8)
    bits[:, 1:] = np.unpackbits(s[:, None], axis=1, bitorder="little")
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes(), 9 * len(s) // 8


def lz77_literal(stream):
    """every byte as (offset 0, length 0, byte) (src/agmv_encode.c:224-231): (bytes, csize field)"""
    s = np.ascontiguousarray(stream, np.uint8)
    out = np.zeros((len(s), 4), np.uint8)
    out[:, 3] = s
    return out.tobytes(), 4 * len(s)


def compress(version, stream, literal=False):
    """(payload, csize field) of a stream"""
    s = np.ascontiguousarray(stream, np.uint8)
    if literal:
        return lzss_literal(s) if version in (1, 2) else lz77_literal(s)
    src = np.concatenate([s, np.zeros(1, np.uint8)])           # (the LZ77 coder reads the byte behind the stream)
    out = np.zeros(4 * len(s) + 64, np.uint8)
    cs = C.c_uint32(0)
    n = (O.oracle().orc_lzss_compress if version in (1, 2) else O.oracle().orc_lz77_compress)(src, len(s), out, C.byref(cs))
    return out[:n].tobytes(), cs.value


def lz_walk(version, tail, usize, csize, limit):
    """src/agmv_decode.c:171-218 on `tail` (the file from the payload on; zeros behind its end) without the bytes themselves:
    (decoded length, payload bytes read).  Stops with an AssertionError as soon as the length passes `limit`."""
    bpos = 0
    if version in (1, 2):
        bits, nbits = 0, csize * 8

        def get(p, k):
            return (int.from_bytes(tail[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << k) - 1)
        while bits < nbits and bpos < usize:
            if get(bits, 1):
                bpos += 1
                bits += 9
            else:
                off, ln, pos = get(bits + 1, 16), get(bits + 17, 4), bpos
                bits += 21
                for i in range(ln):
                    if 0 <= pos - off + i < bpos:
                        bpos += 1
            assert bpos <= limit, "LZSS frame decodes past %d bytes" % limit
        return bpos, min((bits + 7) // 8, len(tail))
    p = 0
    for _ in range(0, csize, 4):
        t = tail[p:p + 4] + b"\0\0\0\0"
        off, ln, pos = t[0] | t[1] << 8, t[2], bpos
        p += 4
        for i in range(ln):
            if 0 <= pos - off + i < bpos:
                bpos += 1
        bpos += 1
        assert bpos <= limit, "LZ77 frame decodes past %d bytes" % limit
    return bpos, min(p, len(tail))


def frame(version, stream, usize=None, csize=None, literal=False):
    """usize, csize: None = what the encoder writes, an int, or a function of that value"""
    s = np.ascontiguousarray(stream, np.uint8)
    payload, cs = compress(version, s, literal)

    def field(v, own):
        return own if v is None else int(v(own)) if callable(v) else int(v)
    return {"stream": s, "payload": payload, "usize": field(usize, len(s)), "csize": field(csize, cs), "literal": literal,
            "plain": usize is None and csize is None, "csize0": cs}


def layout(case):
    """(file image, [(frame index in case["frames"], decoded length)] of the chunks a reader decodes, in order), bounds asserted"""
    if "_layout" in case:
        return case["_layout"]
    w, h, ver = case["w"], case["h"], case["version"]
    img = header(len(case["frames"]), w, h, ver, case["p0"], case["p1"])
    first, at_of = len(img), {}
    parts = [img]
    pos = first
    for t, f in enumerate(case["frames"]):
        assert b"AGFC" not in f["payload"], "%s: the payload of frame %d holds AGFC" % (case["name"], t)
        assert len(f["stream"]) <= room(w, h), "%s: the stream of frame %d is longer than %d" % (case["name"], t, room(w, h))
        at_of[pos] = t
        chunk = b"AGFC" + u32(t + 1) + u32(f["usize"]) + u32(f["csize"]) + f["payload"] + GUARD
        parts.append(chunk)
        pos += len(chunk)
    img = b"".join(parts)
    pos, read = first, []
    for _ in range(len(case["frames"])):
        at = pos if img[pos:pos + 4] == b"AGFC" else img.find(b"AGFC", pos + 4)      # src/agmv_utils.c:140-166: misses one 1 .. 3 bytes on
        if at < 0 or at + 16 > len(img):
            break
        usize, csize = int.from_bytes(img[at + 8:at + 12], "little"), int.from_bytes(img[at + 12:at + 16], "little")
        t = at_of.get(at, -1)
        f = case["frames"][t] if t >= 0 else None
        if f is not None and f["literal"] and f["plain"]:       # closed form: every token is one byte
            n, used = len(f["stream"]), len(f["payload"])
        else:
            n, used = lz_walk(ver, img[at + 16:], usize, csize, room(w, h))
        assert n + 64 <= w * h * 3 + 64 - 16, "%s: chunk at %d decodes to %d bytes" % (case["name"], at, n)
        read.append((t, n))
        pos = at + 16 + used
    # the header counts the chunks a reader gets to: the reference's chunk scan never returns at the end of a file (src/agmv_utils.c:154-162)
    img = img[:4] + u32(len(read)) + img[8:]
    case["_layout"] = (img, read)
    return case["_layout"]


def file_image(case):
    return layout(case)[0]


# ------------------------------------------------------------------------------------------------ content and base streams
def content_frames(rng, w, h, n):
    """n frames of six kinds: noise, flat, the synthetic clip, a repeat of the frame before, low-bit noise on it, flat 8x8 tiles"""
    frames, prev = [], None
    for _ in range(n):
        kind = int(rng.integers(0, 6))
        if kind == 0 or prev is None and kind in (3, 4):
            f = rng.integers(0, 1 << 24, size=(h, w), dtype=np.uint32)
        elif kind == 1:
            f = np.full((h, w), int(rng.integers(0, 1 << 24)), np.uint32)
        elif kind == 2:
            f = S.synth_frame(max(w, 8), max(h, 8), int(rng.integers(0, 50)))[:h, :w].copy()
        elif kind == 3:
            f = prev.copy()
        elif kind == 4:
            f = prev ^ rng.integers(0, 4, size=(h, w), dtype=np.uint32) * np.uint32(0x010101)
        else:
            f = np.repeat(np.repeat(rng.integers(0, 1 << 24, size=((h + 7) // 8, (w + 7) // 8), dtype=np.uint32), 8, 0), 8, 1)[:h, :w].copy()
        frames.append(np.ascontiguousarray(f, np.uint32))
        prev = frames[-1]
    return np.stack(frames)


def clip(kind, w, h, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "synth":                                        # static left quarter: the P-frames hold COPY blocks
        return np.stack([S.synth_frame(max(w, 8), max(h, 8), t, seed)[:h, :w] for t in range(n)]).astype(np.uint32)
    if kind == "noise":
        return rng.integers(0, 1 << 24, size=(n, h, w), dtype=np.uint32)
    if kind == "flat":
        return np.stack([np.full((h, w), int(c), np.uint32) for c in rng.integers(0, 1 << 24, n)])
    if kind == "repeat":                                       # every GOP one flat frame four times: I-frames of FILL, P-frames of COPY alone
        base = rng.integers(0, 1 << 24, (n + 3) // 4)
        return np.stack([np.full((h, w), int(base[t // 4]), np.uint32) for t in range(n)])
    return content_frames(rng, w, h, n)


class Base:
    """a clean clip: frames, palettes (content_palettes, or random_palettes with duplicate slots) and the oracle encoder's streams"""

    def __init__(self, w, h, version, kind, n, seed, palettes="content", gop=True):
        self.w, self.h, self.version, self.m512 = w, h, version, mode512(version)
        self.frames = clip(kind, w, h, n, seed)
        self.p0, self.p1 = S.content_palettes(self.frames[:4]) if palettes == "content" else S.random_palettes(seed, spread=False)
        enc = O.OracleEncoder(w, h, self.m512, self.p0, self.p1)
        self.streams = []
        for f in self.frames:
            if not gop:                                        # every frame coded as an I-frame: no COPY, every block carries its colours
                enc.close()
                enc = O.OracleEncoder(w, h, self.m512, self.p0, self.p1)
            self.streams.append(enc.encode(f))
        enc.close()

    def blocks(self, t):
        """the clean stream of frame t, block by block"""
        s = self.streams[t]
        dec = O.OracleDecoder(self.w, self.h, self.m512, self.p0, self.p1)
        _, _, offs, n = dec.decode(s, want_tables=True)
        dec.close()
        assert n == self.w * self.h // 16
        ends = list(offs[1:n]) + [len(s)]
        return [s[a:b].copy() for a, b in zip(offs[:n], ends)]

    def case(self, name, frames):
        c = {"name": name, "w": self.w, "h": self.h, "version": self.version, "p0": self.p0, "p1": self.p1,
             "frames": [f if isinstance(f, dict) else frame(self.version, f) for f in frames]}
        assert 8 <= len(c["frames"]) <= 24, (name, len(c["frames"]))
        layout(c)
        return c


def cat(blocks):
    return np.concatenate([np.asarray(b, np.uint8).reshape(-1) for b in blocks] + [np.zeros(0, np.uint8)])


def arr(*v):
    return np.array(v, np.uint8)


def normal_block(m512):
    """a NORMAL block whose codes differ; in 512 colours code 5 is an escape code (two bytes)"""
    codes = [[(37 * k + 11) & 0xFF] for k in range(16)]
    codes = [[c[0] - 1] if (c[0] & 0x7F) == 127 or c[0] in (FILL, NORMAL, COPY) else c for c in codes]
    if m512:
        codes[5] = [0xFF, 0x10]
    return arr(NORMAL, *[b for c in codes for b in c])


LZ_OF = {True: {"lzss": 1, "lz77": 3}, False: {"lzss": 2, "lz77": 4}}
TAG = {True: "m512", False: "m256"}


# ------------------------------------------------------------------------------------------------ the damage kinds
def cut_normal_cases():
    """a stream cut at every byte of its last NORMAL block: before it, behind its flag, behind each code, inside the escape code"""
    for m, lz in ((True, "lzss"), (False, "lz77")):
        b = Base(20, 12, LZ_OF[m][lz], "noise", 22, 101, gop=False)
        nb = normal_block(m)
        frames = [b.streams[0], b.streams[1]]
        for c in range(len(nb)):
            frames.append(cat(b.blocks(2 + c)[:-1] + [nb[:c]]))
        frames.append(cat(b.blocks(2 + len(nb))[:-1] + [nb]))
        yield b.case("cut_normal_" + TAG[m], frames)


def cut_fill_copy_cases():
    """cut inside a 2-byte and a 3-byte FILL and right behind a COPY, in the middle of the frame and in its first block"""
    for m, lz in ((True, "lz77"), (False, "lzss")):
        b = Base(20, 12, LZ_OF[m][lz], "noise", 12, 102, palettes="random", gop=False)
        frames = [b.streams[0], b.streams[1]]
        for t, (k, blk, keep) in enumerate([(7, arr(FILL, 0x21), 1), (7, arr(FILL, 0x7F, 0x21), 1), (7, arr(FILL, 0xFF, 0x21), 2), (7, arr(COPY), 1),
                                            (0, arr(FILL, 0x21), 1), (0, arr(COPY), 1), (14, arr(COPY), 1), (7, arr(FILL, 0x7F, 0x21), 3), (7, arr(COPY, COPY), 2)]):
            frames.append(cat(b.blocks(2 + t)[:k] + [blk[:keep]]))
        yield b.case("cut_fill_copy_" + TAG[m], frames)


def flag_cases():
    """bytes flipped to each flag value: a code of a NORMAL block, a block's own flag, a FILL's index byte, the byte behind a 127 escape"""
    for m, lz in ((True, "lzss"), (False, "lz77")):
        b = Base(68, 36, LZ_OF[m][lz], "noise", 20, 103, gop=False)
        frames = [b.streams[0], b.streams[1]]
        t = 2
        for v in (COPY, FILL, NORMAL):
            bl = b.blocks(t)
            bl[40][3] = v                                      # a code
            frames.append(cat(bl)); t += 1
            bl = b.blocks(t)
            bl[41][0] = v                                      # the flag: FILL leaves 15 codes to resync over, COPY 16
            frames.append(cat(bl)); t += 1
            bl = b.blocks(t)
            bl[42] = arr(FILL, v)                              # a FILL's index byte
            frames.append(cat(bl)); t += 1
            bl = b.blocks(t)
            bl[43] = arr(FILL, 0x7F, v) if m else arr(FILL, v, v)
            bl[44][1:3] = (0xFF, v)                            # (512 colours: an escape code inside a NORMAL block)
            frames.append(cat(bl)); t += 1
        bl = b.blocks(t)
        bl[10:14] = [arr(FILL, 5), arr(FILL, 6), arr(FILL, 7), arr(FILL, 8)]
        bl[10][0] = NORMAL                                     # a FILL taken for a NORMAL eats the blocks behind it
        frames.append(cat(bl))
        yield b.case("flags_" + TAG[m], frames)


def garbage_cases():
    """garbage in front of block 0, between blocks and as the last bytes: the resync runs over it, up to bpos and past it"""
    for m, lz in ((True, "lz77"), (False, "lzss")):
        b = Base(68, 36, LZ_OF[m][lz], "synth", 14, 104)
        rng = np.random.default_rng(1040 + m)
        quiet = lambda n: rng.choice(np.array([0x00, 0x11, 0x4F, 0x2E, 0x5F, 0x7F, 0xFF, 0x80], np.uint8), n)        # no flag among them
        loud = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
        frames = [b.streams[0], b.streams[1]]
        bl = lambda t: b.blocks(t)
        frames.append(cat([quiet(5)] + bl(2)))
        frames.append(cat(bl(3)[:60] + [quiet(1)] + bl(3)[60:]))
        frames.append(cat(bl(4)[:77] + [quiet(40)] + bl(4)[77:]))
        frames.append(cat(bl(5)[:100] + [quiet(1)]))           # the last bytes, blocks left: the resync reaches data[bpos]
        frames.append(cat(bl(6)[:100] + [quiet(3)]))
        frames.append(cat(bl(7)[:9] + [quiet(20)]))
        frames.append(cat(bl(8) + [quiet(7)]))                 # behind a whole frame
        frames.append(cat([loud(9)] + bl(9)[:50] + [loud(30)] + bl(9)[50:]))
        frames.append(cat(bl(10)[:120] + [loud(12)]))
        frames.append(cat([quiet(60)]))                        # nothing but garbage
        frames += [b.streams[12], b.streams[13]]
        yield b.case("garbage_" + TAG[m], frames)


STALE_A = [(NORMAL, 0x22), (COPY, 0x22), (FILL, COPY), (0x11, COPY), (0x11, 0x22), (COPY, FILL)]
STALE_B = [(FILL, 0x22), (0x11, COPY), (NORMAL, COPY), (COPY, COPY), (0x11, FILL), (FILL, FILL)]


def stale_cases():
    """frame k is long and holds chosen bytes at p and p + 1; frame k + 1 is the first 7 blocks of a stream, p bytes: it ends on a
    block boundary with blocks left, so block 7 takes its flag from data[bpos].  Pairs at frames 1|2, 3|4 (a GOP start), 5|6, 7|8 (a GOP
    start and the batch edge of AGMV_BATCH_FRAMES=8), 9|10, 11|12."""
    for m in (True, False):
        for tag, combos, lz, geom in (("a", STALE_A, "lzss", (20, 12)), ("b", STALE_B, "lz77", (4, 24))):
            w, h = geom
            b = Base(w, h, LZ_OF[m][lz], "noise", 14, 105, gop=False)
            frames = [b.streams[0]]
            for i, (at_p, at_p1) in enumerate(combos):
                k = 1 + 2 * i
                m_blocks = 7 if w > 4 else 3
                short = cat(b.blocks(k + 1)[:m_blocks])
                p = len(short)
                long_ = b.streams[k].copy()
                assert len(long_) > p + 2
                long_[p], long_[p + 1] = at_p, at_p1
                frames += [long_, short]
            frames.append(b.streams[13])
            yield b.case("stale_%s_%s" % (tag, TAG[m]), frames)


def quirk_cases():
    """the last block as a FILL: clean (the colour comes from the pixel left of and below its corner), as a 3-byte FILL, cut so that
    its last byte is data[bpos], and cut one byte earlier"""
    for m in (True, False):
        for (w, h), lz in (((4, 24), "lzss"), ((20, 12), "lz77"), ((1028, 4), "lzss")):
            b = Base(w, h, LZ_OF[m][lz], "noise", 10, 106, palettes="random" if w == 20 else "content", gop=False)
            last = lambda t, blk: cat(b.blocks(t)[:-1] + [blk])
            f3 = arr(FILL, 0x7F, 0x33) if m else arr(FILL, 0x33)
            frames = [b.streams[0], last(1, arr(FILL, 0x21)), last(2, f3), b.streams[3], last(4, f3[:-1]), b.streams[5], last(6, f3[:-2]) if m else last(6, arr()),
                      last(7, arr(FILL, 0x44)), last(8, arr(FILL)), b.streams[9]]
            yield b.case("quirk_%dx%d_%s" % (w, h, TAG[m]), frames)


def iframe_cases():
    """GOP 2 made to depend on the frames before it: frame 8 holds frame 9's P-frame stream, COPY blocks included / frame 8's own
    stream cut in half; and the clean clip as the control"""
    for m, lz in ((True, "lzss"), (False, "lz77")):
        b = Base(68, 36, LZ_OF[m][lz], "synth", 16, 107)
        assert COPY in [int(x[0]) for x in b.blocks(9)]
        s = list(b.streams)
        yield b.case("pframe_at_i_" + TAG[m], s[:8] + [s[9]] + s[9:])
        yield b.case("truncated_i_" + TAG[m], s[:8] + [s[8][:len(s[8]) // 2]] + s[9:])
        yield b.case("clean_" + TAG[m], s)


def empty_cases():
    """an empty payload (usize = csize = 0, bpos == 0): block 0 takes its flag from the frame before"""
    for m, lz in ((True, "lz77"), (False, "lzss")):
        b = Base(20, 12, LZ_OF[m][lz], "synth", 10, 108, palettes="random")
        s = list(b.streams)
        yield b.case("empty_first_" + TAG[m], [arr()] + s[1:])
        yield b.case("empty_later_" + TAG[m], s[:5] + [arr()] + s[6:8] + [arr()] + s[9:])


def field_cases():
    """usize / csize fields that disagree with the payload.  LZSS stops at usize, perhaps inside a match; LZ77 ignores it.  A csize
    below the payload's cuts the stream, one above it reads on: into the guard bytes, and with +40 past the next chunk's header."""
    for m, lz, geom, kind in ((True, "lzss", (64, 48), "noise"), (True, "lz77", (64, 48), "noise"), (False, "lzss", (20, 12), "synth"), (False, "lz77", (68, 36), "synth")):
        w, h = geom
        v = LZ_OF[m][lz]
        b = Base(w, h, v, kind, 20, 109, gop=kind == "synth")
        s = b.streams
        f = lambda t, **kw: frame(v, s[t], **kw)
        step = 1 if lz == "lzss" else 4
        frames = [f(0), f(1, usize=lambda u: u - 1), f(2, usize=lambda u: u // 2), f(3, usize=lambda u: u + 5), f(4, usize=lambda u: u + 1000), f(5),
                  f(6, csize=lambda c: c - step), f(7, csize=lambda c: c // 2 // 4 * 4), f(8), f(9, usize=lambda u: u + 9, csize=lambda c: c + 8),
                  f(10, usize=lambda u: u + 30, csize=lambda c: c + 40), f(11), f(12)]
        frames += [f(13 + i, usize=lambda u, d=d: max(u - d, 0)) for i, d in enumerate((2, 3, 5, 8, 13))] + [f(18), f(19)]
        yield b.case("fields_%s_%s" % (lz, TAG[m]), frames)


def run_cases():
    """one frame of a COPY and then "4E 4E ...": two-byte FILLs whose index byte is a flag value, the true chain on the odd bytes.
    Every payload is the literal-only encoding."""
    w, h = RUN_GEOMETRY
    nblk = w * h // 16
    for m, lz in ((True, "lz77"), (False, "lzss")):
        v = LZ_OF[m][lz]
        b = Base(w, h, v, "repeat", 8, 110)
        run = np.full(1 + 2 * (nblk - 1), FILL, np.uint8)
        run[0] = COPY
        s = b.streams
        yield b.case("run4e_" + TAG[m], [frame(v, x, literal=True) for x in (s[0], s[1], s[2], run, s[4], s[5], s[6], s[7])])


def damage(rng, b, t, version, prev_len):
    """one frame of a mix: the clean stream of frame t hurt in a way drawn from all the kinds above"""
    w, h = b.w, b.h
    s = b.streams[t].copy()
    spare = room(w, h) - len(s)
    kind = int(rng.integers(0, 12))
    kw = {}
    if kind == 0 and len(s) > 2:
        s = s[:int(rng.integers(1, len(s)))]
    elif kind == 1:
        for _ in range(int(rng.integers(1, 6))):
            s[int(rng.integers(0, len(s)))] = [FILL, NORMAL, COPY, 0x7F, 0xFF][int(rng.integers(0, 5))]
    elif kind == 2 and spare >= 1:
        at = int(rng.integers(0, len(s) + 1))
        s = cat([s[:at], rng.integers(0, 256, int(rng.integers(1, min(70, spare) + 1)), dtype=np.uint8), s[at:]])
    elif kind == 3:                                            # ends on a block boundary with blocks left: a stale flag at data[bpos]
        bl = b.blocks(t)
        s = cat(bl[:int(rng.integers(0, len(bl)))])
    elif kind == 4:
        bl = b.blocks(t)
        bl[-1] = [arr(FILL, 0x21), arr(FILL), arr(FILL, 0x7F) if b.m512 else arr(FILL, 0x5E), arr(COPY)][int(rng.integers(0, 4))]
        s = cat(bl)
    elif kind == 5:
        s = arr()
    elif kind == 6:
        kw["usize"] = lambda u: max(0, u - int(rng.integers(1, 20)))
    elif kind == 7:
        kw["usize"] = lambda u: u + int(rng.integers(1, 40))
    elif kind == 8:
        kw["csize"] = lambda c: max(0, c - int(rng.integers(1, 12)))
    elif kind == 9 and spare >= 60:
        kw["csize"], kw["usize"] = (lambda c: c + 8), (lambda u: u + int(rng.integers(0, 12)))
    elif kind == 10 and prev_len > 4 and len(s) > prev_len // 2 + 2:                  # a flag where a shorter frame behind this one may end
        s[int(rng.integers(0, len(s)))] = COPY
    return frame(version, s, literal=len(s) > 6000, **kw)


def mix_case(name, seed, w, h, version, palettes):
    """a seeded mix of all kinds on the six kinds of content; tests/test_damage_cpu.py draws more of them at random geometries"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(8, 17))
    kind = "noise" if (w, h) == (64, 48) else "synth" if w * h > 4000 else "mixed"
    b = Base(w, h, version, kind, n, seed, palettes)
    frames, prev_len = [], 0
    for t in range(n):
        f = damage(rng, b, t, version, prev_len) if rng.random() < 0.6 else frame(version, b.streams[t], literal=len(b.streams[t]) > 6000)
        frames.append(f)
        prev_len = len(f["stream"])
    c = {"name": name, "w": w, "h": h, "version": version, "p0": b.p0, "p1": b.p1, "frames": frames}
    layout(c)
    return c


def try_mix_case(name, seed, w, h, version, palettes):
    """mix_case, or None where the draw breaks a bound (a payload that happens to hold AGFC, a raised field that decodes too far)"""
    try:
        return mix_case(name, seed, w, h, version, palettes)
    except AssertionError:
        return None


def mix_cases():
    for i, (w, h) in enumerate(GEOMETRIES):
        version = 1 if (w, h) == (64, 48) else 1 + (i + 1) % 4
        yield mix_case("mix_%dx%d_v%d" % (w, h, version), 7000 + i, w, h, version, "content" if i % 2 else "random")


_CASES = None


def cases():
    """every named case, built once per process"""
    global _CASES
    if _CASES is None:
        out = []
        for gen in (cut_normal_cases, cut_fill_copy_cases, flag_cases, garbage_cases, stale_cases, quirk_cases, iframe_cases, empty_cases,
                    field_cases, run_cases, mix_cases):
            out += list(gen())
        assert len({c["name"] for c in out}) == len(out)
        _CASES = out
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)
