"""Cases for k_encode's persistent pipeline (tests/test_gpu_encode_persistent.py), built and checked on the CPU
(tests/test_encode_cases_cpu.py).  Nothing here needs a GPU; the comparison helper runs on whatever device its tensors are on.

Adversarial clip: test_encode_vs_oracle_shapes_and_content's eleven frames (three noise, flat 0x808080 and 0x808181, a repeat
of the round's first frame and that frame ^ 0x010101, four synthetic), then the same kinds again with other seeds and other
flat colours, cut at 27 frames: 7 GOPs, the last one short.  The second round (frames 11 .. 21) has them in another order,
chosen for the batches of the GPU tests that start inside a GOP, at frames 3, 5, 11 and 14: what such a batch does with the
I-frame entries it is handed shows only in P-frames with COPY blocks, and the first round has none behind those frames.
Frame 11 and its I-frame 8 are both synthetic (their left quarter is static: COPY), frames 14 and 15 are
I-frame 12 (noise) again and that frame ^ 0x010101 (COPY everywhere, the one block of 2052x4's second tile included).

Periodic clip: a base of P = 28 frames (7 GOPs: a prime period in GOPs) repeated to n frames, with marker GOPs of seeded noise
(unique per marker) written over given groups.  The encoder's state does not outlive a GOP, so the bytes of frame t are the
oracle's for base[t % P], and a marker's are those of an OracleEncoder started at first_frame_count = 4 * group.  Without the
markers a mix-up of two groups a multiple of 7 apart would go unseen.

Ticket order: ticket t is tile t // n_groups of group t % n_groups (tile-major), and a workgroup runs the frames of its
(tile, group) in order; one workgroup alone (grid 1) therefore runs item k = (tile k // n_frames, frame k % n_frames)."""
import functools

import numpy as np

import oracles as O
import synth as S

ENC_T = 512                                                    # blocks per tile (k_encode: ENC_T lanes, one block each)
N_ADV = 27
P = 28
FLATS = [(0x808080, 0x808181), (0x7F7F7F, 0x7F8080), (0x000000, 0xFFFFFF)]


def tiles_per_frame(w, h):
    return ((w // 4) * (h // 4) + ENC_T - 1) // ENC_T


def adversarial_frames(w, h, n=N_ADV):
    fw, fh = max(w, 8), max(h, 8)
    out, r = [], 0
    while len(out) < n:
        rng = np.random.default_rng(w * 1000 + h + 7919 * r)   # round 0: the frames of test_encode_vs_oracle_shapes_and_content
        noise = [rng.integers(0, 1 << 24, size=(h, w), dtype=np.uint32) for _ in range(3)]
        flat = [np.full((h, w), c, np.uint32) for c in FLATS[r % len(FLATS)]]
        again = [noise[0].copy(), noise[0] ^ np.uint32(0x010101)]
        synth = [S.synth_frame(fw, fh, 4 * r + t)[:h, :w] for t in range(4)]
        if r & 1:                                              # odd rounds: the same kinds in another order (see above)
            out += [synth[0], noise[0], noise[1]] + again + flat + [noise[2]] + synth[1:]
        else:
            out += noise + flat + again + synth
        r += 1
    return np.stack(out[:n])


class Clip:
    """frames [n, h, w], the palettes, and what the oracle makes of them from frame_count 0: bytes per frame, entries [n, h*w]"""


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_clip(w, h, mode512, n=N_ADV):
    c = Clip()
    c.w, c.h, c.mode512, c.n = w, h, mode512, n
    c.frames = _frozen(adversarial_frames(w, h, n))
    c.pal = tuple(_frozen(p) for p in S.content_palettes(c.frames[:5]))
    enc = O.OracleEncoder(w, h, mode512, *c.pal)
    both = [enc.encode(f, want_entries=True) for f in c.frames]
    enc.close()
    c.bytes = [_frozen(b) for b, _ in both]
    c.entries = _frozen(np.stack([e for _, e in both]))
    return c


def rows_of(bytes_list, stride):
    """[len, stride] zero padded, and the sizes"""
    rows = np.zeros((len(bytes_list), stride), np.uint8)
    for i, b in enumerate(bytes_list):
        assert len(b) <= stride
        rows[i, :len(b)] = b
    return rows, np.array([len(b) for b in bytes_list], np.int32)


# ---- ticket order -----------------------------------------------------------------------------------------------------
def n_groups(n_frames, first_fc=0):
    return (n_frames + (first_fc & 3) + 3) // 4


def group_frames(g, n_frames, first_fc=0):
    """[lo, hi) of the batch's frames in its group g; the first group is short when the batch starts inside a GOP"""
    phase = first_fc & 3
    return (0 if g == 0 else 4 * g - phase), min(4 * g - phase + 4, n_frames)


def group_of_frame(f, first_fc=0):
    return (f + (first_fc & 3)) // 4


def ticket_tile_group(t, n_frames, first_fc=0):
    ng = n_groups(n_frames, first_fc)
    return t // ng, t % ng


def items_in_ticket_order(n_frames, tpf, first_fc=0):
    """every (tile, frame) item of a batch in the order ONE workgroup runs them: ticket by ticket, the ticket's frames in order"""
    for t in range(n_groups(n_frames, first_fc) * tpf):
        tile, g = ticket_tile_group(t, n_frames, first_fc)
        lo, hi = group_frames(g, n_frames, first_fc)
        for f in range(lo, hi):
            yield tile, f


def item_tile_frame(k, n_frames):
    """item k of a single workgroup: the groups of a tile cover the batch's frames once, in order"""
    return k // n_frames, k % n_frames


def wrap_marker_groups(n_frames, tpf, first_fc=0):
    """the groups that hold items 65534 .. 65537 of a single workgroup (the 16-bit tag (it + 1) & 0xffff is 0 at item 65535), and
    the first and the last group"""
    assert n_frames * tpf > 65537
    gs = {0, n_groups(n_frames, first_fc) - 1}
    for k in range(65534, 65538):
        gs.add(group_of_frame(item_tile_frame(k, n_frames)[1], first_fc))
    return sorted(gs)


# ---- periodic clip ----------------------------------------------------------------------------------------------------
def marker_frames(w, h, g, m):
    return np.random.default_rng([w, h, g, 0x4D]).integers(0, 1 << 24, size=(m, h, w), dtype=np.uint32)


class Periodic:
    """base[t % P] for t < n_frames, marker GOPs over `marker_groups`; from frame_count 0.
    rows [P + marker frames, stride] / row_sizes: the expected bytes; row_of[t]: the row of frame t"""

    def __init__(self, w, h, mode512, n_frames, marker_groups, stride=None):
        base = oracle_clip(w, h, mode512, P)
        self.w, self.h, self.mode512, self.n, self.pal, self.base = w, h, mode512, n_frames, base.pal, base.frames
        stride = stride or O.max_usize(w, h)
        self.row_of = np.arange(n_frames, dtype=np.int64) % P
        exp, self.markers = list(base.bytes), {}
        for g in sorted(set(marker_groups)):
            lo, hi = group_frames(g, n_frames)
            assert 0 <= lo < hi, "marker group %d outside the clip" % g
            pix = marker_frames(w, h, g, hi - lo)
            enc = O.OracleEncoder(w, h, mode512, *self.pal, first_frame_count=4 * g)
            self.row_of[lo:hi] = len(exp) + np.arange(hi - lo)
            exp += [enc.encode(f) for f in pix]
            enc.close()
            self.markers[g] = pix
        self.rows, self.row_sizes = rows_of(exp, stride)

    def frame(self, t):
        """pixels of frame t (host; the CPU test's view of the clip)"""
        g = t // 4
        return self.markers[g][t - 4 * g] if g in self.markers else self.base[t % P]

    def pixels(self, torch, device):
        """the clip as an int32 tensor [n, h, w] on `device`"""
        base = torch.from_numpy(self.base.view(np.int32).copy()).to(device)
        pix = base[torch.arange(self.n, device=device) % P]
        for g, m in self.markers.items():
            pix[4 * g:4 * g + len(m)] = torch.from_numpy(m.view(np.int32)).to(device)
        return pix


# ---- comparison on the device -----------------------------------------------------------------------------------------
def mismatched_frames(torch, out, sizes, rows, row_sizes, row_of, chunk_bytes=64 << 20):
    """frames whose size, or any byte below the expected size, differs from rows[row_of[t]]: every frame, every such byte,
    in chunks of frames.  Bytes at and above the expected size are unspecified and masked.
    out u8 [n, stride], sizes i32 [n], rows u8 [R, stride], row_sizes i32 [R], row_of i64 [n]: tensors on one device"""
    n, stride = out.shape
    assert rows.shape[1] == stride and sizes.shape == (n,) and row_of.shape == (n,) and row_sizes.shape == (rows.shape[0],)
    col = torch.arange(stride, device=out.device)[None, :]
    step = max(1, chunk_bytes // stride)
    bad = []
    for a in range(0, n, step):
        r = row_of[a:a + step]
        es = row_sizes[r]
        diff = ((out[a:a + step] != rows[r]) & (col < es[:, None])).any(dim=1) | (sizes[a:a + step] != es)
        bad.append(diff.nonzero().flatten() + a)
    return torch.cat(bad).cpu().tolist()
