"""A view of a clip (AGMV_VIEW of include/agmv.h, agmv_hip_view_frames_async of include/agmv_hip_view.h) stated in numpy, and the
selection of a view's frames inside one batch of the decoder stated by enumeration.  Nothing here calls the code under test."""
import numpy as np


def view(full, first=0, count=0, step=1, x=0, y=0, width=0, height=0, cap=None):
    """full: [n, h, w] (any dtype) -> frames first, first + step, ... of it (at most `count` where count != 0, at most `cap` where
    given), of each the window [x, x + width) x [y, y + height); width == height == 0 is the full frame"""
    sel = full[first::step]
    if count:
        sel = sel[:count]
    if cap is not None:
        sel = sel[:cap]
    if width or height:
        sel = sel[:, y:y + height, x:x + width]
    return np.ascontiguousarray(sel)


def length(first, step, count, nframes):
    """the frames of a view in a file of nframes frames (count 0: to the end)"""
    return len(frames_of(first, step, count, nframes))


def frames_of(first, step, count, nframes):
    """the file's frame of every frame of the view, in the view's order"""
    fr = list(range(first, nframes, step))
    return fr[:count] if count else fr


def in_batch(first, step, count, batch_first, batch_n, nframes):
    """(length, row of the first in the batch, view index of the first) of the view's frames inside [batch_first, batch_first +
    batch_n), by enumeration; (0, None, None) for none"""
    hit = [(f - batch_first, j) for j, f in enumerate(frames_of(first, step, count, nframes)) if batch_first <= f < batch_first + batch_n]
    if not hit:
        return 0, None, None
    assert all(b[0] - a[0] == step and b[1] - a[1] == 1 for a, b in zip(hit, hit[1:]))      # an arithmetic progression, consecutive in the view
    return len(hit), hit[0][0], hit[0][1]


def clip(n, h, w, seed, high=0x7E000000):
    """n frames of h x w distinct-looking words with bits 24 .. 31 set: a copy that masks or reorders shows"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 24, (n, h, w), dtype=np.uint32) | np.uint32(high)).astype(np.uint32)
