"""agmv_hip_palette_refine_dev, the weighted k-means over a histogram of AGMV_QuantizeColor codes ("palette refinement" of
include/agmv.h), through AgmvHip against the numpy statement (tests/palette_cases.py).  Everything is exact: the colours, the
number of rounds and both distortions must be the statement's, the histogram must come back as it went, and the words around
the palette must keep their value.  The golden clip's histograms from the start the drivers use, and crafted histograms for the
tie rule, empty and pinned centroids, the edges of the code range, 64-bit sums and the early stop.  Needs an MI355X."""
import numpy as np
import pytest

import palette_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 16
FILL = 0x5A5A5A5A


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


def run(torch, hip, hist, quality, pal, n_free, iterations):
    """-> the statement's dict from the device: pal, rounds, sse; asserts that the histogram and the guard words kept their value"""
    hist = np.array(hist, np.uint32)                          # (writable copies: torch.from_numpy wants them)
    pal = np.array(pal, np.uint32)
    d_hist = torch.from_numpy(hist.view(np.int32)).cuda()
    buf = torch.full((GUARD + len(pal) + GUARD,), FILL, dtype=torch.int32, device="cuda")
    d_pal = buf[GUARD:GUARD + len(pal)]
    d_pal.copy_(torch.from_numpy(pal.view(np.int32)))
    rounds, sse = hip.palette_refine_dev(d_hist, quality, d_pal, n_free, iterations)
    torch.cuda.synchronize()
    hip.check()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "words around the palette were written"
    assert (d_hist.cpu().numpy().view(np.uint32) == hist).all(), "the histogram was modified"
    e = sse.cpu().numpy().view(np.uint64)
    return {"pal": host[GUARD:-GUARD].view(np.uint32).copy(), "rounds": int(rounds.item()), "sse": (int(e[0]), int(e[1]))}


def same(got, want, what):
    bad = np.flatnonzero(got["pal"] != want["pal"])
    assert bad.size == 0, (what, "centroids", bad[:8], [hex(v) for v in got["pal"][bad[:8]]], [hex(v) for v in want["pal"][bad[:8]]])
    assert got["rounds"] == want["rounds"], (what, "rounds", got["rounds"], want["rounds"])
    assert got["sse"] == tuple(want["sse"]), (what, "sse", got["sse"], want["sse"])


@pytest.mark.parametrize("iterations", (1, 16))
@pytest.mark.parametrize("k,n_free", PC.SHAPES)
@pytest.mark.parametrize("quality", (PC.HIGH, PC.MID, PC.LOW))
def test_golden_clip_from_the_drivers_start(torch, hip, quality, k, n_free, iterations):
    start, full = PC.fox_run(quality, k)
    want = PC.at(full, iterations)
    got = run(torch, hip, PC.fox_hist(quality), quality, start, n_free, iterations)
    print("quality %d, k %d, %d iterations: %d rounds, distortion %d -> %d" % ((quality, k, iterations, got["rounds"]) + got["sse"]))
    same(got, want, (quality, k, iterations))


CRAFTED = sorted(PC.crafted())


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_histograms(torch, hip, name):
    quality, hist, pal, n_free, iterations = PC.crafted()[name]
    want = PC.refine(hist, quality, pal, n_free, iterations)
    got = run(torch, hip, hist, quality, pal, n_free, iterations)
    same(got, want, name)
    if name == "n_free_0":
        assert got["rounds"] == 0 and got["sse"][0] == got["sse"][1] and (got["pal"] == pal).all()
    if name == "all_zero":
        assert got["rounds"] == 0 and got["sse"] == (0, 0) and (got["pal"] == pal).all()
    if name == "early_stop":
        assert got["rounds"] < iterations
    if name == "tie_lowest_index_wins":
        assert got["pal"][0] == PC.rgb(102, 102, 101) and got["pal"][2] == pal[2]
    if name == "pinned_attracts":
        assert got["pal"][2] == pal[2]
    if name == "full_bins_round_half_up":
        assert got["pal"][0] == PC.rgb(3, 3, 2)


def test_no_iterations_only_measures(torch, hip):
    start, full = PC.fox_run(PC.LOW, 256)
    got = run(torch, hip, PC.fox_hist(PC.LOW), PC.LOW, start, 256, 0)
    assert (got["pal"] == start).all() and got["rounds"] == 0 and got["sse"] == (full["trace"][0], full["trace"][0])


def test_repeatable_on_one_context(torch, hip):
    """the work area is the context's: a second call must not see the first one's sums or flag"""
    start, full = PC.fox_run(PC.MID, 512)
    for _ in range(2):
        same(run(torch, hip, PC.fox_hist(PC.MID), PC.MID, start, 511, 16), full, "repeat")


BAD = {"k_0": (1, 0, 0), "k_513": (1, 513, 0), "n_free_above_k": (1, 8, 9), "quality_0": (0, 8, 8), "quality_4": (4, 8, 8)}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_arguments_are_refused(torch, hip, name):
    quality, k, n_free = BAD[name]
    d_hist = torch.zeros(1 << 19, dtype=torch.int32, device="cuda")
    d_hist[5] = 9
    d_pal = torch.full((GUARD + 513 + GUARD,), FILL, dtype=torch.int32, device="cuda")
    out = torch.full((8,), FILL, dtype=torch.int32, device="cuda")
    rc = hip.L.agmv_hip_palette_refine_dev(hip.ctx, d_hist.data_ptr(), quality, d_pal.data_ptr() + 4 * GUARD, k, n_free, 4, out.data_ptr(),
                                           out.data_ptr() + 16, None)
    torch.cuda.synchronize()
    assert rc != 0
    msg = hip.L.agmv_hip_last_error().decode()
    assert "agmv_hip_palette_refine_dev" in msg and len(msg) > 40, msg
    assert (d_pal.cpu().numpy() == FILL).all() and (out.cpu().numpy() == FILL).all(), "a refused call wrote to the device"
