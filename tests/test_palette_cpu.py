"""The palette refinement without a GPU: AGMV_BuildPaletteRefined with no rounds is AGMV_BuildPalette and opens no device, the numpy
statement of the refinement (tests/palette_cases.py) behaves like Lloyd's algorithm on the golden clip's histograms, and
encode_frames checks palette_refine before anything else."""

import numpy as np
import pytest

import hostlib as H
import palette_cases as PC

QUALITIES = (PC.HIGH, PC.MID, PC.LOW)


def refined_lib():
    L = H.lib()
    return L


HISTS = [("fox-%d" % q, q) for q in QUALITIES] + [("sparse-%d" % q, q) for q in (PC.HIGH, PC.LOW)]


@pytest.mark.parametrize("name,quality", HISTS, ids=[n for n, _ in HISTS])
@pytest.mark.parametrize("opt", (PC.OPT_II, PC.OPT_III), ids=("opt2", "opt3"))
def test_no_rounds_is_build_palette(name, quality, opt):
    """... on a machine without a GPU too: with iterations = 0 no device is opened"""
    L = refined_lib()
    hist = np.ascontiguousarray(PC.fox_hist(quality) if name.startswith("fox") else PC.sparse_hist())
    want0, want1 = PC.build_palette(hist, quality, opt)
    p0, p1 = np.full(256, 0xA5A5A5A5, np.uint64), np.full(256, 0xA5A5A5A5, np.uint64)
    sse = np.full(2, 77, np.uint64)
    assert L.AGMV_BuildPaletteRefined(hist.ctypes.data, quality, opt, p0.ctypes.data, p1.ctypes.data, 0, sse.ctypes.data) == 0
    assert (p0 == want0).all() and (p1 == want1).all()
    assert L.AGMV_BuildPaletteRefined(hist.ctypes.data, quality, opt, p0.ctypes.data, p1.ctypes.data, 0, None) == 0      # sse may be NULL
    assert (p0 == want0).all() and (p1 == want1).all()


def test_refused_arguments():
    L = refined_lib()
    hist, p = np.zeros(1 << 19, np.uint32), np.zeros(256, np.uint64)
    for args in ((None, 1, 3, p.ctypes.data, p.ctypes.data), (hist.ctypes.data, 1, 3, None, p.ctypes.data), (hist.ctypes.data, 1, 3, p.ctypes.data, None),
                 (hist.ctypes.data, 0, 3, p.ctypes.data, p.ctypes.data), (hist.ctypes.data, 4, 3, p.ctypes.data, p.ctypes.data),
                 (hist.ctypes.data, 1, 0, p.ctypes.data, p.ctypes.data), (hist.ctypes.data, 1, 9, p.ctypes.data, p.ctypes.data)):
        for iterations in (0, 3):                                 # refused before a device would be opened
            assert L.AGMV_BuildPaletteRefined(*args, iterations, None) == -1


def test_slot_map_and_its_inverse():
    """the numpy slot map is AGMV_BuildPalette's: scattering the start the drivers use gives back the library's palettes"""
    for quality in QUALITIES:
        for opt, mode512 in ((PC.OPT_II, False), (PC.OPT_III, True)):
            p0, p1 = PC.build_palette(PC.fox_hist(quality), quality, opt)
            start = PC.start_of(p0, p1, mode512)
            assert len(start) == (512 if mode512 else 256)
            q0, q1 = PC.slots(start, mode512)
            assert (q0 == p0).all() and (q1 == p1).all()
            if mode512:
                assert p0[126] == 0 and start[511] == 0


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("k,n_free", PC.SHAPES)
def test_statement_on_the_golden_clip(quality, k, n_free):
    start, run = PC.fox_run(quality, k)
    trace = run["trace"]
    print("quality %d, k %d: %d rounds, distortion %d -> %d (ratio %.3f)" % (quality, k, run["rounds"], trace[0], trace[-1], trace[-1] / trace[0]))
    assert all(b <= a for a, b in zip(trace, trace[1:])), "the distortion rose in a round: %s" % trace
    assert trace[-1] < trace[0]
    assert run["sse"] == (trace[0], trace[-1]) and 1 <= run["rounds"] <= 16
    assert (run["pal"][n_free:] == start[n_free:]).all()           # pinned
    # no rounds: the input, measured
    none = PC.refine(PC.fox_hist(quality), quality, start, n_free, 0)
    assert (none["pal"] == start).all() and none["rounds"] == 0 and none["sse"][0] == none["sse"][1] == trace[0]
    # a shorter run is a prefix of the longer one
    one = PC.refine(PC.fox_hist(quality), quality, start, n_free, 1)
    short = PC.at(run, 1)
    assert (one["pal"] == short["pal"]).all() and one["rounds"] == short["rounds"] and one["sse"] == short["sse"]


def test_statement_on_the_crafted_cases():
    """what each crafted histogram is there for, in the statement itself (the GPU tests hold the kernel to the statement)"""
    cases = PC.crafted()
    run = {n: PC.refine(h, q, p, nf, it) for n, (q, h, p, nf, it) in cases.items()}
    pal = {n: c[2] for n, c in cases.items()}
    assert run["tie_lowest_index_wins"]["pal"][0] == PC.rgb(102, 102, 101) and run["tie_lowest_index_wins"]["pal"][2] == pal["tie_lowest_index_wins"][2]
    assert run["identical_centroids"]["pal"][1] == pal["identical_centroids"][1] != run["identical_centroids"]["pal"][0]
    assert run["pinned_attracts"]["pal"][2] == pal["pinned_attracts"][2] and run["pinned_attracts"]["rounds"] >= 1
    assert run["n_free_0"]["rounds"] == 0 and run["n_free_0"]["sse"][0] == run["n_free_0"]["sse"][1] > 0
    assert run["k_1"]["rounds"] == 1
    assert run["single_bin"]["pal"][1] == PC.rgb(132, 62, 12) and run["single_bin"]["sse"][1] == 0
    assert (run["all_zero"]["pal"] == pal["all_zero"]).all() and run["all_zero"]["sse"] == (0, 0) and run["all_zero"]["rounds"] == 0
    assert run["full_bins_round_half_up"]["pal"][0] == PC.rgb(3, 3, 2)
    assert 1 <= run["early_stop"]["rounds"] < 64 and len(run["early_stop"]["trace"]) == run["early_stop"]["rounds"] + 1


@pytest.mark.parametrize("bad", (True, 1.5, 0, -1, 65), ids=repr)
def test_encode_frames_refuses_palette_refine(bad, tmp_path):
    """... on a CPU tensor, which a later check would refuse: the argument is looked at first, before the library or a device"""
    import torch

    import libagmv_amd
    frames = torch.zeros((4, 16, 16), dtype=torch.int32)
    with pytest.raises(ValueError, match="palette_refine"):
        libagmv_amd.encode_frames(str(tmp_path / "x.agmv"), frames, palette_refine=bad, scale="no such filter")
    assert not (tmp_path / "x.agmv").exists()
