"""The stream families of tests/lz77_cases.py that tests/test_gpu_lz77_edges.py puts to the GPU, pinned on the CPU first: the
host stage (agmv_lz77_mem) against the brute-force restatement (orc_lz77_compress) on streams longer than the window, and
the tokens the families state in closed form against the brute force and against a numpy statement of one token
(lz77_cases.token_at).  A fixture of the window's low edge must decide: under a window of 65 538 bytes the same stream gives
another token.  The brute force costs about 0.5 s per 70 KB of noise, so it meets a slice of the low-edge family (the first
and the last offset into a segment); the host stage and token_at meet all 408 streams."""
import numpy as np
import pytest

import lz77_cases as Z
from lz77_cases import WIN, host77, orc77, same, token_at, token_starting_at


@pytest.mark.parametrize("out", Z.EDGE_OUT)
@pytest.mark.parametrize("L", Z.EDGE_L)
@pytest.mark.parametrize("i", [Z.EDGE_I[0], Z.EDGE_I[-1]])
def test_low_edge_slice_host_is_brute_force(i, L, out):
    for inside in Z.EDGE_INSIDE:
        if inside == "shorter" and L < 2:
            continue
        x = Z.edge_stream(i, L, out, inside)
        exp = orc77(x)
        assert same(host77(x), exp), (i, L, out, inside)
        assert token_starting_at(exp, i) == Z.edge_token(i, L, out, inside), (i, L, out, inside)


def test_low_edge_family_is_complete():
    grid = Z.edge_grid()
    assert len(grid) == 408 and len(set(grid)) == 408
    for i in Z.EDGE_I:
        assert i > WIN + max(Z.EDGE_OUT) and 0 < i % Z.SEG                      # bytes below i - 65535 are staged with the segment
        S = i - i % Z.SEG
        assert (i - WIN) - (S - WIN) >= 1


@pytest.mark.parametrize("L", Z.EDGE_L)
@pytest.mark.parametrize("i", Z.EDGE_I)
def test_low_edge_tokens_are_stated_and_decisive(i, L):
    """every stream of the family: the stated token is the host stage's and the numpy statement's under a window of 65 535,
    and for a copy that starts below the window a window of 65 538 gives another token"""
    cases = [c for c in Z.edge_grid([i]) if c[1] == L]
    assert len(cases) == (8 if L < 2 else 12)
    for (_, _, out, inside) in cases:
        x = Z.edge_stream(i, L, out, inside)
        exp = Z.edge_token(i, L, out, inside)
        assert token_starting_at(host77(x), i) == exp, (i, L, out, inside)
        assert token_at(x, i, WIN) == exp, (i, L, out, inside)
        wide = token_at(x, i, WIN + 3)
        if out > 0:
            assert wide != exp and wide == (WIN + out, L, 251), (i, L, out, inside)
        else:
            assert wide == exp, (i, L, out, inside)


def test_token_at_is_the_brute_force_token():
    """the numpy statement of one token against the brute force at every token start of short streams"""
    for seed in range(6):
        x = Z.bitstream_like(seed, n=700)
        at = 0
        for t in Z.tokens77(orc77(x, 0x5A)):
            assert token_at(x, at, WIN, 0x5A) == t, (seed, at)
            at += t[1] + 1
    x = np.array([7, 1, 2, 7, 3, 4, 7, 5, 6, 7, 8], np.uint8)
    assert token_at(x, 9) == (9, 1, 8) and token_at(x, 9, 5) == (3, 1, 8) and token_at(x, 0) == (0, 0, 7)


@pytest.mark.parametrize("E,k,tail", Z.ahead_grid())
def test_lookahead_family_host_is_brute_force(E, k, tail):
    i = E - 1 - k
    x = Z.ahead_stream(E, k, tail)
    assert len(x) == i + 255 + tail
    for peek in (0, 0x5A):
        exp = orc77(x, peek)
        assert same(host77(x, peek), exp), peek
        assert token_starting_at(exp, i) == Z.ahead_token(E, k, tail, peek), peek
        assert token_at(x, i, WIN, peek) == Z.ahead_token(E, k, tail, peek), peek


def test_lookahead_family_is_complete():
    assert len(Z.ahead_grid()) == 72 and len(set(Z.ahead_grid())) == 72


@pytest.mark.parametrize("m", Z.SHIFT_M)
def test_shifted_family_host_is_brute_force(m):
    for k in range(0, 256, 17):
        x = Z.shifted_stream(k, m)
        assert len(x) == k + 3 * Z.SEG
        assert same(host77(x), orc77(x)), (k, m)


@pytest.mark.parametrize("m", Z.SHIFT_M)
def test_exit_family_host_is_brute_force_and_exits_as_stated(m):
    """the second segment is entered off a recorded start, and the parse from there ends as exit_stream states"""
    E = 2 * Z.SEG
    for k in range(0, 255, 34):
        x = Z.exit_stream(k, m)
        assert len(x) == 3 * Z.SEG
        assert same(host77(x), orc77(x)), (k, m)
        entry, end, merged = Z.stitch_model(x, 1)
        assert entry == Z.SEG + 1 + k and entry % 256 != 0, (k, m)
        assert (end, merged) == ((E, False) if m == 1 else (E - m + 1, True)), (k, m)
    assert Z.stitch_model(Z.exit_stream(255, m), 1)[0] == Z.SEG                    # k = 255 enters on a recorded start


@pytest.mark.parametrize("seed", range(Z.DEEP_SEEDS))
def test_deep_fuzz_host_is_brute_force(seed):
    x = Z.deep_stream(seed)
    assert 70_000 <= len(x) <= 300_000
    assert same(host77(x, 0x33), orc77(x, 0x33)), seed


def test_lz77_window_limit_and_long_input():
    """matches must start within 65535 bytes: a repeat 70000 bytes later must not be found (the LZ77 twin of
    test_hostlib.test_lz_window_limit_and_long_input)"""
    x = Z.window_limit_stream()
    exp = orc77(x)
    assert same(host77(x), exp)
    i = len(x) - 64
    assert token_at(x, i, i)[:2] == (i, 64)                                     # a window that reaches the first block finds it
    # 70 000 x 65 535 pairs of starts in uniform noise agree in 8 bytes with probability 2^-64 each
    assert max(t[1] for t in Z.tokens77(exp)) < 8
