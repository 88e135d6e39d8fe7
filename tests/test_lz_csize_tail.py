"""The LZSS csize tail rule on the host: above 2^24 output bits the reference's float csize can count the partially
filled last byte, and its file then holds that byte (reference src/agmv_encode.c:176, src/agmv_utils.c:106-112)."""
import numpy as np

import hostlib as H
import lzss_cases as Z


def test_all_literal_stream_above_2_24_bits_keeps_the_partial_byte():
    x = Z.all_literal_stream()
    n = len(x)
    assert n % 8 == 7 and (1 << 24) <= 9 * n < (1 << 25)
    assert not Z.has_repeated_3gram(x)
    exp, ecs = Z.literal_payload(x)
    assert ecs == 9 * n // 8 + 1                                     # the float rounded up: the partial byte is payload
    out = np.full(2 * n + 64, 0xAA, np.uint8)                        # sentinel: a byte the sink never wrote shows as 0xAA
    cs = H.lib().agmv_lzss_mem(np.concatenate([x, np.zeros(8, np.uint8)]), n, out)
    assert cs == ecs
    assert (out[:9 * n // 8] == exp[:9 * n // 8]).all()
    assert out[cs - 1] == exp[-1], "last payload byte %#x, reference %#x" % (out[cs - 1], exp[-1])


def test_literal_payload_matches_the_host_below_2_24_bits():
    """the closed form itself, on a short stream where csize is exact"""
    x = Z.all_literal_stream(5003, seed=1)
    exp, ecs = Z.literal_payload(x)
    got, cs = H.lzss(x)
    assert cs == ecs == 9 * len(x) // 8 and (got == exp).all()
