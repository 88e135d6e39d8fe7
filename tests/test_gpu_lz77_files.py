"""File level with AGMV_LZ77_DEVICE=1 (agmv_pipeline.c: the LZ77 stage on the GPU workers, the persistent buffer behind
the streams on the device): LZ77 files must come out byte-identical to the host stage's and to the reference's; LZSS files
and sequences over more than one device are unaffected by the knob."""
import hashlib
import json
import os

import numpy as np
import pytest

import children as K
import hostlib as H
import oracles as O
import synth as S

pytestmark = pytest.mark.gpu

def encode(tmp_path, sub, so, T, W, Hh, opt, q, comp, batch, frame=S.synth_frame, **env):
    """the clip frame(W, Hh, t), t = 1..T, through the drop-in API in a child process: (bytes of the .agmv file, stderr)"""
    fr = tmp_path / ("fr_%dx%d" % (W, Hh))
    if not fr.exists():
        fr.mkdir()
        for t in range(1, T + 1):
            H.write_bmp(str(fr / ("f%d.bmp" % t)), frame(W, Hh, t))
    d = tmp_path / sub
    d.mkdir()
    os.symlink(str(fr), str(d / "fr"))
    e = dict(dict.fromkeys(("AGMV_LZ77_DEVICE", "AGMV_LZ_DEVICE", "AGMV_DEVICES", "AGMV_DEVICES_OVERSUBSCRIBE")), **env, AGMV_TRACE="1")
    r = K.drive_child(d, "agmv", T, W, Hh, opt, q, comp, batch, so=None if so == H.SO else so, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return open(d / "out.agmv", "rb").read(), r.stderr


def golden_case(golden, tmp_path, name, **env):
    g = golden["files"][name]
    assert g["driver"] == "agmv"
    H.lib()
    data, err = encode(tmp_path, "run", H.SO, g["T"], g["W"], g["H"], g["opt"], g["quality"], g["compression"], 8, **env)
    assert len(data) == g["file_len"]
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"
    return err


def test_lz77_golden_through_the_device_stage(golden, tmp_path):
    err = golden_case(golden, tmp_path, "agmv_opt2_low_lz77_160x128", AGMV_LZ77_DEVICE="1")
    assert b"LZ (device)" in err, err.decode()[-2000:]


def test_lz77_golden_with_the_knob_off_stays_on_the_host(golden, tmp_path):
    err = golden_case(golden, tmp_path, "agmv_opt2_low_lz77_160x128", AGMV_LZ77_DEVICE="0")
    assert b"LZ (host)" in err, err.decode()[-2000:]


def test_lzss_golden_is_unaffected_by_the_knob(golden, tmp_path):
    err = golden_case(golden, tmp_path, "c2_agmv_opt3_low_lzss_320x240", AGMV_LZ77_DEVICE="1")
    assert b"LZ (host)" in err, err.decode()[-2000:]


@pytest.mark.parametrize("shape", [(320, 240, 26, 3), (640, 360, 22, 2)])
def test_sequences_across_batches_knob_on_and_off(tmp_path, shape):
    """batches of 4 frames: the persistent buffer crosses batches, the two workers take turns, frame sizes differ"""
    W, Hh, T, opt = shape
    H.lib()
    off, err0 = encode(tmp_path, "off", H.SO, T, W, Hh, opt, 1, 2, 4)
    on, err1 = encode(tmp_path, "on", H.SO, T, W, Hh, opt, 1, 2, 4, AGMV_LZ77_DEVICE="1")
    assert b"LZ (host)" in err0 and b"LZ (device)" in err1, err1.decode()[-2000:]
    assert int.from_bytes(on[4:8], "little") > 8                     # more than two batches
    assert on == off


def test_two_devices_keep_the_host_stage(tmp_path):
    """AGMV_DEVICES=2: the persistent buffer would have to travel between the devices in batch order; the LZ77 stage stays
    on the host pool and the trace says so"""
    W, Hh, T, opt = 320, 240, 26, 3
    H.lib()
    one, _ = encode(tmp_path, "one", H.SO, T, W, Hh, opt, 1, 2, 4)
    two, err = encode(tmp_path, "two", H.SO, T, W, Hh, opt, 1, 2, 4, AGMV_LZ77_DEVICE="1", AGMV_DEVICES="2",
                      AGMV_DEVICES_OVERSUBSCRIBE="1")
    assert b"4 GPU workers" in err and b"LZ (host)" in err and b"LZ (device)" not in err, err.decode()[-2000:]
    assert two == one


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built here")
def test_device_stage_writes_the_compiled_reference_s_file(tmp_path):
    W, Hh, T, opt = 64, 48, 40, 2
    H.lib()
    ref, _ = encode(tmp_path, "ref", O.REF_SO, T, W, Hh, opt, 1, 2, 4)
    on, err = encode(tmp_path, "on", H.SO, T, W, Hh, opt, 1, 2, 4, AGMV_LZ77_DEVICE="1")
    assert b"LZ (device)" in err
    assert int.from_bytes(ref[4:8], "little") > 8
    assert on == ref


def growing_frame(W, Hh, t):
    """frames 1-8: one flat colour each (FILL blocks, a few hundred bytes of bitstream); from frame 9 on: seeded uniform
    noise (NORMAL blocks of at least 17 bytes each)"""
    if t <= 8:
        return np.full((Hh, W), (29 * t) << 16 | (40 + 17 * t) << 8 | (255 - 23 * t), np.uint32)
    return np.random.default_rng(0xA6D5 + t).integers(0, 1 << 24, (Hh, W), dtype=np.uint32)


def chunk_sizes(data):
    """(usize, csize) of every frame chunk of a file without audio, walked from chunk to chunk"""
    out, at = [], data.find(b"AGFC")
    while at >= 0:
        u, c = int.from_bytes(data[at + 8:at + 12], "little"), int.from_bytes(data[at + 12:at + 16], "little")
        out.append((u, c))
        at = data.find(b"AGFC", at + 16 + c)
    return out


def grows(totals, slack):
    """does a buffer that is sized to the first total it cannot hold, plus a quarter plus `slack`, grow a second time?"""
    cap, times = 0, 0
    for t in totals:
        if t + 16 > cap:
            cap, times = t + t // 4 + slack, times + 1
    return times > 1


@pytest.mark.parametrize("T", [16, 48])
def test_buffers_grow_after_the_first_batch(tmp_path, golden_dir, T):
    """a clip whose streams grow (opt 2 encodes about every other source frame).  A worker's LZ77 payload rows are sized by
    the largest stream of the first batch it sees plus 25 %, and a batch slot's pinned download buffer by the first batch it
    holds plus 25 % + 4096 bytes; both have to grow when the noise frames arrive.  Batch b goes to worker b % 2 and to
    slot b % 4: the 16-frame clip makes the rows grow, but has fewer batches than slots; in the 48-frame clip the slots
    come round again and the download buffer grows too (bitstreams with the host stage, payloads with the device
    stages).  Both facts are checked from the sizes in the file.  The LZ77 file of the 16-frame clip must be the compiled
    reference's."""
    W, Hh, opt = 64, 48, 2
    H.lib()
    for comp, knob in ((2, "AGMV_LZ77_DEVICE"), (1, "AGMV_LZ_DEVICE")):
        off, err0 = encode(tmp_path, "off%d" % comp, H.SO, T, W, Hh, opt, 1, comp, 4, frame=growing_frame)
        on, err1 = encode(tmp_path, "on%d" % comp, H.SO, T, W, Hh, opt, 1, comp, 4, frame=growing_frame, **{knob: "1"})
        assert b"LZ (host)" in err0 and b"LZ (device)" not in err0, err0.decode()[-2000:]
        assert b"LZ (device)" in err1 and b"LZ (host)" not in err1, err1.decode()[-2000:]
        assert on == off
        sizes = chunk_sizes(on)
        print(T, comp, sizes)
        assert len(sizes) == int.from_bytes(on[4:8], "little")
        batches = [sizes[b:b + 4] for b in range(0, len(sizes), 4)]
        tops = [max(u for u, _ in b) for b in batches]
        # the rows: a worker's later batch has a stream more than five times its largest before (the slack is 1.25)
        assert any(tops[b] > 5 * max(tops[b % 2:b:2]) for b in range(2, len(batches))), sizes
        if T > 16:
            for which, pad in ((0, 1), (1, 0)):                      # bitstreams + 1 (host stage), payloads (device stages)
                assert any(grows([sum(s[which] + pad for s in b) for b in batches[slot::4]], 4096) for slot in range(4)), (which, sizes)
        elif comp == 2:                                              # the compiled reference's file of this clip, recorded: it
            g = json.load(open(os.path.join(golden_dir, "lz77_growing_clip.json")))     # takes minutes to make (see the fixture)
            assert (g["T"], g["W"], g["H"], g["opt"], g["compression"]) == (T, W, Hh, opt, comp)
            assert len(on) == g["file_len"] and hashlib.sha256(on).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"
