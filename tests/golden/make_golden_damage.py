#!/usr/bin/env python3
"""What the COMPILED REFERENCE makes of the damaged files of tests/damage_cases.py (build container only; needs oracle/_ref):
    python tests/golden/make_golden_damage.py

  golden_damage.json     per case: the sha256 of the file image, its geometry, and per frame of the header's count
                         [return code, bpos, sha256 of the pixels, sha256 of bitstream[:bpos + 16]] as AGMV_DecodeFrameChunk
                         leaves them (the 16 bytes behind bpos are what the block parser may read on an over-run)

Hashes and integers only.  The corpus asserts its own bounds before the reference sees a file (damage_cases.layout)."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import damage_cases as D  # noqa: E402
import oracles as O  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ref_record(case, td):
    """the fixture entry of one case from the compiled reference"""
    img = D.file_image(case)
    path = os.path.join(td, "d.agmv")
    with open(path, "wb") as f:
        f.write(img)
    err, (w, h, n, ver), fr = O.ref_decode_file(path, want_bitstream=True)
    assert err == 0 and (w, h, n, ver) == (case["w"], case["h"], len(D.layout(case)[1]), case["version"]), (case["name"], err)
    return {"file_sha": hashlib.sha256(img).hexdigest(), "w": w, "h": h, "version": ver,
            "frames": [[f["err"], f["bpos"], sha(f["pix"]), sha(f["bitstream"])] for f in fr]}


def main():
    O.build_oracles()
    assert O.have_ref()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for case in D.cases():
            out[case["name"]] = ref_record(case, td)
            ok = sum(1 for f in out[case["name"]]["frames"] if f[0] == 0)
            print("%-22s %4d x %-4d v%d  %2d frames, %2d decoded" % (case["name"], case["w"], case["h"], case["version"], len(case["frames"]), ok), flush=True)
    json.dump(out, open(os.path.join(HERE, "golden_damage.json"), "w"), indent=0, sort_keys=True)
    print("%d cases, %d frames" % (len(out), sum(len(c["frames"]) for c in out.values())))


if __name__ == "__main__":
    main()
