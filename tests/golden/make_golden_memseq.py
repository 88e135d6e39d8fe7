#!/usr/bin/env python3
"""Fixture of the mixed adaptive clip (build container only: needs the reference tree and oracle/_ref):
    python tests/golden/make_golden_memseq.py

  golden_memseq.json   the compiled reference's AGMV_EncodeVideo (LOW quality, LZSS; OPT_III, OPT_I, OPT_II) over the clip of
                       tests/memseq_cases.py:mixed_clip(), on which the frame skipping takes both of its branches: file hash,
                       length, frame count and rate field, plus the decisions of the chain

The two older EncodeVideo goldens (golden.json video_opt3_low_lzss_160x128, golden_r3.json encodevideo_212) pass the similarity
test in every group, so they never pinned the not-similar branch.  Hashes and numbers only."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import hostlib as Hh  # noqa: E402
import memseq_cases as MC  # noqa: E402
import oracles as O  # noqa: E402
import make_golden as M  # noqa: E402

LENIENCY = {3: 0.2282, 1: 0.2282, 2: 0.1282}
HEAVY = {3: False, 1: True, 2: False}


def main():
    O.build_oracles()
    assert O.have_ref(), "reference build missing"
    R = Hh.bind(C.CDLL(O.REF_SO), missing_ok=True)
    clip = MC.mixed_clip()
    T, H, W = clip.shape
    wide = [np.ascontiguousarray(f.reshape(-1)).astype(np.uint64) for f in clip]
    ratio = [float(R.AGMV_CompareFrameSimilarity(wide[k], wide[k + 1], W, H)) for k in range(T - 1)]    # pair (k + 1, k + 2)
    print("adjacent-pair ratios:", " ".join("%.4f" % r for r in ratio), flush=True)
    out = {}
    for name, (opt, q, comp) in MC.MIXED_CASES.items():
        len32 = float(np.float32(LENIENCY[opt]))
        chain = MC.adaptive_chain(lambda x: np.float32(ratio[x - 1]) >= np.float32(len32), T, HEAVY[opt])
        assert chain.count(True) >= 2 and chain.count(False) >= 2, (name, chain)
        with tempfile.TemporaryDirectory() as td:
            os.mkdir(os.path.join(td, "fr"))
            for t in range(1, T + 1):
                Hh.write_bmp(os.path.join(td, "fr", "f%d.bmp" % t), clip[t - 1])
            subprocess.run([sys.executable, "-c", M.REF_DRIVER % O.REF_SO, "video", str(T), str(W), str(H), str(opt), str(q), str(comp)],
                           cwd=td, stdout=subprocess.DEVNULL, check=True)
            data = open(os.path.join(td, "out.agmv"), "rb").read()
        out[name] = {"driver": "video", "T": T, "W": W, "H": H, "opt": opt, "quality": q, "compression": comp,
                     "file_sha": hashlib.sha256(data).hexdigest(), "file_len": len(data),
                     "frames": int.from_bytes(data[4:8], "little"), "fps_field": int.from_bytes(data[18:22], "little"),
                     "chain": [int(c) for c in chain]}
        # the file agrees with the chain walked here from the reference's own ratios
        assert out[name]["frames"] == sum((1 if HEAVY[opt] else 3) if c else 1 for c in chain), (name, chain, out[name]["frames"])
        print(name, out[name], flush=True)
    json.dump(out, open(os.path.join(HERE, "golden_memseq.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
