"""What the tests' child processes share.  A case runs in a child because the sequence drivers write into the CWD, keep
process-wide state and, like the reference's, free the caller's AGMV object.  A child is a fresh process per job that loads
the two libraries with bare ctypes, the way a C host would, binds them from the tables of libagmv_amd/abi.py and imports no
torch.  The job travels as JSON in argv[1]; the answer is one JSON line on stdout."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import hostlib as H
from libagmv_amd import abi
from libagmv_amd.abi import AGMV_INFO as INFO  # noqa: F401  (for the children)

HIP_SO = os.path.join(H.ROOT, "libagmv_amd", "libagmv_hip.so")

# in front of every child script: `job`, then L (job["so"]) and G (job["hip_so"]) bound from the tables, and the helpers below
PRELUDE = """import json, sys
job = json.loads(sys.argv[1])
sys.path[:0] = [job["tests"], job["root"]]
import ctypes as C
import numpy as np
from children import INFO, download, free, libraries, poisoned, upload
L, G = libraries(job)
"""
# The compiled reference runs in a child with nothing else in it: it reads heap memory it never set (its LZ77 the byte behind a
# frame's stream, src/agmv_encode.c:222), and its files are what they are in a process whose heap is fresh.  Importing numpy, json or
# even abi.py from source leaves text on the heap that changes them.  So that child gets the job as a literal and the signatures it
# needs written out from the table.
REF_DRIVERS = ("CreateAGMV", "AGMV_EncodeAGMV", "AGMV_EncodeFullAGMV", "AGMV_EncodeVideo", "AGMV_DecodeAGMV")


def ref_prelude(job):
    name = lambda t: "None" if t is None else "C." + t.__name__
    lines = ["L.%s.restype, L.%s.argtypes = %s, [%s]\n" % (n, n, name(abi.AGMV[n][0]), ", ".join(name(t) for t in abi.AGMV[n][1])) for n in REF_DRIVERS]
    return "import ctypes as C, sys\njob = %r\nL = C.CDLL(job['so'])\n" % (job,) + "".join(lines)


# a BMP driver over fr/f<t>.bmp of the CWD, then (job["decode"]) AGMV_DecodeAGMV of the file into the CWD
DRIVE = """T, W, Hh = job["T"], job["W"], job["H"]
if job["batch"] and hasattr(L, "AGMV_SetBatchFrames"):              # (the compiled reference has no batches)
    L.AGMV_SetBatchFrames(job["batch"])
args = (job["out"].encode(), b"fr", b"f", 1, 1, T, W, Hh, 24, job["opt"], job["quality"], job["compression"])
if job["driver"] == "video":
    L.AGMV_EncodeVideo(*args)
else:
    (L.AGMV_EncodeAGMV if job["driver"] == "agmv" else L.AGMV_EncodeFullAGMV)(L.CreateAGMV(T, W, Hh, 24), *args)
if job["decode"]:
    sys.exit(L.AGMV_DecodeAGMV(args[0], 1, 1))
"""
DECODE = "L.AGMV_SetBatchFrames(job['batch']) if job['batch'] else None\nsys.exit(L.AGMV_DecodeAGMV(job['path'].encode(), 1, 1))\n"

G = None


def libraries(job):
    """in a child: (libagmv.so, libagmv_hip.so)"""
    global G
    L, G = H.bind(C.CDLL(job["so"])), abi.bind(C.CDLL(job["hip_so"]), abi.HIP)
    return L, G


def upload(a):
    """a numpy array -> device pointer of its copy"""
    d = G.agmv_hip_malloc(a.nbytes)
    assert d and G.agmv_hip_memcpy_h2d(d, a.ctypes.data, a.nbytes) == 0
    return d


def download(d, nbytes):
    out = np.empty(nbytes, np.uint8)
    assert G.agmv_hip_memcpy_d2h(out.ctypes.data, d, nbytes) == 0
    return out


def poisoned(nbytes):
    """device memory of 0xA5 bytes: what a decode that does not write a byte leaves there"""
    d = G.agmv_hip_malloc(nbytes)
    assert d and G.agmv_hip_memset(d, 0xA5, nbytes) == 0
    return d


def free(d):
    G.agmv_hip_free(d)


def start_child(cwd, script, job, env=None, timeout=600, so=None, stdout=subprocess.PIPE, prelude=PRELUDE):
    """prelude + script in a fresh interpreter with `job`; the finished process.  prelude="" for a whole script of its own: one
    that imports torch must do so before a library is loaded (libagmv_amd/hip.py load_library has the reason)"""
    H.lib()
    job = dict(job, so=so or H.SO, hip_so=None if so else HIP_SO, tests=os.path.dirname(os.path.abspath(__file__)), root=H.ROOT)
    env = {k: v for k, v in dict(os.environ, **(env or {})).items() if v is not None}          # (None takes a variable out)
    return subprocess.run([sys.executable, "-c", prelude + script, json.dumps(job)], cwd=str(cwd), env=env, stdout=stdout,
                          stderr=subprocess.PIPE, timeout=timeout)


def run_child(cwd, script, job, env=None, timeout=600, prelude=PRELUDE):
    """... that must end with status 0; its answer"""
    r = start_child(cwd, script, job, env, timeout, prelude=prelude)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def decode_child(cwd, path, batch=0, env=None, timeout=600):
    """AGMV_DecodeAGMV(path) into the BMPs of `cwd` (batch 0: the library's default batches); the finished process"""
    return start_child(cwd, DECODE, {"path": str(path), "batch": batch}, env, timeout, stdout=subprocess.DEVNULL)


def drive_child(cwd, driver, T, W, Hh, opt, quality, compression, batch=0, decode=False, out="out.agmv", so=None, env=None, timeout=1200):
    """AGMV_EncodeAGMV ("agmv") / AGMV_EncodeFullAGMV ("full") / AGMV_EncodeVideo ("video") of library `so` (None: ours) over
    cwd/fr/f1.bmp .. f<T>.bmp into cwd/out, then with `decode` AGMV_DecodeAGMV of it, whose status ends the child; the finished process"""
    job = {"driver": driver, "T": T, "W": W, "H": Hh, "opt": opt, "quality": quality, "compression": compression, "batch": batch,
           "decode": decode, "out": out}
    return start_child(cwd, DRIVE, job, env, timeout, so, subprocess.DEVNULL, ref_prelude(dict(job, so=so)) if so else PRELUDE)
