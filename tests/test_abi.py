"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads, exports every symbol
include/agmv_hip.h declares, and fails LOUDLY (no CPU fallback) when there is no GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from libagmv_amd import build
    import libagmv_amd.hip as H
    build.build()
    L = H.load_library()
    hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    declared = set(re.findall(r"\b(agmv_hip_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("agmv_hip_ctx")
    assert declared == set(H.ABI_SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s


def _prototypes(header):
    """name -> (return type, [parameter declarations]) of every `ret name(args);` of a header of include/"""
    t = open(os.path.join(ROOT, "include", header)).read()
    t = re.sub(r"/\*.*?\*/", " ", t, flags=re.S)
    t = re.sub(r"//[^\n]*", " ", t)
    t = re.sub(r"^\s*#[^\n]*", " ", t, flags=re.M)
    t = re.sub(r"typedef\s+(struct|enum)\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", t, flags=re.S)
    t = re.sub(r'extern\s+"C"\s*\{', " ", t)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(\w+)\s*\(([^()]*)\)\s*;", t):
        args = " ".join(m.group(3).split())
        out[m.group(2)] = (" ".join(m.group(1).split()), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return out


_ENUMS = re.findall(r"typedef\s+enum\s+(\w+)", open(os.path.join(ROOT, "include", "agmv.h")).read())
# what a scalar is to the calling convention: (kind, bytes).  u32 is `unsigned long` in include/agmv.h.
_C_CLASS = dict({"size_t": "u8", "uint32_t": "u4", "uint64_t": "u8", "unsigned long long": "u8", "int": "i4", "Bool": "i4", "unsigned": "u4",
                 "unsigned int": "u4", "u8": "u1", "u16": "u2", "u32": "u8", "f32": "f4", "float": "f4", "void": "void"},
                **{e: "i4" for e in _ENUMS})


def _c_class(decl, is_return=False):
    """the class of a parameter declaration (type and name) or of a return type; an unknown type raises"""
    d = re.sub(r"\bconst\b", " ", decl)
    if "*" in d or "[" in d:
        return "ptr"
    words = d.split()
    if not is_return and " ".join(words) not in _C_CLASS:
        words = words[:-1]                                      # (the parameter's name)
    t = " ".join(words)
    if t in ("AGMV_ENTRY", "AGMV_INFO"):
        return t
    assert t in _C_CLASS, "unknown C type %r in %r" % (t, decl)
    return _C_CLASS[t]


def _ctypes_class(t):
    import ctypes as C
    if t is None:
        return "void"
    if isinstance(t, type) and issubclass(t, C.Structure):
        return t.__name__
    if t in (C.c_void_p, C.c_char_p) or isinstance(t, type) and issubclass(t, C._Pointer):
        return "ptr"
    assert issubclass(t, C._SimpleCData), t
    return {"f": "f4", "d": "f8"}.get(t._type_) or ("i" if t._type_ in "bhilq" else "u") + str(C.sizeof(t))


def test_tables_state_the_headers_prototypes():
    """every function of include/agmv_hip.h is in abi.HIP and the reverse; every entry of abi.HIP and abi.AGMV has the header's
    return class and parameter classes"""
    from libagmv_amd import abi
    hip, agmv = _prototypes("agmv_hip.h"), _prototypes("agmv.h")
    assert set(hip) == set(abi.HIP)
    assert len(hip) == 86
    assert not set(abi.AGMV) - set(agmv), sorted(set(abi.AGMV) - set(agmv))
    for table, protos in ((abi.HIP, hip), (abi.AGMV, agmv)):
        for name, (restype, argtypes) in table.items():
            ret, params = protos[name]
            assert _ctypes_class(restype) == _c_class(ret, True), "%s returns %s" % (name, ret)
            assert [_ctypes_class(a) for a in argtypes] == [_c_class(p) for p in params], "%s(%s)" % (name, ", ".join(params))


def test_table_holds_every_host_function_python_calls():
    """abi.AGMV has every function of include/agmv.h that a Python file of this repository names"""
    from libagmv_amd import abi
    text = ""
    for top in ("libagmv_amd", "tests", "tools", "bench.py", "__graft_entry__.py"):
        for dp, _, fns in os.walk(os.path.join(ROOT, top)) if os.path.isdir(os.path.join(ROOT, top)) else [(ROOT, [], [top])]:
            text += "".join(open(os.path.join(dp, fn)).read() for fn in fns if fn.endswith(".py") and fn not in ("oracles.py", "abi.py"))
    called = {n for n in _prototypes("agmv.h") if re.search(r"\b%s\b" % n, text)}
    assert called <= set(abi.AGMV), sorted(called - set(abi.AGMV))


def test_structures_have_the_headers_layout(tmp_path):
    """sizeof and every offsetof of the three structures, from gcc against include/agmv.h"""
    import ctypes as C
    import subprocess
    from libagmv_amd import abi
    structs = (abi.AGMV_INFO, abi.AGMV_FRAME_QUALITY, abi.AGMV_ENTRY)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"agmv.h\"\nint main(void) {\n" + "".join(
        '    printf("%s %%zu%s\\n", sizeof(%s)%s);\n' % (s.__name__, " %zu" * len(s._fields_), s.__name__,
                                                     "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
        for s in structs) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines == ["%s %d%s" % (s.__name__, C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) for s in structs]
    assert C.sizeof(abi.AGMV_FRAME_QUALITY) == 96


def test_importing_the_table_loads_nothing():
    import subprocess
    import sys
    code = ("import sys; import libagmv_amd.abi; import libagmv_amd.hip as H, libagmv_amd.seq as S; "
            "assert 'torch' not in sys.modules; assert H._libs == {} and S._lib is None; "
            "assert 'libagmv' not in open('/proc/self/maps').read()")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_bind_sets_every_signature():
    import libagmv_amd.hip as H
    from libagmv_amd import abi, build
    build.build()
    L = H.load_library()
    for name, (restype, argtypes) in abi.HIP.items():
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes) and f.restype is restype, name
    with pytest.raises(AttributeError, match="agmv_hip_no_such_call"):
        abi.bind(L, {"agmv_hip_no_such_call": (None, ())})
    assert abi.bind(L, {"agmv_hip_no_such_call": (None, ())}, missing_ok=True) is L


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import libagmv_amd
    with pytest.raises(libagmv_amd.HipUnavailable) as ei:
        libagmv_amd.AgmvHip(0)
    assert "no CPU fallback" in str(ei.value)


def test_product_never_touches_the_oracle():
    """only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use oracle/."""
    for dp, _, fns in os.walk(os.path.join(ROOT, "libagmv_amd")):
        for fn in fns:
            if fn.endswith((".py", ".c", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                assert "oracle" not in txt.lower().replace("no cpu fallback", ""), os.path.join(dp, fn)


def test_example_program_builds_against_the_drop_in_headers(tmp_path):
    """the reference's README flow compiles and links unchanged against include/agmv.h + libagmv.so"""
    import subprocess
    from libagmv_amd import build
    build.build()
    exe = str(tmp_path / "agmv_example")
    subprocess.run(["gcc", os.path.join(ROOT, "examples", "encode_decode.c"), "-I" + os.path.join(ROOT, "include"),
                    "-L" + os.path.join(ROOT, "libagmv_amd"), "-lagmv", "-lagmv_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "libagmv_amd"), "-o", exe], check=True)
    assert os.path.exists(exe)


def test_build_refuses_kernels_that_spill():
    """the device build is refused when hipcc reports scratch use for any kernel (libagmv_amd/build.py): the parser of its remarks"""
    from libagmv_amd import build as B
    sample = ("a.hip:185:1: remark: Function Name: k_one [-Rpass-analysis=kernel-resource-usage]\n"
              "a.hip:185:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
              "a.hip:209:1: remark: Function Name: k_two [-Rpass-analysis=kernel-resource-usage]\n"
              "a.hip:209:1: remark:     ScratchSize [bytes/lane]: 12 [-Rpass-analysis=kernel-resource-usage]\n")
    assert B._scratch_users(sample) == ["k_two (12 bytes/lane)"]
    assert B._scratch_users("") == []
