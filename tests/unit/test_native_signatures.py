"""The ctypes argtype lists in ops/native.py against the PK_EXPORT declarations in csrc/kernels:
ctypes checks nothing at the call, so a list edited on one side only passes garbage silently."""
import ctypes
import glob
import os
import re

from polykey_service_amd.ops import native

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _kind(param: str):
    """One C parameter declaration -> the ctypes type that carries it."""
    param = param.strip()
    if "*" in param or re.match(r"hipStream_t\b", param):
        return ctypes.c_void_p
    ctype = " ".join(re.sub(r"\bconst\b", "", param).split()[:-1])  # without the parameter's name
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_int64, "float": ctypes.c_float}[ctype]


def _exports() -> dict:
    """name -> (return type, [ctypes kind per parameter]) of every PK_EXPORT in csrc/kernels/*.hip."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "csrc", "kernels", "*.hip"))):
        text = re.sub(r"//[^\n]*", "", open(path).read())
        for ret, name, params in re.findall(r"PK_EXPORT\s+(\w+)\s+(\w+)\s*\(([^)]*)\)", text):
            assert name not in out, name
            params = params.strip()
            out[name] = (ret, [] if params in ("", "void") else [_kind(p) for p in params.split(",")])
    return out


def test_signatures_match_the_c_declarations():
    exports = _exports()
    assert len(exports) >= len(native.SIGNATURES)
    for name, argtypes in native.SIGNATURES.items():
        assert name in exports, f"{name}: no PK_EXPORT declaration"
        ret, kinds = exports[name]
        assert ret == "int", (name, ret)
        assert len(kinds) == len(argtypes), (name, len(kinds), len(argtypes))
        for i, (want, got) in enumerate(zip(kinds, argtypes)):
            assert want is got, f"{name}: argument {i} is {want.__name__} in C, {got.__name__} in SIGNATURES"


def test_no_fp8_attention_or_rope_export_remains():
    names = set(_exports()) | set(native.SIGNATURES)
    assert not [n for n in names if n.endswith("_fp8")], names
    assert "pk_decode_num_parts" not in names
    for n in ("pk_rope_and_cache", "pk_paged_decode", "pk_paged_decode_qkv", "pk_paged_prefill"):
        assert native.SIGNATURES[n][-4:] == [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p], n
