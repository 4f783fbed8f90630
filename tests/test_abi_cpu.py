"""CPU: the C-ABI library builds for gfx950, loads without a GPU and exports every symbol that
include/gemnet_hip.h declares (no compute calls here)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gemnet_pytorch_amd import _abi, _lib


def declared_symbols():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_header_declares_the_bound_functions():
    syms = declared_symbols()
    assert set(_lib.SIGNATURES) <= set(syms)
    assert {"gn_abi_version", "gn_error_string"} <= set(syms)


def test_library_exports_every_declared_symbol(lib):
    for s in declared_symbols():
        assert hasattr(lib, s), f"{s} declared in include/gemnet_hip.h but not exported"
    assert lib.gn_abi_version() == 16


def test_gemm_args_struct_matches_header():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct \{(.*?)\} gn_gemm_args;", text, flags=re.S).group(1)
    names = re.findall(r"[\*\s]([A-Za-z_][A-Za-z0-9_]*)\s*[;,]", body)
    assert names == [n for n, _ in _lib.GemmArgs._fields_]


def test_derived_layouts_match_the_compiler(tmp_path):
    """sizeof / offsetof of the six structs as g++ lays them out == the ctypes classes read from the header == the numpy
    dtypes of the three device-table rows."""
    structs = _lib.ABI.structs
    assert sorted(structs) == ["gn_chain_args", "gn_chain_op", "gn_gemm_args", "gn_pack_job", "gn_tn_problem", "gn_tn_target"]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "gemnet_hip.h"', 'int main() {']
    for s, cls in structs.items():
        lines.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s} {n} %zu\\n", offsetof({s}, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    want = {}
    for line in subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n"):
        if line:
            s, field, value = line.split()
            want.setdefault(s, {})[field] = int(value)
    assert {s: w["sizeof"] for s, w in want.items()} == {"gn_gemm_args": 192, "gn_chain_op": 248, "gn_chain_args": 4968,
                                                        "gn_pack_job": 40, "gn_tn_problem": 64, "gn_tn_target": 40}
    for s, cls in structs.items():
        got = {n: getattr(cls, n).offset for n, _ in cls._fields_}
        got["sizeof"] = ctypes.sizeof(cls)
        assert got == want[s], s
    for s in ("gn_pack_job", "gn_tn_problem", "gn_tn_target"):
        dt = np.dtype(structs[s])
        got = {n: dt.fields[n][1] for n in dt.names}
        got["sizeof"] = dt.itemsize
        assert got == want[s], s
        for n, ct in structs[s]._fields_:      # addresses as unsigned 64-bit integers, the values in their C types
            assert dt.fields[n][0] == np.dtype(np.uint64 if ct is ctypes.c_void_p else ct), (s, n)


def test_pinned_signatures():
    """One hand-written signature per scalar kind (int, int64_t, float, double, struct pointer, values only, no parameters,
    int64_t and const char* returns) against what the header gives."""
    vp, i, i64, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    pinned = {
        "gn_index_gpu_stage1": (i, [vp, i, vp, vp, i, i, i, i64, d, d, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gn_force_loss_f32": (i, [vp, vp, i64, vp, vp, i64, vp, f, f, vp, vp, vp, vp, vp]),
        "gn_gemm_tn_splitk": (i, [i, i, i]),
        "gn_gemm_f32": (i, [ctypes.POINTER(_lib.GemmArgs), vp]),
        "gn_pack_weight_split_bytes": (i64, [i, i]),
        "gn_error_string": (ctypes.c_char_p, [i]),
        "gn_abi_version": (i, []),
    }
    for name, (restype, argtypes) in pinned.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert _lib.ABI.funcs[name][0] is restype, name


@pytest.mark.parametrize("text", [
    "int gn_x(unsigned long n, void* stream);",
    "unsigned long gn_x(int n);",
    "typedef struct { int n; size_t bytes; } gn_y;\nint gn_x(const gn_y* y, void* stream);",
])
def test_reader_refuses_unknown_types(text):
    with pytest.raises(TypeError, match="gn_[xy]"):
        _abi.parse(text)


def test_every_declared_function_is_bound(lib):
    assert set(_lib.SIGNATURES) == set(declared_symbols()) == set(_lib.ABI.funcs)
    for name, (restype, _) in _lib.ABI.funcs.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == _lib.SIGNATURES[name], name
        assert fn.restype is restype, name
