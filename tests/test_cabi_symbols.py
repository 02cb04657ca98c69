"""The C-ABI library loads without a GPU and exports every symbol include/rgcn_hip.h declares; the binding declares every entry
point's argument and return types from that header, so misuse raises, and every call site passes as many arguments as the header
says; the package fails loudly (no fallback) when the library or the header is absent or unreadable."""
import ast
import ctypes
import glob
import os
import re

import pytest

from conftest import ROOT
from torch_rgcn import _native


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rgcn_hip.h")).read()
    return sorted(set(re.findall(r"RGCN_API[^;(]*?\b(rgcn_\w+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    names = declared_symbols()
    for must in ("rgcn_spmm_f32", "rgcn_wgrad_f32", "rgcn_featureless_fwd_f32", "rgcn_featureless_wgrad_f32",
                 "rgcn_edge_norm_host", "rgcn_plan_fill_host", "rgcn_distmult_fwd_f32", "rgcn_last_error"):
        assert must in names
    assert len(names) >= 15


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_native._LIB_PATH)
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing
    assert b"gfx950" in ctypes.cast(lib.rgcn_version, ctypes.CFUNCTYPE(ctypes.c_char_p))()


C_TYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "const char *": ctypes.c_char_p}


def declared_prototypes():
    """{name: (return type, [parameter declarations])} read from the header, independently of the binder"""
    text = open(os.path.join(ROOT, "include", "rgcn_hip.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^RGCN_API\s+([\w\s*]+?)\s*\b(rgcn_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def test_every_prototype_binds():
    L = _native.lib()
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols() and len(protos) == _native._bind(L, _native._HEADER_PATH)
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is C_TYPES[ret], (name, ret, fn.restype)
        assert len(fn.argtypes) == len(params), (name, params, fn.argtypes)
        for decl, ct in zip(params, fn.argtypes):
            want = ctypes.c_char_p if decl.startswith("const char *") else ctypes.c_void_p if "*" in decl else C_TYPES[decl.split()[0]]
            assert ct is want, (name, decl, ct)
    assert L.rgcn_colsum_scratch_floats.argtypes == [ctypes.c_int64, ctypes.c_int32] and L.rgcn_colsum_scratch_floats.restype is ctypes.c_int64
    assert L.rgcn_fbasis_tile_supported.argtypes == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]


def test_misuse_raises():
    block_ok, tile_ok = _native.lib().rgcn_block_supported, _native.lib().rgcn_fbasis_tile_supported
    assert block_ok(8, 8) and not block_ok(9, 9)
    with pytest.raises(TypeError):
        block_ok(8)
    with pytest.raises(ctypes.ArgumentError):
        block_ok(8, 8.0)
    with pytest.raises(ctypes.ArgumentError):
        block_ok(8, None)
    with pytest.raises(ctypes.ArgumentError):
        tile_ok(13, 8, 16, ctypes.c_int32(40000))
    # the 64-bit node count arrives whole: fewer nodes than one 16-node tile are refused, and 8 is the low half of 2^32 + 8
    assert tile_ok(13, 8, 16, 40000) and not tile_ok(13, 8, 16, 8) and tile_ok(13, 8, 16, 2 ** 32 + 8)


def test_call_sites_pass_the_declared_number_of_arguments():
    """ctypes lets surplus arguments of a cdecl function through, so the arity of every call site is compared with the header here"""
    protos = declared_prototypes()
    native = os.path.join(ROOT, "torch-rgcn_amd", "torch_rgcn", "_native.py")
    files = [native] + sorted(glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)) + sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")))
    seen, bad = set(), []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("rgcn_")):
                continue
            name, where = node.func.attr, f"{os.path.relpath(path, ROOT)}:{node.lineno}"
            if name not in protos:
                if path == native:
                    bad.append(f"{where}: {name} is not declared in the header")
                continue
            seen.add(name)
            if node.keywords or any(isinstance(a, ast.Starred) for a in node.args):
                bad.append(f"{where}: {name} called with keywords or *args")
            elif len(node.args) != len(protos[name][1]):
                bad.append(f"{where}: {name} takes {len(protos[name][1])} arguments, {len(node.args)} given")
    assert not bad, "\n".join(bad)
    assert len(seen) >= 100, len(seen)       # the walk does find the call sites


def test_a_header_with_an_unknown_type_is_loud(tmp_path):
    L = ctypes.CDLL(_native._LIB_PATH)
    text = open(_native._HEADER_PATH).read()
    for good, broken in (("RGCN_API int rgcn_block_supported(int32_t bi, int32_t bo);", "RGCN_API int rgcn_block_supported(int32_t bi, float bo);"),
                         ("RGCN_API int rgcn_block_supported(int32_t bi, int32_t bo);", "RGCN_API double rgcn_block_supported(int32_t bi, int32_t bo);"),
                         ("RGCN_API int rgcn_block_supported(int32_t bi, int32_t bo);", "RGCN_API int rgcn_block_supported(int32_t bi, int (*cb)(int));"),
                         ("RGCN_API int rgcn_block_supported(", "RGCN_API int rgcn_no_such_entry_point(")):
        assert text.count(good) == 1
        bad = tmp_path / "rgcn_hip.h"
        bad.write_text(text.replace(good, broken))
        with pytest.raises(_native.NativeLibraryError):
            _native._bind(L, str(bad))
    with pytest.raises(_native.NativeLibraryError):
        _native._bind(L, str(tmp_path / "absent.h"))
    assert _native._bind(L, _native._HEADER_PATH) == len(declared_symbols())


def test_missing_library_is_loud(monkeypatch):
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "_LIB_PATH", "/nonexistent/librgcn_hip.so")
    with pytest.raises(_native.NativeLibraryError):
        _native.lib()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "torch-rgcn_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("no oracle", ""), os.path.join(dirpath, f)


def test_block_tile_backward_takes_with_diag4_what_it_takes_without():
    """functional._backward_route asks _bwd_blk_plan once, with the caller's diag4: a tall plan the kernel takes for the dense dW it takes
    for dW's diagonal 4 x 4 blocks too (they need less of the LDS), for every relation count"""
    lib = ctypes.CDLL(_native._LIB_PATH)
    for R in list(range(1, 700)) + [4095, 65534, 65535]:
        dense, diag = lib.rgcn_bwd_blk_max_rows(R, 0), lib.rgcn_bwd_blk_max_rows(R, _native.F_DIAG4)
        assert diag >= dense, (R, dense, diag)
        assert not lib.rgcn_bwd_blk_supported(dense, R, 0) or lib.rgcn_bwd_blk_supported(dense, R, _native.F_DIAG4), R
