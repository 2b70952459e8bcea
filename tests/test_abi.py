"""The C-ABI library loads and exports every symbol include/relgnn.h declares (no compute calls)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def declared_functions():
    text = (ROOT / "include" / "relgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(relgnn_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_functions():
    names = declared_functions()
    assert "relgnn_seg_reduce_fwd" in names and len(names) >= 10


def test_library_exports_every_declared_symbol():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, "declared in relgnn.h but not exported: %s" % missing


def test_python_binding_covers_header():
    from tf_gnn_samples_amd import _lib
    assert sorted(_lib.exported_signatures()) == declared_functions()


_C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def _c_type(text, returned=False):
    """The ctypes type of one C parameter (or return) type as the header writes it: any pointer is c_void_p (a returned
    const char* c_char_p), the scalar types map to their ctypes."""
    if "*" in text:
        return ctypes.c_char_p if returned and re.fullmatch(r"const\s+char\s*\*", text.strip()) else ctypes.c_void_p
    words = [w for w in text.split() if w != "const"]
    return _C_TYPES[words[0]]            # (a parameter's name, when it has one, is the second word)


def declared_signatures():
    """name -> (restype, [argtypes]) for every function include/relgnn.h declares, read from the text with its comments stripped."""
    text = (ROOT / "include" / "relgnn.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\**)\s*\b(relgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = " ".join(params.split())
        args = [] if params in ("", "void") else [_c_type(a) for a in params.split(",")]
        out[name] = (_c_type(ret, returned=True), args)
    return out


def test_python_binding_types_every_argument_as_the_header_declares_it():
    """restype and argtypes of _lib's table against the header, element for element: a c_int32 where the header says int64_t is a
    silently wrong value for any argument passed on the stack, and most entries have more than six."""
    from tf_gnn_samples_amd import _lib
    declared, bound = declared_signatures(), _lib.exported_signatures()
    assert sorted(declared) == declared_functions() and len(declared) == 126
    assert sorted(bound) == sorted(declared)
    wrong = {n: (bound[n], declared[n]) for n in declared if (bound[n][0], list(bound[n][1])) != declared[n]}
    assert not wrong, "bound (restype, argtypes) vs the header's: %s" % wrong


def test_loader_types_every_symbol_and_reports_version():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    lib = _lib.load_library()
    assert lib.relgnn_abi_version() == 1
    assert _lib.status_string(0) == "ok"
    assert "argument" in _lib.status_string(1)


def test_product_path_refuses_cpu_tensors():
    """No CPU fallback: a CPU tensor must fail loudly, not silently compute."""
    import torch
    from tf_gnn_samples_amd import _lib
    with pytest.raises(_lib.RelGnnLibraryError):
        _lib.ptr(torch.zeros(4))


def test_package_does_not_import_oracle():
    import subprocess, sys
    code = ("import sys; import tf_gnn_samples_amd, tf_gnn_samples_amd.gnns, tf_gnn_samples_amd.models, "
            "tf_gnn_samples_amd.tasks, tf_gnn_samples_amd.ops; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(ROOT))
    for py in (ROOT / "tf_gnn_samples_amd").rglob("*.py"):
        assert not re.search(r"^\s*(from|import)\s+oracle\b", py.read_text(), flags=re.M), py
