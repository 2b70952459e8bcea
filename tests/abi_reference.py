"""The one reader of the C ABI's headers (include/relgnn*.h) for the tests: what a header declares, as names and as ctypes
signatures.  A helper, not a test: tests/test_abi.py holds every header to tf_gnn_samples_amd/_lib.py's table, to the library's
exports and to what the loader sets with it."""
import ctypes
import re
from pathlib import Path

INCLUDE = Path(__file__).resolve().parent.parent / "include"

_C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def stripped(header):
    """The text of include/<header> without its comments."""
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def declared_names(header):
    """Every relgnn_x( the header writes outside a comment, sorted: the loose scan the parser below is held against."""
    return sorted(set(re.findall(r"\b(relgnn_[a-z0-9_]+)\s*\(", stripped(header))))


def _c_type(text, returned=False):
    """The ctypes type of one C parameter (or return) type as the headers write it: any pointer is c_void_p (a returned
    const char* c_char_p), the scalar types map to their ctypes."""
    if "*" in text:
        return ctypes.c_char_p if returned and re.fullmatch(r"const\s+char\s*\*", text.strip()) else ctypes.c_void_p
    return _C_TYPES[[w for w in text.split() if w != "const"][0]]        # (a parameter's name, when it has one, is the second word)


def declared_signatures(header):
    """name -> (restype, [argtypes]) of every function the header declares, in the header's order."""
    out = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\**)\s*\b(relgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", stripped(header),
                                        flags=re.M):
        params = " ".join(params.split())
        out[name] = (_c_type(ret, returned=True), [] if params in ("", "void") else [_c_type(a) for a in params.split(",")])
    return out
