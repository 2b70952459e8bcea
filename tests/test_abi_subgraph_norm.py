"""include/relgnn_subgraph_norm.h <-> the library's exported symbols <-> _lib.subgraph_norm_signatures(); the argument checks that run
on the host in front of a launch (no compute calls)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "relgnn_subgraph_norm.h"
NAMES = ["relgnn_softmax_ce_weighted_bwd", "relgnn_softmax_ce_weighted_stats", "relgnn_softmax_ce_weighted_stats_workspace_bytes",
         "relgnn_subgraph_induced_emit_weighted", "relgnn_subgraph_visit_count"]
_C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def declared_signatures():
    c_type = lambda text: ctypes.c_void_p if "*" in text else _C_TYPES[[w for w in text.split() if w != "const"][0]]
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S))
    declared = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\**)\s*\b(relgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = " ".join(params.split())
        declared[name] = (c_type(ret), [] if params == "void" else [c_type(a) for a in params.split(",")])
    assert sorted(declared) == sorted(set(re.findall(r"\b(relgnn_[a-z0-9_]+)\s*\(", text)))
    return declared


def test_header_is_built_and_declares_the_five_entry_points():
    from tf_gnn_samples_amd import _build
    assert HEADER in _build.HEADERS
    assert sorted(declared_signatures()) == NAMES


def test_python_binding_types_every_argument_as_the_header_declares_it():
    from tf_gnn_samples_amd import _lib
    declared, bound = declared_signatures(), _lib.subgraph_norm_signatures()
    assert sorted(bound) == sorted(declared)
    wrong = {n: (bound[n], declared[n]) for n in declared if (bound[n][0], list(bound[n][1])) != declared[n]}
    assert not wrong, "bound (restype, argtypes) vs the header's: %s" % wrong
    others = set(_lib.exported_signatures()) | set(_lib.subgraph_signatures()) | set(_lib.sampling_signatures())
    assert not others & set(bound)


def test_library_exports_and_checks_its_arguments_on_the_host():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    assert not [n for n in NAMES if not hasattr(raw, n)]
    lib = _lib.load_library()
    for n, (restype, argtypes) in _lib.subgraph_norm_signatures().items():
        assert getattr(lib, n).restype is restype and list(getattr(lib, n).argtypes) == list(argtypes), n
    assert lib.relgnn_softmax_ce_weighted_stats_workspace_bytes() >= 4 * 8
    # node_bound > V, V * L = 2^31, null pointers
    assert lib.relgnn_subgraph_visit_count(None, None, 300, 3, 10, None, None, 301, None, None, None, None) == _lib.EINVAL
    assert lib.relgnn_subgraph_visit_count(None, None, 1 << 30, 2, 10, None, None, 4, None, None, None, None) == _lib.EUNSUPPORTED
    assert lib.relgnn_subgraph_visit_count(None, None, 300, 3, 1 << 31, None, None, 4, None, None, None, None) == _lib.EUNSUPPORTED
    assert lib.relgnn_subgraph_visit_count(None, None, 300, 3, 10, None, None, 4, None, None, None, None) == _lib.EINVAL
    # n > node_bound; a clip that is not positive; an empty set is no launch
    emit = lib.relgnn_subgraph_induced_emit_weighted
    assert emit(None, None, 300, 3, 10, None, 5, 4, None, None, None, None, 2.0, 0, None, None, None, None) == _lib.EINVAL
    assert emit(None, None, 300, 3, 10, None, 0, 4, None, None, None, None, 0.0, 0, None, None, None, None) == _lib.EINVAL
    assert emit(None, None, 300, 3, 10, None, 0, 4, None, None, None, None, float("nan"), 0, None, None, None, None) == _lib.EINVAL
    assert emit(None, None, 300, 3, 10, None, 0, 4, None, None, None, None, 2.0, 0, None, None, None, None) == _lib.OK
    assert emit(None, None, 300, 3, 10, None, 2, 4, None, None, None, None, 2.0, 0, None, None, None, None) == _lib.EINVAL
    # a zero or NaN denominator, ld < cols, no gradient at all
    stats, bwd = lib.relgnn_softmax_ce_weighted_stats, lib.relgnn_softmax_ce_weighted_bwd
    assert stats(None, 7, None, None, None, 0.0, 0, 7, None, None, 0, None) == _lib.EINVAL
    assert bwd(None, 7, None, None, None, 0.0, 0, 7, None, None, None, 7, None) == _lib.EINVAL
    assert bwd(None, 7, None, None, None, float("nan"), 0, 7, None, None, None, 7, None) == _lib.EINVAL
    assert bwd(None, 6, None, None, None, 1.0, 0, 7, None, None, None, 7, None) == _lib.EINVAL
    assert bwd(None, 7, None, None, None, 1.0, 0, 7, None, None, None, 7, None) == _lib.OK          # no rows: nothing to do
    assert bwd(None, 7, None, None, None, 1.0, 3, 7, None, None, None, 7, None) == _lib.EINVAL
