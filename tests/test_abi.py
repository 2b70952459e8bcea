"""The C ABI, header by header: every include/relgnn*.h against tf_gnn_samples_amd/_lib.py's table for it, the library's exported
symbols and what the loader sets (no compute calls).  The headers are read by tests/abi_reference.py."""
import ctypes
import re
from pathlib import Path

import pytest

from abi_reference import declared_names, declared_signatures, stripped

ROOT = Path(__file__).resolve().parent.parent
HEADERS = sorted(p.name for p in (ROOT / "include").iterdir())

_i32, _f32, _ptr = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
# what is pinned per header: the number of entry points; `names`: all of them; `has`: some of them; `nargs`: argument counts;
# `signature`: whole signatures; `source`: the kernel file the build must compile for it
PINNED = {
    "relgnn.h": dict(count=126, has=["relgnn_seg_reduce_fwd"]),
    "relgnn_dropout.h": dict(count=4, names=["relgnn_dropout_bwd", "relgnn_dropout_fwd", "relgnn_dropout_residual_bwd",
                                             "relgnn_dropout_residual_fwd"], source="dropout.hip"),
    "relgnn_predict.h": dict(count=3, names=["relgnn_predict_candidates_f32", "relgnn_predict_sigmoid_f32", "relgnn_predict_softmax_f32"]),
    "relgnn_parallel.h": dict(count=1, names=["relgnn_mt_pack_scaled_f32"], source="parallel.hip",
                              signature={"relgnn_mt_pack_scaled_f32": (ctypes.c_int, [_ptr, _ptr, _i32, _f32, _ptr, _ptr])}),
    "relgnn_sparse_features.h": dict(count=4, names=["relgnn_csr_project_f32", "relgnn_csr_project_slab", "relgnn_csr_project_split_above",
                                                     "relgnn_csr_project_supported"]),
    "relgnn_sampling.h": dict(count=11, has=["relgnn_neighbour_sample_supported", "relgnn_neighbour_sample_take"]),
    "relgnn_layered_sampling.h": dict(count=2, names=["relgnn_neighbour_sample_degrees_by_hop", "relgnn_neighbour_sample_relabel_by_hop"]),
    "relgnn_sparse_subset.h": dict(count=9, has=["relgnn_split_plan_count", "relgnn_split_plan_fill", "relgnn_sparse_subset_count"]),
    "relgnn_sparse_update.h": dict(count=3, names=["relgnn_rows_adam_catch_up", "relgnn_rows_adam_step", "relgnn_rows_adam_supported"],
                                   nargs={"relgnn_rows_adam_catch_up": 15, "relgnn_rows_adam_step": 20}),
    "relgnn_sparse_gradient.h": dict(count=6, names=["relgnn_named_rows_count", "relgnn_named_rows_fill", "relgnn_named_rows_workspace_bytes",
                                                     "relgnn_rows_adam_step_compact", "relgnn_rows_l2norm",
                                                     "relgnn_rows_l2norm_workspace_bytes"],
                                     nargs={"relgnn_rows_adam_step_compact": 21, "relgnn_rows_l2norm": 10}),
    "relgnn_subgraph.h": dict(count=8, names=["relgnn_subgraph_clear", "relgnn_subgraph_induced_count", "relgnn_subgraph_induced_emit",
                                              "relgnn_subgraph_max_walk_length", "relgnn_subgraph_number", "relgnn_subgraph_supported",
                                              "relgnn_subgraph_walk", "relgnn_subgraph_workspace_bytes"], source="subgraph_sample.hip"),
    "relgnn_subgraph_norm.h": dict(count=5, names=["relgnn_softmax_ce_weighted_bwd", "relgnn_softmax_ce_weighted_stats",
                                                   "relgnn_softmax_ce_weighted_stats_workspace_bytes",
                                                   "relgnn_subgraph_induced_emit_weighted", "relgnn_subgraph_visit_count"]),
}
TOTAL = 182


def _library_path():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    return str(_lib.LIB_PATH)


def test_header_declares_functions():
    names = declared_names("relgnn.h")
    assert "relgnn_seg_reduce_fwd" in names and len(names) >= 10


def test_binding_build_and_include_list_the_same_headers():
    """One table per header, every header a build dependency (is_stale() watches it), and every header pinned here."""
    from tf_gnn_samples_amd import _build, _lib
    assert set(_lib.ABI) == {h.name for h in _build.HEADERS} == set(HEADERS) == set(PINNED)
    assert len(_build.HEADERS) == len(HEADERS) == 12 and all(h.parent == ROOT / "include" for h in _build.HEADERS)
    assert all(isinstance(_lib.signatures(h), dict) and _lib.signatures(h) is not _lib.ABI[h] for h in HEADERS)       # copies
    sources = {p.name for p in _build._sources()}
    assert not [pin["source"] for pin in PINNED.values() if "source" in pin and pin["source"] not in sources]


@pytest.mark.parametrize("header", HEADERS)
def test_python_binding_covers_header(header):
    """The loose scan, the parser and the table name the same functions, and those are the pinned ones."""
    from tf_gnn_samples_amd import _lib
    pin, names = PINNED[header], declared_names(header)
    assert names == sorted(declared_signatures(header)) == sorted(_lib.signatures(header))
    assert len(names) == pin["count"] and names == pin.get("names", names) and not [n for n in pin.get("has", []) if n not in names]
    if header == "relgnn.h":
        assert not [n for n in names if "dropout" in n]


@pytest.mark.parametrize("header", HEADERS)
def test_python_binding_types_every_argument_as_the_header_declares_it(header):
    """restype and argtypes of _lib's table against the header, element for element: a c_int32 where the header says int64_t is a
    silently wrong value for any argument passed on the stack, and most entries have more than six."""
    from tf_gnn_samples_amd import _lib
    declared, bound = declared_signatures(header), _lib.signatures(header)
    assert sorted(bound) == sorted(declared)
    wrong = {n: (bound[n], declared[n]) for n in declared if (bound[n][0], list(bound[n][1])) != declared[n]}
    assert not wrong, "bound (restype, argtypes) vs the header's: %s" % wrong
    for name, nargs in PINNED[header].get("nargs", {}).items():
        assert len(declared[name][1]) == nargs, name
    for name, signature in PINNED[header].get("signature", {}).items():
        assert declared[name] == signature, name


@pytest.mark.parametrize("header", HEADERS)
def test_library_exports_every_declared_symbol(header):
    raw = ctypes.CDLL(_library_path())
    missing = [n for n in declared_names(header) if not hasattr(raw, n)]
    assert not missing, "declared in %s but not exported: %s" % (header, missing)


@pytest.mark.parametrize("header", HEADERS)
def test_loader_types_every_symbol(header):
    """What load_library() left on the functions themselves: one it skipped would keep ctypes' int / untyped convention, which
    truncates every int64_t, size_t and float argument without a word."""
    from tf_gnn_samples_amd import _lib
    _library_path()
    lib = _lib.load_library()
    for name, (restype, argtypes) in _lib.signatures(header).items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_no_name_is_bound_by_two_headers(monkeypatch):
    from tf_gnn_samples_amd import _lib
    names = [n for h in HEADERS for n in _lib.signatures(h)]
    assert len(names) == len(set(names)) == TOTAL == sum(pin["count"] for pin in PINNED.values())
    union = _lib.signatures()
    assert sorted(union) == sorted(names) and all(union[n] == _lib.signatures(h)[n] for h in HEADERS for n in _lib.signatures(h))
    # ... and the binding itself refuses a second binding, where the later table used to win
    monkeypatch.setitem(_lib.ABI, "relgnn_parallel.h", dict(_lib.ABI["relgnn_parallel.h"], relgnn_dropout_fwd=(ctypes.c_int, [])))
    with pytest.raises(_lib.RelGnnLibraryError, match="relgnn_dropout_fwd is bound by both relgnn_dropout.h and relgnn_parallel.h"):
        _lib.signatures()


def test_constants_mirror_the_header():
    """Every `#define RELGNN_<NAME> <integer>` of relgnn.h that _lib restates by hand has the header's value."""
    from tf_gnn_samples_amd import _lib
    defined = {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+RELGNN_(\w+)\s+(\d+)u?\b", stripped("relgnn.h"), flags=re.M)}
    mirrored = {n: v for n, v in defined.items() if hasattr(_lib, n)}
    wrong = {n: (getattr(_lib, n), v) for n, v in mirrored.items() if getattr(_lib, n) != v}
    assert not wrong, "_lib's value vs the header's: %s" % wrong
    assert set(mirrored) >= {"OK", "EINVAL", "ENOSPC", "EHIP", "EUNSUPPORTED", "ERRFLAG_INDEX_OUT_OF_RANGE", "ERRFLAG_NOT_SORTED",
                             "AGG_SUM", "AGG_MEAN", "AGG_SQRT_N", "AGG_MAX", "MT_MAX", "ACT_LINEAR", "ACT_TANH", "ACT_RELU",
                             "ACT_LEAKY_RELU", "ACT_ELU", "ACT_SELU", "ACT_GELU"}


def test_loader_types_every_symbol_and_reports_version():
    from tf_gnn_samples_amd import _lib
    _library_path()
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
