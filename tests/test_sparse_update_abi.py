"""include/relgnn_sparse_update.h <-> exported symbols <-> _lib.sparse_update_signatures(), as tests/test_abi.py holds relgnn.h and the
other side headers are held; the argument checks that need no GPU (every refusal returns before anything is launched)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "relgnn_sparse_update.h"

C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def declared_signatures():
    c_type = lambda text: ctypes.c_void_p if "*" in text else C_TYPES[[w for w in text.split() if w != "const"][0]]
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S))
    declared = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\**)\s*\b(relgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = " ".join(params.split())
        declared[name] = (c_type(ret), [] if params == "void" else [c_type(a) for a in params.split(",")])
    return declared


def test_header_binding_and_library_agree():
    from tf_gnn_samples_amd import _build, _lib
    assert HEADER in _build.HEADERS
    declared, bound = declared_signatures(), _lib.sparse_update_signatures()
    assert sorted(declared) == sorted(bound) == ["relgnn_rows_adam_catch_up", "relgnn_rows_adam_step", "relgnn_rows_adam_supported"]
    wrong = {n: (bound[n], declared[n]) for n in declared if (bound[n][0], list(bound[n][1])) != declared[n]}
    assert not wrong, "bound (restype, argtypes) vs the header's: %s" % wrong
    assert len(declared["relgnn_rows_adam_catch_up"][1]) == 15 and len(declared["relgnn_rows_adam_step"][1]) == 20
    others = [_lib.exported_signatures(), _lib.dropout_signatures(), _lib.predict_signatures(), _lib.parallel_signatures(),
              _lib.sparse_features_signatures(), _lib.sampling_signatures(), _lib.sparse_subset_signatures()]
    assert all(not set(o) & set(bound) for o in others)
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    assert not [n for n in declared if not hasattr(raw, n)]


def test_supported_widths_and_refusals_before_any_launch():
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    taken = [n for n in range(0, 1100) if lib.relgnn_rows_adam_supported(n)]
    assert taken == list(range(4, 1025, 4)) and not lib.relgnn_rows_adam_supported(-4)
    assert all(bool(lib.relgnn_rows_adam_supported(n)) == bool(lib.relgnn_csr_project_supported(n)) for n in range(0, 1100))    # the projection's own rule
    fake = 4096                                            # a 16-byte aligned non-null "pointer": every call below returns before it is read
    catch_up = lambda F=8, p=fake, ld=8, n=8, base=0, t=2: lib.relgnn_rows_adam_catch_up(None, F, p, fake, fake, ld, n, fake, fake, base, t, 0.9,
                                                                                       0.999, 1e-8, None)
    assert catch_up(F=0) == _lib.OK and catch_up(base=2, t=2) == _lib.OK                     # nothing to do: no launch
    assert catch_up(n=6) == _lib.EUNSUPPORTED and catch_up(n=1028) == _lib.EUNSUPPORTED
    for bad in (dict(F=-1), dict(F=2 ** 31 - 1), dict(base=-1), dict(base=3, t=2), dict(p=None), dict(p=fake + 4), dict(ld=4), dict(ld=9, n=8)):
        assert catch_up(**bad) == _lib.EINVAL, bad
    step = lambda F=8, p=fake, g=fake, ld_g=8, ld=8, n=8, table=fake, base=0, t=1, norm=fake, clip=1.0: lib.relgnn_rows_adam_step(
        None, F, p, g, ld_g, fake, fake, ld, n, fake, table, base, t, norm, clip, 1e-3, 0.9, 0.999, 1e-8, None)
    assert step(n=2) == _lib.EUNSUPPORTED
    for bad in (dict(F=-1), dict(base=1, t=1), dict(base=-1, t=0), dict(table=None), dict(norm=None), dict(g=None), dict(g=fake + 8),
                dict(ld_g=4), dict(ld=10), dict(p=None)):
        assert step(**bad) == _lib.EINVAL, bad
