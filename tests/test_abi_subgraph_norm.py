"""include/relgnn_subgraph_norm.h: the argument checks that run on the host in front of a launch (no compute calls).  The header is
held against the binding and the library by tests/test_abi.py."""


def test_library_exports_and_checks_its_arguments_on_the_host():
    from tf_gnn_samples_amd import _build, _lib
    if not _lib.LIB_PATH.exists():
        _build.build_library()
    lib = _lib.load_library()
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
