"""include/relgnn_sparse_gradient.h: the argument checks that need no GPU (every refusal returns before anything is launched).  The
header is held against the binding and the library by tests/test_abi.py."""


def test_refusals_before_any_launch():
    from tf_gnn_samples_amd import _lib
    lib = _lib.load_library()
    fake = 4096                                            # a 16-byte aligned non-null "pointer": every call below returns before it is read
    assert lib.relgnn_rows_l2norm_workspace_bytes() == 32 * 8 and lib.relgnn_named_rows_workspace_bytes(1 << 20) >= 256
    count = lambda rowptr=fake, F=8, slot=fake, out=fake, ws=fake, nbytes=1 << 30: lib.relgnn_named_rows_count(rowptr, F, slot, out, ws,
                                                                                                             nbytes, None)
    for bad in (dict(F=-1), dict(rowptr=None), dict(slot=None), dict(out=None), dict(ws=None)):
        assert count(**bad) == _lib.EINVAL, bad
    assert count(F=2 ** 31 - 1) == _lib.EUNSUPPORTED and count(nbytes=8) == _lib.ENOSPC
    fill = lambda F=8, T=2, words=fake, slabs=fake, num_slabs=1, combos=fake, num_combos=1: lib.relgnn_named_rows_fill(
        fake, F, fake, T, words, fake, slabs, fake, num_slabs, combos, fake, num_combos, None)
    assert fill(T=0) == _lib.OK                            # nothing named: nothing launched
    for bad in (dict(F=-1), dict(T=-1), dict(T=9), dict(words=None), dict(slabs=None), dict(slabs=fake + 4), dict(combos=None),
                dict(num_slabs=-1), dict(num_combos=-1)):
        assert fill(**bad) == _lib.EINVAL, bad
    norm = lambda words=fake, T=2, g=fake, ld=8, n=8, F=8, out=fake, ws=fake, nbytes=256: lib.relgnn_rows_l2norm(words, T, g, ld, n, F, out,
                                                                                                             ws, nbytes, None)
    assert norm(n=6) == _lib.EUNSUPPORTED and norm(n=1028) == _lib.EUNSUPPORTED and norm(nbytes=255) == _lib.ENOSPC
    for bad in (dict(T=-1), dict(T=9), dict(words=None), dict(g=None), dict(ld=4), dict(out=None), dict(ws=None), dict(ws=fake + 4)):
        assert norm(**bad) == _lib.EINVAL, bad
    step = lambda words=fake, T=2, F=8, p=fake, g=fake, ld_g=8, ld=8, n=8, table=fake, base=0, t=1, norm=fake, clip=1.0: \
        lib.relgnn_rows_adam_step_compact(words, T, F, p, g, ld_g, fake, fake, ld, n, fake, table, base, t, norm, clip, 1e-3, 0.9, 0.999,
                                          1e-8, None)
    assert step(n=2) == _lib.EUNSUPPORTED
    for bad in (dict(T=-1), dict(T=9), dict(F=-1), dict(base=1, t=1), dict(base=-1, t=0), dict(table=None), dict(norm=None), dict(g=None),
                dict(g=fake + 8), dict(ld_g=4), dict(ld=10), dict(p=None), dict(words=None)):
        assert step(**bad) == _lib.EINVAL, bad
