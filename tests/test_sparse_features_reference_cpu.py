"""tests/sparse_features_reference.py checked against itself: the kernel's arithmetic restated in float32 lies inside every bound at
the shapes the GPU tests use, and each plausible mistake of a CSR projection lies outside."""
import numpy as np
import pytest

import sparse_features_reference as R

N = 8                                    # columns are independent draws: a property of the first 8 holds for every width


def _inputs():
    csr = R.structure()
    table, dout = R.tables()
    return csr, table[:, :N], dout[:, :N]


def test_the_structure_has_the_row_lengths_the_kernel_branches_on():
    csr = R.structure()
    lengths = np.diff(csr.rowptr)
    assert set(lengths) == set(R.SHORT_LENGTHS) | {l for l, _ in R.LONG_LENGTHS} and 190 <= csr.shape[0] <= 210
    for r in range(csr.shape[0]):
        c = csr.col[csr.rowptr[r]:csr.rowptr[r + 1]]
        assert (np.diff(c) > 0).all() and (len(c) == 0 or (0 <= c[0] and c[-1] < R.NUM_TABLE_ROWS))
        assert lengths[r] <= 65 or c[-1] < R.NUM_TABLE_ROWS - R.NEGATIVE_ROWS
    assert (np.abs(csr.val) >= 0.5).all() and (np.abs(csr.val) <= 2.0).all()
    t = R.transpose(csr)
    assert np.array_equal(R.dense64(t), R.dense64(csr).T)
    for f in range(t.shape[0]):
        assert (np.diff(t.col[t.rowptr[f]:t.rowptr[f + 1]]) > 0).all()


def test_the_700_term_row_leaves_room_for_one_dropped_term():
    """4 * bound is about 0.18 against a smallest term of 0.25."""
    csr, table, _ = _inputs()
    pre = R.forward64(csr, table)
    longest = np.flatnonzero(np.diff(csr.rowptr) == 700)
    assert len(longest) == 2
    b = 4.0 * R.bound(pre.k, pre.sum_abs)[longest]
    print("700 terms: 4 * bound in [%.4f, %.4f], smallest term %.4f" % (b.min(), b.max(), pre.min_abs[longest].min()))
    assert 0.15 < b.min() and b.max() < 0.22 and pre.min_abs[longest].min() >= 0.25


def test_no_pre_activation_sits_near_a_kink():
    csr = R.structure()
    table, _ = R.tables()
    pre = R.forward64(csr, table)
    terms = pre.k > 0
    assert (np.abs(pre.value[terms]) > R.preactivation_margin(pre)[terms]).all()        # the share of left-out elements is zero
    assert not pre.value[~terms].any()                                                    # an empty row is exactly act(0)


def test_float32_sequential_sum_lies_inside_the_linear_bound():
    csr, table, _ = _inputs()
    pre = R.forward64(csr, table)
    got = R.sequential32(csr, table).astype(np.float64)
    err, tol = np.abs(got - pre.value), R.bound(pre.k, pre.sum_abs)
    print("linear: worst error / bound %.3f" % float((err[tol > 0] / tol[tol > 0]).max()))
    assert (err <= tol).all()
    assert (pre.min_abs[pre.k > 0] > 4.0 * tol[pre.k > 0]).all()                          # one dropped term shows everywhere


@pytest.mark.parametrize("name", R.GRADIENT_ACTIVATIONS)
def test_float32_sequential_gradient_lies_inside_its_bound(name):
    csr, _, dout = _inputs()
    y = R.outputs(name)[:, :N]
    res, tol = R.gradient64(csr, dout, y, name)
    got = R.sequential32(csr, dout, y, name).astype(np.float64)
    err = np.abs(got - res.value)
    has = res.k > 0
    print("%s: worst error / bound %.3f" % (name, float((err[has] / tol[has]).max())))
    assert (err <= tol).all()
    assert (res.min_abs[has] > 4.0 * tol[has]).all(), float((res.min_abs[has] / tol[has]).min())
    if name not in ("linear", "tanh"):                 # the derivative's other branch is among the terms
        d = R.dact_from_output64(name, y.astype(np.float64))
        assert (d[-R.NEGATIVE_ROWS:] != d[0, 0]).any() and (d[:-R.NEGATIVE_ROWS] == d[0, 0]).all()


@pytest.mark.parametrize("name", R.ACTIVATIONS)
def test_activated_forward_restated_in_float32_lies_inside_its_tolerance(name):
    import torch
    csr, table, _ = _inputs()
    want, tol, _ = R.forward_act64(csr, table, name)
    pre32 = torch.from_numpy(R.sequential32(csr, table))
    fn = {"linear": lambda x: x, "tanh": torch.tanh, "relu": torch.relu, "leaky_relu": lambda x: torch.nn.functional.leaky_relu(x, 0.2),
          "elu": torch.nn.functional.elu, "selu": torch.selu, "gelu": lambda x: torch.nn.functional.gelu(x)}[name]
    got = fn(pre32).numpy().astype(np.float64)
    assert (np.abs(got - want) <= tol).all()


def _outside(mutant, res, tol, affected):
    """Share of the affected elements at which a (float64, exactly computed) mutant misses the tolerance."""
    miss = np.abs(mutant - res.value) > tol
    return float(miss[affected].mean())


def _drop(csr, keep):
    counts = np.add.reduceat(keep.astype(np.int64), csr.rowptr[:-1][np.diff(csr.rowptr) > 0])
    lengths = np.zeros(csr.shape[0], np.int64)
    lengths[np.diff(csr.rowptr) > 0] = counts
    return R.Csr(np.concatenate([[0], np.cumsum(lengths)]), csr.col[keep], csr.val[keep], csr.shape)


def test_plausible_mistakes_lie_outside_the_bounds():
    csr, table, dout = _inputs()
    lengths = np.diff(csr.rowptr)
    pre = R.forward64(csr, table)
    tol = R.bound(pre.k, pre.sum_abs)
    nonempty = np.broadcast_to((lengths > 0)[:, None], tol.shape)
    rng = np.random.default_rng(0)
    # one dropped term, anywhere in its row: every element of every non-empty row
    keep = np.ones(len(csr.col), bool)
    keep[[rng.integers(csr.rowptr[r], csr.rowptr[r + 1]) for r in np.flatnonzero(lengths > 0)]] = False
    assert _outside(R.forward64(_drop(csr, keep), table).value, pre, tol, nonempty) == 1.0
    # the last term of a long row's tail dropped
    long_rows = np.flatnonzero(lengths > 128)
    keep = np.ones(len(csr.col), bool)
    keep[csr.rowptr[long_rows + 1] - 1] = False
    assert _outside(R.forward64(_drop(csr, keep), table).value, pre, tol, np.broadcast_to((lengths > 128)[:, None], tol.shape)) == 1.0
    # the value of the neighbouring entry used; un-normalised values (every stored value taken as 1)
    several = np.broadcast_to((lengths > 1)[:, None], tol.shape)
    shifted = csr._replace(val=np.roll(csr.val, -1))
    assert _outside(R.forward64(shifted, table).value, pre, tol, several) > 0.99
    assert _outside(R.forward64(csr._replace(val=np.ones_like(csr.val)), table).value, pre, tol, nonempty) > 0.99
    # the activation applied per term instead of per sum (rows of several terms)
    for name in ("tanh", "relu", "elu"):
        want, atol, _ = R.forward_act64(csr, table, name)
        per_term = R._sum_rows(csr, R.act64(name, csr.val.astype(np.float64)[:, None] * table.astype(np.float64)[csr.col])[0]).value
        assert float((np.abs(per_term - want) > atol)[several].mean()) > 0.9, name
    # the gradient over the transposed structure: the transpose taken without permuting the values; act' of the wrong row
    t = R.transpose(csr)
    tl = np.diff(t.rowptr)
    y = R.outputs("tanh")[:t.shape[1], :N]
    g = dout[:t.shape[1]]
    res, gtol = R.gradient64(t, g, y, "tanh")
    several_t = np.broadcast_to((tl > 1)[:, None], gtol.shape)
    unpermuted = t._replace(val=csr.val)
    assert _outside(R.gradient64(unpermuted, g, y, "tanh")[0].value, res, gtol, several_t) > 0.99
    wrong_row = R.gradient64(t, g, np.roll(y, 1, axis=0), "tanh")[0].value
    assert _outside(wrong_row, res, gtol, np.broadcast_to((tl > 0)[:, None], gtol.shape)) > 0.99
    # ... and one dropped term of the gradient
    keep = np.ones(len(t.col), bool)
    keep[[rng.integers(t.rowptr[f], t.rowptr[f + 1]) for f in np.flatnonzero(tl > 0)]] = False
    assert _outside(R.gradient64(_drop(t, keep), g, y, "tanh")[0].value, res, gtol, np.broadcast_to((tl > 0)[:, None], gtol.shape)) == 1.0
