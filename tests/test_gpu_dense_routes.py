"""The complete route table of dense.py: for every case of tests/dense_route_cases.py — layouts, shapes, activations, `weight`,
`premask`, `out=` and switch values — the sequence of librelgnn entry points the product launches (or the exception it raises),
against tests/golden/dense_routes.json.  The fixture was recorded by that file's `record` command at the commit BEFORE dense.py's
routing was gathered into _route(): the refactor may not move a single product to another entry point.  The two cases that combine
out= with an activation other than ReLU / a premask are the exception: the old code dropped out= silently, now they raise."""
import json
from pathlib import Path

import pytest

import dense_route_cases as RC

GOLDEN = Path(__file__).resolve().parent / "golden" / "dense_routes.json"
# out= together with an epilogue that only a fresh result can carry: ValueError instead of a result that ignores out=
NOW_REFUSED = ("nn_out_accumulate_tanh", "nt_out_premask")


@pytest.mark.gpu
def test_every_dense_product_ends_on_the_recorded_entry_points(gpu_device):
    from tf_gnn_samples_amd import _lib
    want = json.loads(GOLDEN.read_text())
    handle = _lib.load_library()
    got = RC.run(gpu_device)
    assert _lib.load_library() is handle                                  # the recording proxy is gone again
    assert sorted(got) == sorted(want)
    for name in NOW_REFUSED:
        assert want[name]["raises"] is None and want[name]["calls"], name  # (the parent launched the product and ignored out=)
        assert got[name] == {"calls": [], "queries": [], "raises": "ValueError"}, (name, got[name])
    wrong = {name: (got[name], want[name]) for name in want if name not in NOW_REFUSED and got[name] != want[name]}
    assert not wrong, wrong


def test_the_route_table_reaches_every_entry_point_the_dense_modules_call():
    """A condition on the case list, not a measurement: every relgnn_* name in dense.py and the modules split out of it appears in
    the recorded table."""
    import re
    want = json.loads(GOLDEN.read_text())
    recorded = {c for row in want.values() for c in row["calls"] + row["queries"]}
    pkg = Path(__file__).resolve().parent.parent / "tf_gnn_samples_amd"
    called = set()
    for module in ("dense.py", "dense_kernels.py", "activation_tags.py"):
        called |= set(re.findall(r"[.\"](relgnn_\w+)[(\"]", (pkg / module).read_text()))
    assert called and not (called - recorded), sorted(called - recorded)
