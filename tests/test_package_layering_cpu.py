"""The package's layering ("Layering"): every sibling import at module top and pointing downwards, the ops package a flat
list of re-exports of the same objects, one activation table."""
import ast
import importlib
import math
import pathlib
import subprocess
import sys
import types

import pytest
import torch

import tf_gnn_samples_amd as pkg
from tf_gnn_samples_amd import _lib, activation_tags, activations, graph, handover, ops, utils, weight_grad_stream

ROOT = pathlib.Path(pkg.__file__).parent
# top-level name (module or subpackage) -> layer; an import may point to the same or a lower layer only
LAYERS = {name: i for i, names in enumerate([
    ("_lib", "config", "_build", "variables"),
    ("activations", "handover", "activation_tags", "weight_grad_stream", "weight_images"),
    ("graph", "dense_kernels", "dense"),
    ("ops",),
    ("utils",),
    ("gnns", "tasks", "predict", "parallel"),
    ("models",),
]) for name in names}
# inside ops/: segment imports no sibling, the other families import segment only, __init__ imports them all
OPS_FAMILIES = {"segment", "edge", "typed", "rgat", "rgcn", "rgdcn", "dropout"}
# (module, imported name) pairs that may stay inside a function: hoisting them closes a cycle at import time
LAZY_ALLOWED = {
    ("tasks.sparse_graph_task", "GraphStore"),      # tasks.batcher imports DeviceBatch from tasks.sparse_graph_task at its top
}


def _modules():
    for path in sorted(ROOT.rglob("*.py")):
        rel = path.relative_to(ROOT).with_suffix("")
        parts = rel.parts[:-1] if rel.name == "__init__" else rel.parts
        yield ".".join(parts), path, rel.name == "__init__"


def _sibling_imports(name, path, is_init):
    """(node, in_function, target module relative to the package, imported names) for every import of a package sibling."""
    tree = ast.parse(path.read_text())
    here = name.split(".") if name else []
    package = here if is_init else here[:-1]

    def visit(node, in_function):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ImportFrom) and child.level:
                base = package[:len(package) - (child.level - 1)]
                target = base + (child.module.split(".") if child.module else [])
                yield child, in_function, ".".join(target), [a.name for a in child.names]
            elif isinstance(child, (ast.Import, ast.ImportFrom)):
                names = [child.module] if isinstance(child, ast.ImportFrom) else [a.name for a in child.names]
                assert not any(n and n.split(".")[0] == pkg.__name__ for n in names), "%s: absolute import of the package" % name
            yield from visit(child, in_function or isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)))

    yield from visit(tree, False)


def test_sibling_imports_sit_at_module_top_and_point_downwards():
    lazy, seen = set(), 0
    for name, path, is_init in _modules():
        if not name:
            continue
        top = name.split(".")[0]
        assert top in LAYERS, "%s has no layer: add it to LAYERS (and to DESIGN.md)" % name
        for node, in_function, target, names in _sibling_imports(name, path, is_init):
            seen += 1
            if in_function:
                lazy |= {(name, n) for n in names}
                continue
            # `from . import a, b` / `from .. import a, b` name modules; `from .a import x` names a module's contents
            targets = [target] if (target and node.module) else [".".join(filter(None, [target, n])) for n in names]
            for t in targets:
                assert LAYERS[t.split(".")[0]] <= LAYERS[top], "%s (line %d) imports %s from a higher layer" % (name, node.lineno, t)
                if top == "ops" and t.split(".")[0] == "ops" and not is_init:
                    assert name != "ops.segment" and t == "ops.segment", "%s imports %s: ops families import ops.segment only" % (name, t)
    assert seen > 100 and lazy == LAZY_ALLOWED
    assert not any(m.split(".")[0] in ("ops", "dense", "dense_kernels", "graph", "utils", "activations", "handover") for m, _ in LAZY_ALLOWED)
    assert {p.stem for p in (ROOT / "ops").glob("*.py")} == OPS_FAMILIES | {"__init__"}


def test_every_module_imports_without_a_gpu_or_the_library():
    """In a fresh interpreter (here everything is imported already): no import loads librelgnn or initialises the GPU runtime."""
    names = [pkg.__name__ + "." + name for name, _, _ in _modules() if name]
    code = ("import importlib, torch\n"
            "from tf_gnn_samples_amd import _lib\n"
            "def refuse(*a, **k): raise AssertionError('load_library() during import')\n"
            "_lib.load_library = refuse\n"
            "for name in %r: importlib.import_module(name)\n"
            "assert not torch.cuda.is_initialized()\n" % names)
    done = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT.parent), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]


def test_ops_reexports_are_the_home_modules_objects(monkeypatch):
    tree = ast.parse((ROOT / "ops" / "__init__.py").read_text())
    assert all(isinstance(n, ast.ImportFrom) or (isinstance(n, ast.Expr) and isinstance(n.value, ast.Constant)) for n in tree.body), \
        "ops/__init__.py is a list of re-exports and nothing else"
    count = 0
    for node in tree.body[1:]:
        home = importlib.import_module("." + (node.module or ""), pkg.__name__ + (".ops" if node.level == 1 else ""))
        for a in node.names:
            assert getattr(ops, a.asname or a.name) is getattr(home, a.name), a.name
            count += 1
    assert count > 50
    assert ops.SplitPlan is graph.SplitPlan and ops.LONG_SEGMENT is graph.LONG_SEGMENT
    assert ops.handover_word is handover.handover_word and ops.HandoverError is handover.HandoverError
    assert ops.activation_id is activations.activation_id and ops._FUSABLE_ACTS is activations.FUSABLE_ACTS
    assert utils.get_activation is activations.get_activation and utils.apply_activation is activations.apply_activation
    assert (activation_tags._FROM_OUTPUT_ACTS, activation_tags._IDEMPOTENT_ACTS) == (activations.FROM_OUTPUT_ACTS, activations.IDEMPOTENT_ACTS)
    for private in ("_DEFER", "_SIDE_STREAMS", "_accumulator_keeps_the_tensor", "_side_stream"):
        assert hasattr(weight_grad_stream, private) and not hasattr(ops, private)
    # outside callers go through the package attribute: a test that replaces it intercepts them
    for target in ("aggregate_then_transform", "unsorted_segment_sum", "edge_mlp_first_product"):
        assert target in vars(ops) and isinstance(vars(ops)[target], types.FunctionType)
        monkeypatch.setattr(ops, target, target)
        assert utils.ops is ops and getattr(ops, target) is target
    assert utils.get_aggregation_function("sum") == "unsorted_segment_sum"


_X = torch.cat([torch.linspace(-12.0, 12.0, 1001), torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, 1e-20, -1e-20,
                                                                 88.0, -88.0, 1e4, -1e4, 1e30, -1e30, 3.4e38, -3.4e38])]).float()
# the reference's get_activation (utils/utils.py:36-58): name -> (_lib id, the expression this project has always computed)
_EXPECTED = {
    "linear": (_lib.ACT_LINEAR, None),
    "tanh": (_lib.ACT_TANH, torch.tanh),
    "relu": (_lib.ACT_RELU, torch.relu),
    "leaky_relu": (_lib.ACT_LEAKY_RELU, lambda x: torch.nn.functional.leaky_relu(x, 0.2)),
    "elu": (_lib.ACT_ELU, torch.nn.functional.elu),
    "selu": (_lib.ACT_SELU, torch.selu),
    "gelu": (_lib.ACT_GELU, lambda x: x * (0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))))),
}


@pytest.mark.parametrize("name", list(_EXPECTED))
def test_activation_table_agrees_with_every_view_of_it(name):
    act, expr = _EXPECTED[name]
    for spelling in (name, name.upper(), name.title()):
        assert activations.activation_id(spelling) == act == getattr(_lib, "ACT_" + name.upper())
        fn = activations.get_activation(spelling)
        assert fn is activations.activation_of_id(act)
        assert (fn is None) == (expr is None)
        if expr is not None:
            assert torch.equal(fn(_X).view(torch.int32), expr(_X).view(torch.int32))      # bit for bit
    assert activations.apply_activation(None, _X) is _X
    if name in ("tanh", "relu", "elu", "selu"):
        assert fn is expr                                                                 # the same objects as ever


def test_activation_sets_and_errors():
    ids = {n: i for n, (i, _) in _EXPECTED.items()}
    assert [a.id for a in activations.ACTIVATIONS] == list(range(7)) and [a.name for a in activations.ACTIVATIONS] == list(_EXPECTED)
    assert set(activations.FROM_OUTPUT_ACTS) == {ids[n] for n in ("tanh", "relu", "leaky_relu", "elu", "selu")}
    assert set(activations.IDEMPOTENT_ACTS) == {ids["relu"]}
    assert activations.FUSABLE_ACTS == {ids["linear"]} | set(activations.FROM_OUTPUT_ACTS)
    assert activations.activation_id(None) == _lib.ACT_LINEAR and activations.get_activation(None) is None
    assert utils._GRU_FUSABLE == {None: 0, "linear": 0, "tanh": 1, "relu": 2, "leaky_relu": 3, "elu": 4, "selu": 5}
    with pytest.raises(ValueError) as e:
        activations.activation_id("Swish")
    assert str(e.value) == "Unknown activation function 'Swish'!"                        # the caller's string
    with pytest.raises(ValueError) as e:
        activations.get_activation("Swish")
    assert str(e.value) == "Unknown activation function 'swish'!"                        # the reference reports the lowered one


@pytest.mark.parametrize("Din,Dout,route", [(12, 100, None), (7, 9, None), (64, 96, (1024, 6)), (10, 60, (600, 1)), (32, 32, (1024, 1))])
def test_tile_sum_takes_the_general_sub_rule(monkeypatch, Din, Dout, route):
    """1024-float pieces where the matrix splits into them, the whole matrix where it is small and float4-sized, else per-type sums."""
    from tf_gnn_samples_amd.ops import typed
    counts, calls = [2, 0, 3], []
    part = torch.randn(sum(counts), Din, Dout)
    side = types.SimpleNamespace(chunk_counts=counts, weight_grad_plan=lambda K: ("rowptr%d" % K, "col"))

    def reduce(mode, X, rowptr, stride, col, w, num_out):
        calls.append((mode, tuple(X.shape), rowptr, stride, col, w, num_out))
        return torch.zeros(num_out, X.shape[1])

    monkeypatch.setattr(typed, "_seg_reduce_raw", reduce)
    got = typed._sum_tiles_per_type(part, side, len(counts))
    assert got.shape == (3, Din, Dout)
    if route is None:
        assert not calls
        assert torch.equal(got, torch.stack([part[0:2].sum(0), torch.zeros(Din, Dout), part[2:5].sum(0)]))
    else:
        sub, K = route
        assert calls == [(_lib.AGG_SUM, (5 * K, sub), "rowptr%d" % K, 1, "col", None, 3 * K)]
