"""The edge_mlp route switch and the panel table of the fused first product of an edge MLP (csrc/edge_mlp_fused.hip): host code only."""
import numpy as np
import pytest


def test_the_switch_defaults_to_the_materialised_route():
    from tf_gnn_samples_amd import config
    assert config.default_of("edge_mlp") == "materialize"
    before = config.current()
    with config.override(edge_mlp="fused") as s:
        assert s.edge_mlp == "fused" and config.settings.edge_mlp == "fused"
    assert config.current() == before
    with pytest.raises(ValueError, match="RELGNN_EDGE_MLP must be one of"):
        with config.override(edge_mlp="both"):
            pass
    assert config.current() == before
    assert config.attribute_of("RELGNN_EDGE_MLP") == "edge_mlp"


def test_panel_table_covers_every_message_once_within_its_type():
    from tf_gnn_samples_amd.graph import edge_mlp_panel_table
    offsets = [0, 900, 1200, 1200, 1328, 1329, 1458]
    table = edge_mlp_panel_table(offsets)
    assert table.dtype == np.int32 and table.ndim == 2 and table.shape[1] == 4 and table.flags["C_CONTIGUOUS"]
    first, rows, wsel, pad = (table[:, i].astype(np.int64) for i in range(4))
    assert (pad == 0).all()
    assert ((rows >= 1) & (rows <= 128)).all()
    seen = np.zeros(offsets[-1], dtype=np.int64)
    for f, r in zip(first, rows):
        seen[f:f + r] += 1
    assert (seen == 1).all()                                              # every message in exactly one panel
    for f, r, l in zip(first, rows, wsel):
        assert offsets[l] <= f and f + r <= offsets[l + 1], (f, r, l)     # no panel crosses a type boundary; weight index = type
    assert 2 not in set(wsel.tolist())                                    # the empty type has no panel
    by_type = {l: rows[wsel == l].tolist() for l in range(6)}
    assert by_type[0] == [128] * 7 + [4]                                  # 900 = 7 * 128 + 4
    assert by_type[1] == [128, 128, 44]
    assert by_type[2] == []
    assert by_type[3] == [128]
    assert by_type[4] == [1]
    assert by_type[5] == [128, 1]
    assert (np.diff(first) > 0).all()                                     # in message order


@pytest.mark.parametrize("offsets", [[0], [0, 0, 0]])
def test_panel_table_of_no_messages_is_empty(offsets):
    from tf_gnn_samples_amd.graph import edge_mlp_panel_table
    table = edge_mlp_panel_table(offsets)
    assert table.shape == (0, 4) and table.dtype == np.int32


def test_route_rule_keeps_the_materialised_route_without_the_switch():
    """The rule answers before it touches the library or the tensors when the switch is off (the default) or the limb route is."""
    from tf_gnn_samples_amd import config
    from tf_gnn_samples_amd.gnns import pair
    assert pair._edge_mlp_fused_ok(None, None, None, 0, 0) is False
    with config.override(edge_mlp="fused", gemm="lib"):
        assert pair._edge_mlp_fused_ok(None, None, None, 0, 0) is False
