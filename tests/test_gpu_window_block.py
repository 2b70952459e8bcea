"""The block of a window of target rows on the GPU (csrc/window_block.hip; tasks/layerwise.py: window_block): every output equals the
NumPy statement of tests/window_block_reference.py exactly, integers and the float degree table; the block is the sampler's own one-hop
exact block; the stamp array is all zero after every call and after a refused one; two streams give the same bytes."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import window_block_reference as WR  # noqa: E402

pytestmark = pytest.mark.gpu

V = WR.HUB_V
HUB = WR.HUB
_DEVICE_GRAPHS = {}


def device_graph(name, adjacency, num_nodes, device):
    """One device RelGraph per test graph, shared by the tests of this module (the reference is computed from the host lists)."""
    from tf_gnn_samples_amd.graph import RelGraph
    if name not in _DEVICE_GRAPHS:
        _DEVICE_GRAPHS[name] = RelGraph([torch.as_tensor(a, device=device) for a in adjacency], num_nodes)
    return _DEVICE_GRAPHS[name]


def host_block(block):
    return WR.Block(block.nodes.cpu().numpy(), [a.cpu().numpy() for a in block.adjacency_lists],
                    block.type_to_num_incoming_edges.cpu().numpy(),
                    tuple(int(a.shape[0]) for a in block.adjacency_lists) + (block.num_sources - block.num_targets,))


def check_block(graph, adjacency, num_nodes, a, b):
    from tf_gnn_samples_amd.tasks.layerwise import window_block, window_blocker
    block = window_block(graph, a, b)
    got, want = host_block(block), WR.window_block(adjacency, num_nodes, a, b)
    assert got.nodes.dtype == np.int32 and got.degrees.dtype == np.float32 and all(x.dtype == np.int32 for x in got.adjacency_lists)
    assert WR.same_block(got, want), (a, b, got.sizes, want.sizes)
    assert (block.num_sources, block.num_targets, block.first, block.last) == (len(want.nodes), b - a, a, b)
    assert block.graph.V == block.num_sources and block.graph.num_targets == b - a and block.graph.M == sum(want.sizes[:-1])
    assert not bool(window_blocker(graph).stamp.any()), (a, b)
    return block, want


@pytest.mark.parametrize("L", [2, 3])
def test_the_windows_of_the_hub_graph(gpu_device, L):
    """[0, 300) has no outside source; [16, 17) is the hub alone, 5 000 entries under one target; every window of B = 64 and B = 250."""
    adjacency, _ = WR.hub_graph(L)
    graph = device_graph(("hub", L), adjacency, V, gpu_device)
    windows = [(0, V), (HUB, HUB + 1), (0, HUB), (HUB, V), (V - 1, V)] + WR.target_windows(V, 64) + WR.target_windows(V, 250)
    assert (250, V) in windows and (256, V) in windows
    for a, b in windows:
        block, want = check_block(graph, adjacency, V, a, b)
        if (a, b) == (0, V):
            assert block.num_sources == V and want.sizes[-1] == 0
        if (a, b) == (HUB, HUB + 1):
            assert want.sizes[1] == 5000 and block.num_targets == 1 and block.num_sources > 200
    # the block's graph is the ordinary constructor's: its by-target slice is the full graph's, re-based
    block, _ = check_block(graph, adjacency, V, 64, 128)
    first, last = int(graph.rowptr_t[64 * L]), int(graph.rowptr_t[128 * L])
    assert np.array_equal(block.graph.rowptr_t[:64 * L + 1].cpu().numpy(), graph.rowptr_t[64 * L:128 * L + 1].cpu().numpy() - first)
    assert block.graph.M == last - first


def test_windows_at_the_tile_and_wave_edges(gpu_device):
    """Windows of exactly 0, 1, 63, 64, 65, 1 023, 1 024, 1 025 and 2 049 entries; one whose every entry has the last type; a source V - 1."""
    adjacency, num_nodes, windows = WR.tile_edge_graph()
    L = len(adjacency)
    graph = device_graph("tiles", adjacency, num_nodes, gpu_device)
    seen = []
    for (a, b), count in windows:
        block, want = check_block(graph, adjacency, num_nodes, a, b)
        assert sum(want.sizes[:L]) == count
        seen.append(count)
    assert seen[:len(WR.EDGE_COUNTS)] == list(WR.EDGE_COUNTS)
    (a, b), count = windows[len(WR.EDGE_COUNTS)]
    assert host_block(check_block(graph, adjacency, num_nodes, a, b)[0]).sizes[:L] == (0,) * (L - 1) + (count,)
    assert num_nodes - 1 in check_block(graph, adjacency, num_nodes, *windows[1][0])[1].nodes
    # windows that straddle the generated ones, and the whole graph (5 356 entries: six tiles, no outside source)
    for a, b in [(3, 77), (40, num_nodes), (0, num_nodes)]:
        check_block(graph, adjacency, num_nodes, a, b)


@pytest.mark.parametrize("L", [2, 3])
def test_the_block_is_the_sampler_s_one_hop_exact_block(gpu_device, L):
    """sample_by_hop(arange(a, b)) with fanouts [0] numbers the seeds first and the nodes first reached in hop 1 ascending behind them,
    and lays a hop's edges type after type in the order of the frontier and, inside a bucket, of its positions: the sampler numbers the
    new sources the same way, so the ARRAYS are equal (nodes, every list, the degree table), not merely the multisets."""
    from tf_gnn_samples_amd.tasks.layerwise import window_block, window_blocker
    from tf_gnn_samples_amd.tasks.neighbour_sampling import NeighbourSampler
    adjacency, _ = WR.hub_graph(L)
    graph = device_graph(("hub", L), adjacency, V, gpu_device)
    sampler = NeighbourSampler(device_graph(("hub-sampler", L), adjacency, V, gpu_device), [0], seed=3)
    for draw, (a, b) in enumerate([(0, V), (HUB, HUB + 1), (0, HUB), (64, 128), (250, V)]):
        sub = sampler.sample_by_hop(np.arange(a, b, dtype=np.int32), draw)
        block = window_block(graph, a, b)
        assert torch.equal(sub.nodes, block.nodes) and sub.num_nodes == block.num_sources and sub.hop_nodes[0] == block.num_targets
        assert all(torch.equal(x, y) for x, y in zip(sub.adjacency_lists, block.adjacency_lists))
        assert torch.equal(sub.type_to_num_incoming_edges, block.type_to_num_incoming_edges)
    assert not bool(window_blocker(graph).stamp.any()) and not bool(sampler.stamp.any())


def test_refusals_leave_the_stamps_zero_and_launch_nothing(gpu_device, monkeypatch):
    from tf_gnn_samples_amd import _lib
    from tf_gnn_samples_amd.tasks.layerwise import window_block, window_blocker
    adjacency, _ = WR.hub_graph(2)
    graph = device_graph(("hub", 2), adjacency, V, gpu_device)
    window_block(graph, 0, 64)
    blocker = window_blocker(graph)
    assert blocker is window_blocker(graph) and blocker.stamp.shape == (V,) and blocker.stamp.dtype == torch.int32
    launched, real = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *args: (launched.append(name), real(name, *args))[1])
    for a, b in [(5, 5), (6, 5), (0, V + 1), (-1, 4), (V, V + 1), (0.0, 4), (0, True)]:
        with pytest.raises(ValueError, match="window_block"):
            window_block(graph, a, b)
    assert launched == [] and not bool(blocker.stamp.any())
    # a call that raises half way (the emit refused) leaves the array zero too: StampedNodeSet's guard
    def failing(name, *args):
        if name == "relgnn_window_block_emit":
            raise RuntimeError("refused")
        return real(name, *args)
    monkeypatch.setattr(_lib, "launch", failing)
    with pytest.raises(RuntimeError, match="refused"):
        window_block(graph, HUB, HUB + 1)
    assert not bool(blocker.stamp.any())
    monkeypatch.setattr(_lib, "launch", real)
    check_block(graph, adjacency, V, HUB, HUB + 1)
    # an empty slice launches nothing over entries and reads nothing back
    empty = [np.zeros((0, 2), np.int32), np.asarray([[0, 1]], np.int32)]
    lonely = device_graph("lonely", empty, 40, gpu_device)
    block, _ = check_block(lonely, empty, 40, 8, 24)
    assert block.num_sources == 16 and block.graph.M == 0
    check_block(lonely, empty, 40, 0, 8)


def test_two_streams_give_the_same_bytes(gpu_device):
    from tf_gnn_samples_amd.tasks.layerwise import window_block
    adjacency, _ = WR.hub_graph(3)
    graph = device_graph(("hub", 3), adjacency, V, gpu_device)
    torch.cuda.synchronize(gpu_device)
    blocks = []
    for _ in range(2):
        stream = torch.cuda.Stream(device=gpu_device)
        with torch.cuda.stream(stream):
            blocks.append(host_block(window_block(graph, 0, 250)))
        stream.synchronize()
    assert WR.same_block(*blocks)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(blocks[0].adjacency_lists, blocks[1].adjacency_lists))
    assert blocks[0].nodes.tobytes() == blocks[1].nodes.tobytes() and blocks[0].degrees.tobytes() == blocks[1].degrees.tobytes()
