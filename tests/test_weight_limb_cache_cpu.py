"""Host logic of dense.weight_limbs (the limb images of a step's weight operands, split once per optimizer step in one launch),
with the library stubbed out (its split entry point records the launch): which images are (re)split when, and that an evicted
image leaves nothing behind."""
import gc
import types
import weakref

import pytest
import torch

CPU = torch.device("cpu")


@pytest.fixture
def cache(monkeypatch):
    from tf_gnn_samples_amd import _lib, dense as DN, weight_images as WI
    launches = []

    class Lib:
        @staticmethod
        def relgnn_limb_elements(r, c):
            return ((r + 31) // 32) * 32 * c * 3

        @staticmethod
        def relgnn_limb_split_multi_f32(n, *arrays_and_stream):            # one launch: n matrices
            launches.append(n)
            return _lib.OK
    monkeypatch.setattr(_lib, "load_library", lambda: Lib())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    from tf_gnn_samples_amd import config
    monkeypatch.setattr(config.settings, "weight_limb_cache", "1")
    WI.clear()                                             # every test starts from an empty cache
    yield DN, launches
    WI.clear()


def _step(DN, layers, dense):
    for ks in layers:
        DN.weight_limbs(ks, DN.WEIGHT_NN)
    DN.weight_limbs(dense, DN.WEIGHT_NN)
    DN.weight_limbs(dense, DN.WEIGHT_NT)
    for ks in layers[::-1]:
        DN.weight_limbs(ks, DN.WEIGHT_NT)


def test_one_launch_per_step_after_the_first(cache):
    DN, launches = cache
    layers = [[torch.nn.Parameter(torch.randn(32, 32)) for _ in range(3)] for _ in range(3)]
    dense = torch.nn.Parameter(torch.randn(32, 32))
    _step(DN, layers, dense)
    assert launches == [3, 3, 3, 1, 1, 3, 3, 3]            # first step: every image on its own
    for _ in range(3):
        del launches[:]
        DN.weights_changed()
        _step(DN, layers, dense)
        assert launches == [20]                            # 8 images, 20 matrices, one launch
    del launches[:]
    _step(DN, layers, dense)                               # nothing changed (an evaluation pass): nothing is split
    assert launches == []


def test_in_place_writes_and_dead_tensors(cache):
    from tf_gnn_samples_amd import weight_images as WI
    DN, launches = cache
    a, b = torch.nn.Parameter(torch.randn(32, 32)), torch.nn.Parameter(torch.randn(32, 32))
    DN.weight_limbs(a, DN.WEIGHT_NN); DN.weight_limbs(b, DN.WEIGHT_NN)
    del launches[:]
    with torch.no_grad():
        a.add_(1.0)                                        # the version counter moves: only a's image is stale
    DN.weight_limbs(b, DN.WEIGHT_NN)
    assert launches == []
    DN.weight_limbs(a, DN.WEIGHT_NN)
    assert launches == [1]
    v = a.view(32, 32)                                     # a view shares the parameter's identity and version
    DN.weight_limbs(v, DN.WEIGHT_NN)
    assert launches == [1]
    DN.weights_changed(); DN.weights_changed()             # two updates without a request in between
    del launches[:]
    DN.weight_limbs(a, DN.WEIGHT_NN)                       # b's image was not used during the last step: dropped, not re-split
    assert launches == [1]
    assert WI.image_count(CPU) == 1
    del a, v
    DN.weights_changed()
    DN.weight_limbs(b, DN.WEIGHT_NN)                       # the dead parameter's image is forgotten
    assert WI.image_count(CPU) == 1 and launches == [1, 1]


def test_an_evicted_image_leaves_no_reference_to_its_buffer(cache):
    """Six images that are re-split together every step (more than four: their marshalled launch arguments are kept).  An image
    that is evicted — its parameter died; its parameter was not used during the last generation — is referenced by nothing in the
    cache afterwards: a weakref to its buffer, taken before, is dead."""
    from tf_gnn_samples_amd import weight_images as WI
    DN, launches = cache
    params = [torch.nn.Parameter(torch.randn(32, 32)) for _ in range(6)]
    for _ in range(3):                                     # the recurring set: split one by one, then twice in one launch
        for p in params:
            DN.weight_limbs(p, DN.WEIGHT_NN)
        DN.weights_changed()
    assert launches == [1] * 6 + [6, 6] and WI.image_count(CPU) == 6
    bufs = [weakref.ref(DN.weight_limbs(p, DN.WEIGHT_NN)) for p in params]
    assert launches[8:] == [6] and all(r() is not None for r in bufs)
    dead = params.pop()                                    # (a) the parameter dies
    del dead
    DN.weights_changed()
    for p in params:
        DN.weight_limbs(p, DN.WEIGHT_NN)
    gc.collect()
    assert WI.image_count(CPU) == 5 and bufs[5]() is None and all(r() is not None for r in bufs[:5])
    DN.weights_changed()                                   # (b) params[4] sits out a whole generation
    for p in params[:4]:
        DN.weight_limbs(p, DN.WEIGHT_NN)
    DN.weights_changed()
    DN.weight_limbs(params[0], DN.WEIGHT_NN)
    gc.collect()
    assert WI.image_count(CPU) == 4 and bufs[4]() is None and all(r() is not None for r in bufs[:4])
    assert launches[9:] == [5, 5, 4]                       # (the evicted images were dropped, not re-split)


def test_a_parameter_whose_storage_is_replaced_gets_a_new_image(cache):
    """`p.data = other` moves a parameter to another storage WITHOUT moving its version, and nobody calls weights_changed(): the
    image found by the identity of the tensor objects (the second request below) must not be handed out for the new storage."""
    from tf_gnn_samples_amd import weight_images as WI
    DN, launches = cache
    ws = [torch.nn.Parameter(torch.randn(32, 128)) for _ in range(3)]
    im = DN.weight_image(ws, DN.WEIGHT_NN, separate=True)
    assert DN.weight_image(ws, DN.WEIGHT_NN, separate=True) is im and launches == [3]      # found by identity: nothing split
    old = weakref.ref(im.buf)
    version = ws[1]._version
    ws[1].data = torch.randn(32, 128)
    assert ws[1]._version == version
    del im
    im2 = DN.weight_image(ws, DN.WEIGHT_NN, separate=True)
    assert launches == [3, 3] and im2.items[1][0] == ws[1].data_ptr()
    assert DN.weight_image(ws, DN.WEIGHT_NN, separate=True) is im2 and launches == [3, 3]
    gc.collect()
    assert WI.image_count(CPU) == 1 and old() is None      # the image of the old storage went with the request that replaced it
