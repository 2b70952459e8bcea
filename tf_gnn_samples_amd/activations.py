"""The activations of the reference's get_activation (utils/utils.py:36-58): ONE table, one row each — the id the kernels take
(_lib.ACT_*), the accepted name, the torch callable, and the two facts the fused routes ask about.  Every other view (name -> id,
name -> callable, id -> callable, the id sets) is read off it."""
import math
from collections import namedtuple
from typing import Optional

import torch

from . import _lib


def _gelu(x):
    # erf form of the reference (utils/utils.py:53-55)
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x * cdf


def _leaky_relu(x):
    return torch.nn.functional.leaky_relu(x, 0.2)  # tf.nn.leaky_relu default alpha


# from_output: the derivative follows from the OUTPUT (relgnn_act_bwd_from_output; safe to fuse as an epilogue) — gelu needs the
# pre-activation.  idempotent: the gradient factor is 0 or 1, applying it twice changes nothing (activation_tags.py).
Activation = namedtuple("Activation", "id name fn from_output idempotent")
ACTIVATIONS = (
    Activation(_lib.ACT_LINEAR, "linear", None, False, False),
    Activation(_lib.ACT_TANH, "tanh", torch.tanh, True, False),
    Activation(_lib.ACT_RELU, "relu", torch.relu, True, True),
    Activation(_lib.ACT_LEAKY_RELU, "leaky_relu", _leaky_relu, True, False),
    Activation(_lib.ACT_ELU, "elu", torch.nn.functional.elu, True, False),
    Activation(_lib.ACT_SELU, "selu", torch.selu, True, False),
    Activation(_lib.ACT_GELU, "gelu", _gelu, False, False),
)
_BY_NAME = {a.name: a for a in ACTIVATIONS}
_BY_ID = {a.id: a for a in ACTIVATIONS}

FROM_OUTPUT_ACTS = tuple(a.id for a in ACTIVATIONS if a.from_output)
IDEMPOTENT_ACTS = tuple(a.id for a in ACTIVATIONS if a.idempotent)
FUSABLE_ACTS = {_lib.ACT_LINEAR, *FROM_OUTPUT_ACTS}


def _named(name: str, shown: str) -> Activation:
    if name not in _BY_NAME:
        raise ValueError("Unknown activation function '%s'!" % shown)
    return _BY_NAME[name]


def activation_id(activation_fun: Optional[str]) -> int:
    """Same accepted strings and error as get_activation (utils/utils.py:36-58)."""
    if activation_fun is None:
        return _lib.ACT_LINEAR
    return _named(activation_fun.lower(), activation_fun).id


def get_activation(activation_fun: Optional[str]):
    if activation_fun is None:
        return None
    activation_fun = activation_fun.lower()
    return _named(activation_fun, activation_fun).fn


def activation_of_id(act: int):
    """The callable get_activation returns for the name of id `act` (None: linear)."""
    return _BY_ID[act].fn


def apply_activation(fn, x):
    return x if fn is None else fn(x)
