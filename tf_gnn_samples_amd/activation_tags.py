"""Tags on tensor objects through which the Dense products learn what their operands are: an activation's output whose gradient
factor a consumer may fold into its input-gradient product, a gradient that already carries that factor, a gradient whose rows are
zero-padded to a multiple of 16 columns.  Nothing here launches a kernel; dense.py reads the tags when it routes a product."""
import torch

from .activations import FROM_OUTPUT_ACTS as _FROM_OUTPUT_ACTS, IDEMPOTENT_ACTS as _IDEMPOTENT_ACTS
from .config import settings as _cfg

# ---- activation gradients folded into the product that feeds them ------------------------------------------------------------------
# y = act(z) is differentiated from its OUTPUT (relgnn_act_bwd_from_output: tanh, relu, leaky_relu, elu, selu) by the function that
# produced it: g_z = g_y * act'(y) — one pass over [V, D] per activation and step (three ReLU' and two tanh' passes per C2 step,
# 16-34 us each).  The function that CONSUMES y computes g_y as an input-gradient product and can apply act'(y) in that product's
# epilogue (relgnn_limb_gemm_xf32_dact: same bits, no pass).  Protocol, all on Python attributes of the tensors involved:
#   * a producer tags its output:            mark_activation_output(y, act, sole_consumer=...)
#   * a consumer that sees a tagged input x and whose input-gradient route can fuse returns g_x already multiplied by act'(x) and
#     tags it:                               mark_premasked(g_x, x, act)
#   * the producer's backward skips its own pass iff the gradient it receives IS that tagged tensor:  is_premasked(g, y, act)
# A gradient that autograd had to sum with other contributions, copy or pass through a hook arrives as another tensor object
# without the tag, and the producer multiplies as always.  That is exact for ReLU whatever happened in between (its factor is 0 or
# 1: applying it twice, or to a sum whose first term already carries it, changes nothing).  The other activations' factors are not
# idempotent: folding one into ONE of several contributions would leave the producer multiplying the sum again.  They are only
# folded when y provably has exactly one reader in the autograd graph, which takes two words: whoever hands y over vouches that
# only the function it is handed to will read it (the tag's flag: the driver loop of models/sparse_graph_model.py knows its own
# dataflow), and that function says that it reads it exactly once (sole_reader=True: the aggregate-first RGCN layer's first
# timestep, the driver's Dense between layers; a GGNN layer, which feeds its input to the messages AND to the cell, does not).
# (_FROM_OUTPUT_ACTS: tanh .. selu — gelu needs the pre-activation; _IDEMPOTENT_ACTS: relu — both columns of activations.ACTIVATIONS)


def mark_activation_output(y: torch.Tensor, act: int, sole_consumer: bool = False) -> torch.Tensor:
    if act in _FROM_OUTPUT_ACTS and y.is_cuda and y.dtype == torch.float32 and y.dim() == 2:
        y._relgnn_act = (int(act), y._version, bool(sole_consumer))
    return y


def vouch_sole_consumer(y: torch.Tensor, sole: bool) -> torch.Tensor:
    """The caller knows how many functions will read y (a tagged activation output): set / clear the tag's sole-consumer word."""
    tag = getattr(y, "_relgnn_act", None)
    if tag is not None:
        y._relgnn_act = (tag[0], tag[1], bool(sole))
    return y


def fusable_activation_of(x: torch.Tensor, sole_reader: bool = False) -> int:
    """The activation whose gradient a consumer of x may apply in its input-gradient product (0 = none).  sole_reader: the caller
    reads x exactly once (needed, together with the hander's word in the tag, for every activation but ReLU)."""
    tag = getattr(x, "_relgnn_act", None)
    if tag is None or tag[1] != x._version or getattr(x, "_backward_hooks", None) or _cfg.act_fusion != "1":
        return 0
    act, _, only_this_callee = tag
    return act if (act in _IDEMPOTENT_ACTS or (only_this_callee and sole_reader)) else 0


def mark_premasked(g: torch.Tensor, y: torch.Tensor, act: int) -> torch.Tensor:
    g._relgnn_premasked = (y.data_ptr(), y._version, int(act), tuple(y.shape))
    return g


def is_premasked(g: torch.Tensor, y: torch.Tensor, act: int) -> bool:
    return getattr(g, "_relgnn_premasked", None) == (y.data_ptr(), y._version, int(act), tuple(y.shape))


def mark_zero_padded(g: torch.Tensor, ld: int) -> torch.Tensor:
    """g [M, K] is a view of rows of ld >= K floats whose columns K .. ld-1 hold ZEROS (written by g's producer: the loss gradient
    of tasks/ppi_task.py through relgnn_sigmoid_ce_bwd_padded).  A consumer whose product reduces over K may then read [M, ld]
    and meet a reduction length that is a multiple of 16 — the limb route — without a padding copy.  The tag is on the tensor
    object: anything autograd copies, sums or passes through a hook arrives untagged and takes the plain route."""
    g._relgnn_zero_pad = (g.data_ptr(), tuple(g.shape), g.stride(0), int(ld))
    return g


def zero_padded_operand(g: torch.Tensor):
    """The [M, ld] view behind a tensor tagged by mark_zero_padded (None: not tagged, or no longer the tensor that was tagged)."""
    tag = getattr(g, "_relgnn_zero_pad", None)
    if (tag is None or g.dim() != 2 or tag != (g.data_ptr(), tuple(g.shape), g.stride(0), tag[3]) or g.stride(1) != 1
            or g.stride(0) != tag[3] or tag[3] < g.shape[1] or tag[3] % 16):
        return None
    return torch.as_strided(g, (g.shape[0], tag[3]), (tag[3], 1))
