"""The hand-over status word of the wave-role kernels (include/relgnn.h RELGNN_HANDOVER_*): one int32[2] block per device, who
allocates it, who reads it and how a set bit is reported.  Nothing outside this module reads _HANDOVER_WORDS."""
from typing import Optional

import torch

_HANDOVER_WORDS = {}


def handover_word(device=None) -> torch.Tensor:
    """The hand-over status block of `device` (int32[2] in HBM, include/relgnn.h RELGNN_HANDOVER_*): the kernels whose wave roles hand
    data over through LDS counters (relgnn_limb_gemm_xf32_pc: the default forward products; relgnn_rgcn_fused_fwd) OR a bit into
    word 0 when one of their bounded polls runs out — such a launch has written wrong numbers.  The library neither allocates nor
    remembers anything: the block is the caller's, like `err_flag`.  One per device, allocated by the first caller — a model does it
    when it is built, so that a step captured into a hipGraph carries a live pointer (an allocation cannot be captured)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    w = _HANDOVER_WORDS.get(dev.index)
    if w is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the hand-over status block of %s does not exist yet and cannot be allocated inside a stream "
                               "capture: call ops.handover_word(device) (or build the model) before capturing" % dev)
        w = torch.zeros(2, dtype=torch.int32, device=dev)
        _HANDOVER_WORDS[dev.index] = w
    return w


def handover_status(reset: bool = True, device=None) -> int:
    """Word 0 of handover_word(device): 0 = every poll of every launch so far completed.  Waits for the current stream (.item() is a
    stream-ordered copy), not for the device: a training / evaluation loop does not call this — it reads the word with every step's
    metrics copy (models.readback.MetricsReadback) and raises there; this is for code that launches the kernels directly (tests,
    scripts, smoke())."""
    w = handover_word(device)
    v = int(w[0].item())
    if reset and v:
        w[0].zero_()
    return v


class HandoverError(RuntimeError):
    pass


def raise_on_handover(value: int):
    if value:
        raise HandoverError(
            "a wave-role kernel gave up on an LDS hand-over (status 0x%x:%s%s%s%s): the results of that launch are wrong — every "
            "step since the last clean check is suspect" % (
                value, " fused-layer matrix wave" if value & 1 else "", " fused-layer gather wave" if value & 2 else "",
                " product matrix wave" if value & 4 else "", " product producer wave" if value & 8 else ""))


def handover_word_if_any(device) -> Optional[torch.Tensor]:
    """The hand-over status block of `device` if somebody has allocated one (handover_word), else None; allocates nothing.  For a
    readback that carries the word to the host with a copy of its own (models/readback.py)."""
    return _HANDOVER_WORDS.get(torch.device(device).index)


def report_handover(value: int, device):
    """`value`: word 0 of `device`'s status block as read on the host, by whatever copy brought it there.  Not zero: raises
    HandoverError after zeroing the device's word — reported once; later steps start clean."""
    if value:
        word = handover_word_if_any(device)
        if word is not None:
            word[0].zero_()
        raise_on_handover(value)
