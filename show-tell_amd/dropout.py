"""Dropout for the decoders: the host side of csrc/dropout.h.

The kernels hold no random-number state.  An element's fate is a pure function of (seed, step, site, packed row, column):
Philox4x32-10 keyed by the 64-bit seed, counter (column / 4, packed row, site, step); kept iff word >= floor(p * 2^32); a kept
element is T(float(x) * float32(1 / (1 - p))), a dropped one +0.  Sites: l = the output of recurrent layer l (L - 1: the rows
in front of ``linear``), SITE_INPUT = the layer-0 input rows.  A module owns a seed and a host-side step counter
(``Decoder.seed_dropout``); each training-mode ``forward()`` / ``loss()`` consumes one step and its backward reuses it -- no
device round trip, and nothing to checkpoint on the device.  tests/_dropout_cases.py holds the numpy replica of the mask.
"""
import warnings

import torch

from ._lib import DropoutDesc, check, dtype_code, lib, ptr, stream

SITE_INPUT = 255
_MASK64 = (1 << 64) - 1


def check_p(name, p):
    """Argument error of a dropout probability, raised at construction: a number in [0, 1) (torch allows 1, which zeroes
    everything and has no finite scale; the kernels refuse it).  Returns it as a float."""
    try:
        v = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in [0, 1) (got {p!r})") from None
    if not 0.0 <= v < 1.0:
        raise ValueError(f"{name} must be in [0, 1) (got {p!r})")
    return v


def signed64(seed):
    """A seed as the C ABI's `long` carries its 64 bits."""
    s = int(seed) & _MASK64
    return s - (1 << 64) if s >> 63 else s


class DropoutState:
    """What a decoder keeps for its dropout: the three probabilities, the seed and the step counter."""

    def __init__(self, p_in=0.0, p_layer=0.0, p_out=0.0, num_layers=1):
        self.p_in, self.p_layer, self.p_out = check_p("dropout_in", p_in), check_p("dropout", p_layer), check_p("dropout_out", p_out)
        if self.p_layer > 0 and num_layers == 1:
            warnings.warn("dropout option adds dropout after all but last recurrent layer, so non-zero dropout expects "
                          f"num_layers greater than 1, but got dropout={p_layer} and num_layers={num_layers}")
        self.layer_on = self.p_layer > 0 and num_layers > 1
        self.seed = torch.initial_seed() & _MASK64
        self.step = 0

    def reseed(self, seed):
        self.seed, self.step = int(seed) & _MASK64, 0

    def active(self):
        return self.p_in > 0 or self.layer_on or self.p_out > 0

    def take(self, training):
        """The (seed, step) of one training-mode call, consuming the step; None when dropout is off for this call."""
        if not (training and self.active()):
            return None
        if self.step >= 2 ** 31 - 1:
            raise OverflowError("the dropout step counter is exhausted: call seed_dropout() with a new seed")
        st = (self.seed, self.step)
        self.step += 1
        return st

    def desc(self, seed_step, nbytes, device):
        """The st_dropout of one call and the buffer of dropped copies it points at (None when no site needs one)."""
        d = DropoutDesc()
        d.p_in, d.p_layer, d.p_out = self.p_in, self.p_layer if self.layer_on else 0.0, self.p_out
        d.seed, d.step = signed64(seed_step[0]), seed_step[1]
        buf = None
        if self.layer_on or self.p_out > 0:
            buf = torch.empty(nbytes, device=device, dtype=torch.uint8)
            d.buf, d.buf_bytes = buf.data_ptr(), nbytes
        return d, buf


def dropout_rows(x, p, seed, step, site, row0=0, out=None):
    """st_dropout_rows on a 2-d fp32 / bf16 device tensor whose rows are contiguous (a row stride is allowed): `out` (default: a
    new tensor; `x` itself for in place) receives the masked rows, row r of `x` being packed row row0 + r."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("dropout_rows takes a 2-d tensor with contiguous rows")
    y = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or y.stride(1) != 1:
        raise ValueError("out must match x in shape and dtype and have contiguous rows")
    check(lib().st_dropout_rows(ptr(x), ptr(y), dtype_code(x.dtype), x.shape[0], x.shape[1], x.stride(0), y.stride(0), float(p),
                                signed64(seed), int(step), int(site), int(row0), stream()), "st_dropout_rows")
    return y
