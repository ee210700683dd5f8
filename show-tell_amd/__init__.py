"""show-tell on MI355X: HIP/CDNA4 kernels behind the reference's nn.Module surface.

    from showtell_amd.cnn import ResNet                 # cnn.py
    from showtell_amd.rnn import RNN                    # rnn.py
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM   # LSTM/rnn_lstm.py
    from showtell_amd.cnn_attn import ResNet            # Attention/cnn_attn.py
    from showtell_amd import optim                      # SGD / Adam of main.py:96-100
"""
from . import _lib  # noqa: F401
from ._lib import ShowTellHipError  # noqa: F401

__all__ = ["ShowTellHipError", "mark_modified"]


def mark_modified(*modules_or_parameters):
    """Tell the kernels' cached weight copies that tensors were written behind PyTorch's back.

    No bf16 kernel reads a parameter directly: each reads a derived copy (the bf16 working copies of _weights.working_copy and
    of the optimizers, the backbone's packed filters) that is refreshed when the parameter's version counter or address
    changes.  An in-place write through ``.data`` (``p.data.copy_(..)``, ``p.data.normal_()``) or through a raw pointer
    moves neither, so after such writes to a model that has already run, call this on the modules or tensors written:
    it bumps the version counter of every parameter and buffer given (modules, tensors, or lists / generators of
    either, e.g. ``rnn.parameters()``) and drops a backbone's packed filters (they are packed again by the next forward).
    Host-side only: no kernel launch, no synchronisation."""
    import torch

    def tensors_of(obj):
        if isinstance(obj, torch.nn.Module):
            for sub in obj.modules():
                bb = getattr(sub, "_bb", None)
                if bb is not None:
                    bb.invalidate_packed()
            return list(obj.parameters()) + list(obj.buffers())
        if torch.is_tensor(obj):
            return [obj]
        if isinstance(obj, (str, bytes)) or not hasattr(obj, "__iter__"):
            raise TypeError(f"mark_modified takes modules, tensors or iterables of them, not {type(obj).__name__}")
        return [t for o in obj for t in tensors_of(o)]

    for t in tensors_of(modules_or_parameters):
        torch.autograd.graph.increment_version(t)
