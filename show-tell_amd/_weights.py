"""The copies of the weights that the kernels read, and the rules that keep them current.

In bf16 no kernel reads a parameter: each reads a derived copy.  A parameter's bf16 working copy lives on the
parameter itself (``p._st_shadow``, valid for the version counter ``_st_shadow_ver`` and the address ``_st_shadow_ptr``);
it is either cast on demand (``working_copy``) or a view of an optimizer's flat bf16 buffer that the step kernel
refreshes (``adopt_working_copy``).  A module that moves (``.cuda()`` / ``.cpu()`` / ``.to()``) forgets the copies of the
tensors that moved (``FollowsMoves``).  Writes behind PyTorch's back are announced with ``showtell_amd.mark_modified``.
Nothing outside this module touches the three attributes.
"""
import torch

from . import ops

_ATTRS = ("_st_shadow", "_st_shadow_ver", "_st_shadow_ptr")


def working_copy(p, dtype):
    """The tensor the kernels read for parameter `p`: itself in fp32 mode, a cached bf16
    shadow otherwise (refreshed when the parameter was modified or moved)."""
    if dtype == torch.float32:
        return p.data
    sh = getattr(p, "_st_shadow", None)
    if (sh is None or sh.device != p.device or getattr(p, "_st_shadow_ver", -1) != p._version
            or getattr(p, "_st_shadow_ptr", 0) != p.data_ptr()):
        if sh is None or sh.device != p.device or sh.shape != p.shape:
            sh = torch.empty(p.shape, device=p.device, dtype=dtype)
        ops.cast(p.data.contiguous(), dtype, out=sh)
        adopt_working_copy(p, sh)
    return sh


def adopt_working_copy(p, view):
    """`view` holds the current values of `p` in the kernels' dtype: working_copy returns it until p changes or moves."""
    p._st_shadow, p._st_shadow_ver, p._st_shadow_ptr = view, p._version, p.data_ptr()


def grad_buffer(p):
    if p.grad is None:
        p.grad = torch.zeros_like(p.data, dtype=torch.float32)
    return p.grad


def storage_places(module):
    """(device, address) of every parameter of `module`, to be taken before Module._apply"""
    return [(p.device, p.data_ptr()) for p in module.parameters()]


def drop_moved_working_copies(module, places):
    """After Module._apply (.cuda() / .cpu() / .to()), with `places` = storage_places(module) from before it: forget the
    working copy of every parameter whose storage moved.  working_copy alone cannot be relied on here: a round trip
    .cpu() -> .cuda() leaves the version counter where it was and the caching allocator hands the block it freed back at
    the same address, so weights written on the host in between (through `.data`, as the reference initialises its layers)
    would be invisible.  Host-side, and only when a module is moved."""
    for p, place in zip(module.parameters(), places):
        if (p.device, p.data_ptr()) != place:
            for attr in _ATTRS:
                if hasattr(p, attr):
                    delattr(p, attr)


class FollowsMoves:
    """Mixin in front of nn.Module: .cuda() / .cpu() / .to() replaced the storage the bf16 copies were cast from."""

    def _apply(self, fn, *a, **k):
        places = storage_places(self)
        out = super()._apply(fn, *a, **k)
        drop_moved_working_copies(self, places)
        return out
