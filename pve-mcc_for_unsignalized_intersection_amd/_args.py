"""The binding's tensor-argument checks, stated once: what batched.py, replay.py and learner.py accept as a tensor argument and
what they refuse.  Every refusal is a PveError whose text the caller supplies (users and tests match on those texts).
"device": a torch.device; same_device=False compares its type only (a batch created on "cuda" holds tensors of "cuda:0")."""
import numpy as np
import torch

from ._capi import PveError


def is_tensor_of(x, dtype, device=None, same_device=False, shapes=None, numel=None):
    """x is a tensor of `dtype`, on `device` (None: anywhere), whose shape is one of `shapes` and which has `numel` elements
    (None: any)"""
    return (torch.is_tensor(x) and x.dtype == dtype
            and (device is None or (x.device == device if same_device else x.device.type == device.type))
            and (shapes is None or tuple(x.shape) in shapes) and (numel is None or x.numel() == numel))


def tensor_in(x, device, dtype, shape, message, tail=False, convert=True):
    """An input: x (convert=True: a tensor or anything NumPy takes) brought to `device` as `dtype`, made contiguous.  Its shape
    must be `shape`; tail=True: its trailing dimensions must be `shape` and it must not be empty."""
    if convert and not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    x = x.to(device=device, dtype=dtype).contiguous()
    if (tuple(x.shape[-len(shape):]) if tail else tuple(x.shape)) != tuple(shape) or (tail and x.numel() == 0):
        raise PveError(message)
    return x


def tensor_out(out, device, dtype, shape, message, same_shape=False, same_device=False):
    """An output: a fresh tensor of `shape` (out=None), or the caller's contiguous `out` of `dtype` on `device` with as many
    elements (same_shape=True: with that very shape)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    shape = tuple(shape)
    if not is_tensor_of(out, dtype, device, same_device, (shape,) if same_shape else None, int(np.prod(shape))) or not out.is_contiguous():
        raise PveError(message)
    return out
