"""What the callers of the library's polygon-soup entry points share
(mesh.polygon_report, render, topology): inputs moved to the device and
checked for length, the handle of a repeated build and its stage times.
Imports nothing of this package at load time, so all three may import it."""
from __future__ import annotations

import ctypes as C

import numpy as np


def current_device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def to_device(x, dev, dtype):
    """A numpy array or a tensor as a contiguous tensor of `dtype` on `dev`
    (one already in place passes through unchanged)."""
    import torch
    x = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.to(dev, dtype).contiguous()


def soup_on_device(vertices, offsets, indices, dev, prefix: str = ""):
    """``(v, off, idx, P)``: vertices fp32 [V, 3] (None stays None), offsets
    int64 [P + 1] and indices int64 on `dev`, after the two length checks the
    library cannot make; their messages start with `prefix`."""
    import torch
    v = None if vertices is None else to_device(vertices, dev, torch.float32).reshape(-1, 3)
    off, idx = to_device(offsets, dev, torch.int64).reshape(-1), to_device(indices, dev, torch.int64).reshape(-1)
    P = off.numel() - 1
    if P < 0:
        raise ValueError(f"{prefix}offsets holds P + 1 entries")
    if P > 0 and idx.numel() < int(off[-1]):  # (the library reads indices[:offsets[-1]])
        raise ValueError(f"{prefix}offsets end at {int(off[-1])}, only {idx.numel()} indices given")
    return v, off, idx, P


class Handle:
    """A library handle on device `dev`, made by the function named `create`
    and freed by the one named `destroy`: ``h.h`` is the pointer, ``h.close()``
    frees it."""

    def __init__(self, dev, create: str, destroy: str):
        from .. import _hip
        self._hip, self._destroy, self.h = _hip, destroy, C.c_void_p()
        _hip.check(getattr(_hip.lib(), create)(C.byref(self.h), dev.index), create)

    def close(self):
        if self.h:
            getattr(self._hip.lib(), self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stage_ms(stages_fn, handle: Handle, names) -> dict:
    """The stage times of the handle's last timed build, by name
    (``stages_fn``: its tnp_debug_*_stages); timing is switched off."""
    ms = (C.c_double * len(names))()
    stages_fn(handle.h, 0, ms, len(names))
    return dict(zip(names, (float(x) for x in ms)))
