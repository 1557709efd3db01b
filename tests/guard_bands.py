"""0xA5 guard bands behind every buffer a call allocates: what a test looks at to see that a kernel wrote nothing past
the end of a buffer it was given.  Shared by the GPU tests that run calls with too small a capacity."""
import contextlib
import math

import numpy as np
import torch

GUARD = 256                                   # bytes of 0xA5 behind every buffer a guarded call allocates


@contextlib.contextmanager
def guarded_empty():
    """Every torch.empty inside the block hands out the front of a larger buffer whose last GUARD bytes are 0xA5; yields
    the list of those guards (uint8 views), to be looked at after the call."""
    real, guards = torch.empty, []

    def empty(*size, dtype=None, device=None, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dtype = dtype or torch.float32
        item = torch.tensor([], dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        pad = -nbytes % 16
        buf = torch.full((nbytes + pad + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        guards.append(buf[nbytes:])
        return buf[:nbytes].view(dtype).view(shape)

    torch.empty = empty
    try:
        yield guards
    finally:
        torch.empty = real


def guards_intact(guards):
    return all(bool((g == 0xA5).all()) for g in guards)


def forget_workspaces():
    """Drops the cached workspaces of robosimgs_amd._lib.sized_call: the next call allocates its own -- inside
    guarded_empty() that is one more guarded buffer, filled with 0xA5 throughout."""
    from robosimgs_amd import _lib
    _lib._workspaces.clear()


def workspace_slack_intact():
    """A cached workspace is a quarter larger than the call asked for (it grows rarely), so the guard behind it is far
    from the last byte in use.  Allocated inside guarded_empty() the whole buffer starts as 0xA5: the part the call was
    never given -- numel = int((size + 256) * 1.25) + 256 bytes of which at most 255 + size are in use, i.e. everything
    from (numel - 255) / 1.25 on -- must still be.  False where no workspace was allocated."""
    from robosimgs_amd import _lib
    bufs = list(_lib._workspaces.values())
    return bool(bufs) and all(bool((b[int(math.ceil((b.numel() - 255) / 1.25)):] == 0xA5).all()) for b in bufs)
