"""Guarded device buffers for the tests that hold an entry point to its workspace plan and to its outputs.

A guarded buffer is ONE uint8 device allocation of ``HEAD + payload + TAIL`` bytes.  Both guards hold ``GUARD``; the payload holds a
byte the caller chooses (0xFF reads as NaN in a float or a double, as -1 in an int, as 255 in a byte).  The payload starts 4,096
bytes into the allocation, so it keeps the allocator's alignment (the entry points ask for 16 or 256 bytes).  ``guard_case`` is
the two-call protocol built on it: the same call once over a zeroed and once over a 0xFF workspace, every output in a guarded
buffer of its own, nothing compared but bits and byte patterns."""
import math

import torch

HEAD = TAIL = 4096
GUARD = 0xA5
POISON = 0xFF
DEV = "cuda:0"


class Guarded:
    """``shape`` elements of ``dtype`` between two guards; ``ptr`` is the payload's address, ``view`` its typed view."""

    def __init__(self, shape, dtype=torch.uint8, fill=POISON, device=DEV):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.nbytes = math.prod(self.shape) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.empty(HEAD + self.nbytes + TAIL, dtype=torch.uint8, device=device)
        self.raw[:HEAD] = GUARD
        self.raw[HEAD:HEAD + self.nbytes] = fill
        self.raw[HEAD + self.nbytes:] = GUARD
        self.bytes = self.raw[HEAD:HEAD + self.nbytes]
        self.ptr = self.raw.data_ptr() + HEAD
        self.view = self.bytes.view(dtype).view(self.shape)
        self.fill = fill
        assert self.ptr % 256 == 0

    def intact(self):
        """Both guards still hold GUARD; waits for the device first."""
        torch.cuda.synchronize()
        return bool((self.raw[:HEAD] == GUARD).all()) and bool((self.raw[HEAD + self.nbytes:] == GUARD).all())

    def written(self):
        """No element still holds the pre-fill: a float is finite (the 0xFF pre-fill is a NaN), an integer or a byte is not the pre-fill's
        value.  Only meaningful for a payload filled with POISON."""
        assert self.fill == POISON
        if self.view.dtype.is_floating_point:
            return bool(torch.isfinite(self.view).all())
        return bool((self.view != (POISON if self.view.dtype == torch.uint8 else -1)).all())


def same_bits(a, b):
    """Two tensors of one shape and dtype hold the same bytes (NaNs compare by their bits)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def guard_case(entry, need_bytes, outputs, call, reference=None, fills=(0x00, POISON), last_error=None, inout=None):
    """The protocol of one entry point.  ``outputs``: name -> (shape, dtype), pre-filled with POISON; ``inout`` (optional): name -> the
    tensor a buffer that the entry point reads AND writes (parameters, Adam moments) starts from, copied afresh for every call;
    ``call(ws, out)`` makes the call with the guarded workspace ``ws`` (exactly ``need_bytes`` long) and the dict ``out`` of guarded
    buffers (outputs and in/out alike) and gives the return code; ``reference``: name -> the tensor the public wrapper returned, or
    left behind, for the same inputs (None: guards and written elements only).  Asserted in this order: the return code and every
    guard per call, the calls equal bit for bit, every output element written (in/out buffers: finite), the reference.  Returns the
    buffers of the last call as plain tensors."""
    assert need_bytes > 0, (entry, need_bytes, last_error() if last_error else None)
    inout = inout or {}
    calls = []
    for fill in fills:
        ws = Guarded(need_bytes, torch.uint8, fill)
        out = {name: Guarded(shape, dtype, POISON) for name, (shape, dtype) in outputs.items()}
        for name, start in inout.items():
            out[name] = Guarded(start.shape, start.dtype, 0x00)
            out[name].view.copy_(start)
        rc = call(ws, out)
        assert rc == 0, (entry, rc, last_error() if last_error else None)
        assert ws.intact(), f"{entry}: the call wrote outside the {need_bytes} bytes its planner reports (workspace pre-fill {fill:#04x})"
        for name, g in out.items():
            assert g.intact(), f"{entry}: the call wrote outside its buffer `{name}` {g.shape}"
        calls.append(out)
    print(f"{entry}: workspace of {need_bytes} bytes pre-filled with {', '.join(f'{f:#04x}' for f in fills)}; outputs "
          f"{ {k: v.shape for k, v in calls[0].items() if k not in inout} } pre-filled with {POISON:#04x}"
          f"{f'; in/out {sorted(inout)}' if inout else ''}; "
          f"{'compared with the wrapper' if reference is not None else 'guards and written elements only'}")
    for other in calls[1:]:
        for name in calls[0]:
            assert same_bits(calls[0][name].view, other[name].view), f"{entry}: `{name}` depends on what the workspace held before the call"
    for out in calls:
        for name, g in out.items():
            ok = bool(torch.isfinite(g.view).all()) if name in inout else g.written()
            assert ok, f"{entry}: `{name}` {g.shape} has elements that are unwritten or not finite"
    if reference is not None:
        assert set(reference) == set(calls[0]), (entry, sorted(reference), sorted(calls[0]))
        for name, want in reference.items():
            got = calls[0][name].view
            assert same_bits(got, want.reshape(got.shape)), f"{entry}: `{name}` differs from what the public wrapper returns"
    return {name: g.view for name, g in calls[-1].items()}
