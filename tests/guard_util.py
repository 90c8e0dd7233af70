"""Guard bands around caller-supplied kernel outputs, and bit-exact snapshots of kernel inputs.

A kernel output is carved out of one larger tensor: FRONT guard elements, the payload, `tail_elems` guard elements, every byte
of all three set to one fill byte that is neither 0x00 nor 0xFF. A kernel that stores before the start of its output, or past
its end by up to one tile, changes a guard byte; one that writes into an input changes the input against its clone. Both are
found by `GuardSet.check` after the caller has synchronised. What this cannot see: loads out of bounds, stores that land beyond
the tail guard, and memory the library owns itself.

`PlainSet` has the same interface and hands out exactly-sized tensors without guards: a case run once on each proves that the
guarded call did the same work as an ordinary one (tests/test_kernel_bounds_gpu.py)."""
import numpy as np

FRONT = 64    # guard elements before the payload: 64 * itemsize is a multiple of 16 bytes for every dtype used
FILL = 0x5A   # not all-zero, not all-one bits; as int8 90, as fp32 1.5e16, as int32 1515870810: nothing a kernel here writes


def _torch():
    import torch

    return torch


def _dtype(d):
    """A torch dtype, or its name ("int8", "bfloat16", ...)."""
    return getattr(_torch(), d) if isinstance(d, str) else d


def _numel(shape):
    return int(np.prod(shape, dtype=np.int64)) if len(shape) else 1


def guarded(shape, dtype, fill=FILL, tail_elems=FRONT, device="cuda"):
    """(buffer, view): `buffer` is a 1-D tensor of FRONT + prod(shape) + tail_elems elements of `dtype` whose every BYTE is
    `fill`; `view` is its contiguous payload of `shape`. The payload keeps the buffer's 16-byte alignment."""
    torch = _torch()
    dtype = _dtype(dtype)
    shape = tuple(int(s) for s in shape)
    tail_elems = int(tail_elems)
    if tail_elems < FRONT:
        raise ValueError(f"a tail guard is at least {FRONT} elements, got {tail_elems}")
    if not 0 < int(fill) < 255:
        raise ValueError("the fill byte must be neither 0x00 nor 0xFF")
    n = _numel(shape)
    item = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((FRONT + n + tail_elems) * item,), int(fill), dtype=torch.uint8, device=device)
    buf = raw.view(dtype)
    view = buf[FRONT:FRONT + n].view(shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def _first_diff(a_u8, b_u8):
    """Index of the first byte at which two uint8 tensors differ, or -1."""
    torch = _torch()
    ne = a_u8 != b_u8
    if not bool(ne.any()):
        return -1
    return int(torch.nonzero(ne)[0, 0])


class GuardSet:
    """Collects the guarded outputs and the inputs of one call of one entry point.

    out(name, shape, dtype, tail_elems, init=None) -> the payload view to pass to the kernel (dtype: a torch dtype or its name).
        `init` (a tensor of that shape)
        makes it an in/out argument: the payload starts as a copy of it. Without it the payload holds the fill bytes.
    inp(name, tensor) -> the tensor itself; a clone is kept.
    check(where): after a synchronise, both guards of every output hold the fill byte for byte and every input equals its
        clone bit for bit; otherwise an AssertionError naming `where`, the buffer and the first damaged element offset
        (relative to the payload's first element for outputs: negative = front guard, >= numel = tail guard)."""

    guards = True

    def __init__(self, entry="", device="cuda", fill=FILL):
        self.entry, self.device, self.fill = entry, device, fill
        self.outs = {}     # name -> (buffer, view, tail_elems)
        self.inps = {}     # name -> (tensor, clone)
        self.fresh = []    # outputs without `init`: their payload is all fill bytes until the kernel writes it

    def out(self, name, shape, dtype, tail_elems, init=None):
        if name in self.outs or name in self.inps:
            raise KeyError(f"buffer name {name!r} used twice")
        buf, view = guarded(shape, dtype, self.fill, tail_elems, self.device)
        if init is not None:
            view.copy_(init.reshape(view.shape))
        self.outs[name] = (buf, view, int(tail_elems))
        if init is None:
            self.fresh.append(name)
        return view

    def inp(self, name, tensor):
        if name in self.outs or name in self.inps:
            raise KeyError(f"buffer name {name!r} used twice")
        self.inps[name] = (tensor, tensor.clone())
        return tensor

    def payloads(self):
        return {k: v[1] for k, v in self.outs.items()}

    def untouched(self):
        """Names of the non-empty outputs created without `init` whose payload still holds nothing but fill bytes: the call
        did not write them at all."""
        torch = _torch()
        return [n for n in self.fresh if self.outs[n][1].numel() and
                bool((self.outs[n][1].reshape(-1).view(torch.uint8) == self.fill).all())]

    def problems(self):
        torch = _torch()
        bad = []
        for name, (buf, view, tail) in self.outs.items():
            item = buf.element_size()
            raw = buf.view(torch.uint8)
            n = view.numel()
            front = raw[:FRONT * item]
            i = _first_diff(front, torch.full_like(front, self.fill))
            if i >= 0:
                bad.append(f"output {name!r}: front guard damaged, first at element {i // item - FRONT} "
                           f"(byte {i % item} of it; {FRONT} guard elements before a payload of {n})")
            back = raw[(FRONT + n) * item:]
            assert back.numel() == tail * item
            i = _first_diff(back, torch.full_like(back, self.fill))
            if i >= 0:
                bad.append(f"output {name!r}: tail guard damaged, first at element {n + i // item} "
                           f"(byte {i % item} of it; payload of {n} elements, {tail} guard elements after it)")
        for name, (t, clone) in self.inps.items():
            a = t.contiguous().reshape(-1).view(torch.uint8)
            b = clone.contiguous().reshape(-1).view(torch.uint8)
            i = _first_diff(a, b)
            if i >= 0:
                item = t.element_size()
                bad.append(f"input {name!r}: changed by the call, first at element {i // item} (byte {i % item} of it)")
        return bad

    def check(self, where=None):
        bad = self.problems()
        if bad:
            raise AssertionError(f"{where or self.entry}: " + "; ".join(bad))


class PlainSet:
    """GuardSet's interface on exactly-sized tensors: no guards, no clones. Untouched payload bytes hold the same fill.
    Inputs are kept alive like GuardSet keeps them: a case may hand the kernel raw pointers after its own references are gone."""

    guards = False

    def __init__(self, entry="", device="cuda", fill=FILL):
        self.entry, self.device, self.fill = entry, device, fill
        self.outs = {}
        self.inps = {}

    def out(self, name, shape, dtype, tail_elems, init=None):
        torch = _torch()
        dtype = _dtype(dtype)
        shape = tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        t = torch.full((max(_numel(shape), 1) * item,), int(self.fill), dtype=torch.uint8, device=self.device)
        t = t.view(dtype)[:_numel(shape)].view(shape)
        if init is not None:
            t.copy_(init.reshape(t.shape))
        self.outs[name] = t
        return t

    def inp(self, name, tensor):
        if name in self.outs or name in self.inps:
            raise KeyError(f"buffer name {name!r} used twice")
        self.inps[name] = tensor
        return tensor

    def payloads(self):
        return dict(self.outs)

    def check(self, where=None):
        pass


def same_bits(a, b):
    """-1 if two tensors of one shape and dtype hold the same bytes, else the first differing element offset."""
    torch = _torch()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.numel() == 0:
        return -1
    i = _first_diff(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    return -1 if i < 0 else i // a.element_size()
