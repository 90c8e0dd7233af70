"""GPU: guard bands at the tile edges of every C-ABI entry point that writes caller-supplied device memory.

The value of each output is pinned by the oracle tests; what they mostly do not see is WHERE a kernel writes: they hand it
exactly-sized outputs, so a store one row or one 16-byte vector past the end lands in the allocator's slack or in a
neighbouring tensor. Here every case of tests/kernel_bounds_cases.py is called through hanabi_hip._capi with

  * every output carved out of a larger buffer (guard_util.GuardSet): 64 guard elements in front, at least one full workgroup
    tile behind, all of it one fill byte that must still be there afterwards, byte for byte;
  * every input cloned before the call and compared bit for bit after it;

and once more with plain exactly-sized buffers (guard_util.PlainSet): the guarded payloads must equal those bit for bit, which
shows that the guarded call did the real work and that an offset base pointer changes nothing. Every entry point here is
bit-reproducible between two calls (integer sums, or floating-point sums in a fixed order), so no case compares within a bound.

Sizes are the smallest at which the bounds logic can go wrong: for a row tile T, n in {1, T - 1, T + 1}, and one row past a
whole workgroup where it holds several tiles. No case passes a misaligned pointer or a bad size: refusals are tested elsewhere.
One process, one GPU, the default stream."""
import pytest

import kernel_bounds_cases as KB
from guard_util import GuardSet, PlainSet, same_bits

pytestmark = pytest.mark.gpu

ALL = KB.flat_cases()


@pytest.mark.parametrize("entry,fn,params", ALL, ids=[KB.case_id(e, p) for e, _, p in ALL])
def test_entry_point_writes_inside_its_buffers(entry, fn, params):
    import torch

    where = KB.case_id(entry, params)
    guarded = GuardSet(entry)
    fn(guarded, *params)
    torch.cuda.synchronize()
    guarded.check(where)
    assert guarded.outs, f"{where}: the case guards no output"
    assert not guarded.untouched(), f"{where}: outputs the call never wrote (a no-op call proves nothing): {guarded.untouched()}"

    plain = PlainSet(entry)
    fn(plain, *params)
    torch.cuda.synchronize()
    got, want = guarded.payloads(), plain.payloads()
    assert got.keys() == want.keys()
    for name in got:
        i = same_bits(got[name], want[name])
        assert i < 0, (f"{where}: output {name!r} differs between the guarded and the plain call, first at element {i}: "
                       f"{got[name].reshape(-1)[i].item()!r} against {want[name].reshape(-1)[i].item()!r}")
