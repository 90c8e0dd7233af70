"""hb_noisy_adam_multi with a gradient-product entry (learner_tail_l2_dw1_kernel) under the guard-band sweep's protocol
(tests/test_kernel_bounds_gpu.py): once with every output inside guard bands and every input cloned, once on exactly-sized
buffers, the payloads equal bit for bit. The entry point is hb_noisy_adam_multi, which the sweep's table already lists; these
are its cases for the product mode, kept here beside the mode's other tests.

Role B owns one 32 x 64 tile of the product per workgroup: rows one short of a tile, one past, two tiles plus one; columns one
64-column tile, one tile and 8 columns, 8 columns. Role A: hb_noisy_adam_multi's lanes on n_adam stepped entries."""
import numpy as np
import pytest

import kernel_bounds_cases as KB
from guard_util import GuardSet, PlainSet, same_bits

pytestmark = pytest.mark.gpu

ENTRY = "hb_noisy_adam_multi"
TAIL_ROWS = 32
PARAMS = [(dt, b, k, h, na) for dt in ("bfloat16", "float16") for (b, k, h, na) in ((17, 31, 64, 2), (256, 33, 72, 0), (1, 65, 8, 2))]


def gradient_product(g, dtype, batch, k_rows, hidden, n_adam):
    import torch

    import test_learner_kernels_f64 as TL

    rng = np.random.default_rng(batch + k_rows + hidden)
    ldx = (k_rows + 7) // 8 * 8
    x = g.inp("x", TL._dev(rng.standard_normal((batch, ldx)), dtype)[0])
    dh = g.inp("dh", TL._dev(rng.standard_normal((batch, hidden)) * 0.1, dtype)[0])
    ld = hidden + 4
    out = g.out("dw1", (k_rows, ld), dtype, KB.tail(TAIL_ROWS, ld))
    ts = [KB._adam_tensor(g, f"t{i}", rng, r, c, dtype, dtype, True, 4, KB.LANE_ROWS * 4)
          for i, (r, c) in enumerate(((17, 12), (1, 128))[:n_adam])]
    tab = (KB._K().HbAdamTensor * (1 + len(ts)))()
    for i, T in enumerate(ts):
        T.table_entry(tab[i])
    d = tab[len(ts)]                   # the product entry, last in the table
    d.grad, d.grad_dtype, d.grad_ld, d.n, d.cols = out.data_ptr(), KB.CODE[dtype], ld, k_rows * hidden, hidden
    d.gx, d.gdh, d.g_batch, d.g_ldx, d.g_ldh = x.data_ptr(), dh.data_ptr(), batch, ldx, hidden
    step = g.inp("step", torch.tensor([2.0], device="cuda"))
    KB._call(ENTRY, tab, 1 + len(ts), KB._p(step), 0.0, KB.CODE[dtype], KB.LR, KB.B1, KB.B2, KB.EPS)


@pytest.mark.parametrize("params", PARAMS, ids=["-".join(str(v) for v in p) for p in PARAMS])
def test_gradient_product_writes_inside_its_buffers(params):
    import torch

    where = f"{ENTRY} product {params}"
    guarded = GuardSet(ENTRY)
    gradient_product(guarded, *params)
    torch.cuda.synchronize()
    guarded.check(where)
    assert guarded.outs and not guarded.untouched(), where
    plain = PlainSet(ENTRY)
    gradient_product(plain, *params)
    torch.cuda.synchronize()
    got, want = guarded.payloads(), plain.payloads()
    assert got.keys() == want.keys()
    for k in got:
        assert same_bits(got[k], want[k]) == -1, (where, k, same_bits(got[k], want[k]))
