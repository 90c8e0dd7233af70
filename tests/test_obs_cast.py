"""GPU: hb_obs_cast (csrc/policy.hip, obs_cast_kernel) through the C-ABI against numpy. int8 -> bf16 / fp16 is exact for every int8
value, so every assertion is equality.

  16-byte chunk path and the cols % 16 tail      cols 1, 15 (tail only), 16 (chunks only), 17, 171, 658, 1 280
  unaligned 16-byte loads                        odd cols: row r starts at byte r * cols
  unaligned 16-byte stores                       out_ld = cols + 1: row r starts at an odd element
  the grid-stride loop                           26 000 x 658: more 16-column chunks than 4 096 workgroups x 256 lanes
  the tail's own stride loop                     300 x 15: one workgroup, 4 500 tail elements
  "padding columns are never written"            the output is full of a sentinel: columns [cols, out_ld) and one whole extra
                                                 row after the last keep it"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HB_OK, HB_ERR_INVALID = 0, -1
CODE = {"bfloat16": 1, "float16": 2}
SENTINEL = 12.5            # exact in bf16 and fp16, and no int8 value
GRID_CAP, BLOCK = 4096, 256
SHAPES = [(1, 1), (3, 15), (5, 16), (257, 17), (64, 171), (1000, 658), (300, 1280), (26000, 658),
          (300, 15)]   # no chunk, so one workgroup: 4 500 tail elements for 256 lanes, the tail's stride loop runs 18 times


def _K():
    from hanabi_hip import _capi as K

    return K


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=2)
def _inputs(rows, cols):
    """name -> int8 [rows, cols]: 0 / 1 rows at densities 0, 0.3 and 1, and the full int8 range with -128 and 127 in it"""
    rng = np.random.default_rng(rows * 4099 + cols)
    full = rng.integers(-128, 128, (rows, cols)).astype(np.int8)
    full.reshape(-1)[0] = -128
    full.reshape(-1)[-1] = 127
    if full.size >= 256:
        full.reshape(-1)[:256] = np.arange(-128, 128).astype(np.int8)      # every int8 value
    return {"zeros": np.zeros((rows, cols), np.int8), "ones": np.ones((rows, cols), np.int8),
            "bits": (rng.random((rows, cols)) < 0.3).astype(np.int8), "int8": full}


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_obs_cast_equals_numpy_and_leaves_padding_alone(rows, cols, dtype):
    import torch

    K = _K()
    L, s = K.lib(), K.current_stream()
    if rows == 26000:
        assert rows * (cols >> 4) > GRID_CAP * BLOCK, "this shape must make the grid-stride loop run more than once"
    if (rows, cols) == (300, 15):
        assert cols >> 4 == 0 and rows * (cols & 15) > BLOCK, "this shape must make the tail's stride loop run more than once"
    tdt = getattr(torch, dtype)
    for out_ld in (cols, cols + 1, (cols + 63) // 64 * 64):
        for name, src in _inputs(rows, cols).items():
            src_d = torch.from_numpy(src).cuda()
            out = torch.full((rows + 1, out_ld), SENTINEL, dtype=tdt, device="cuda")
            K.check(L.hb_obs_cast(_ptr(src_d), _ptr(out), CODE[dtype], rows, cols, out_ld, s))
            want_d = torch.from_numpy(src.astype(np.float32)).cuda()        # every int8 value is a bf16 and an fp16 value
            got = out.float()                                               # (compared on the device: 18 M elements at the largest)
            where = (rows, cols, out_ld, dtype, name)
            assert torch.equal(got[:rows, :cols], want_d), (where, "values")
            assert bool((got[:rows, cols:] == SENTINEL).all()), (where, "padding columns written")
            assert bool((got[rows] == SENTINEL).all()), (where, "the row after the last written")
            assert torch.equal(src_d, torch.from_numpy(src).cuda()), (where, "input changed")


def test_obs_cast_argument_checks():
    import torch

    K = _K()
    L, s = K.lib(), K.current_stream()
    src = torch.ones((4, 20), dtype=torch.int8, device="cuda")
    out = torch.full((4, 24), SENTINEL, dtype=torch.bfloat16, device="cuda")
    assert L.hb_obs_cast(_ptr(src), _ptr(out), 1, 4, 20, 19, s) == HB_ERR_INVALID and b"out_ld" in L.hb_last_error()
    for code in (0, 3, -1):
        assert L.hb_obs_cast(_ptr(src), _ptr(out), code, 4, 20, 24, s) == HB_ERR_INVALID and b"out_dtype" in L.hb_last_error()
    assert L.hb_obs_cast(None, _ptr(out), 1, 4, 20, 24, s) == HB_ERR_INVALID and b"null" in L.hb_last_error()
    assert L.hb_obs_cast(_ptr(src), _ptr(out), 1, 0, 20, 24, s) == HB_OK
    torch.cuda.synchronize()
    assert (out.float() == SENTINEL).all(), "a refused or empty call wrote"
