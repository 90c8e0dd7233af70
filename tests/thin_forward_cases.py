"""The case tables of tests/test_thin_forward_f64.py (hb_thin_forward on the device), kept apart from it so that the host test
tests/test_thin_forward_cpu.py can check them without importing a device test module."""
BF, HF = "bfloat16", "float16"

# layer 1: B, n, k, dtype, fp32 out, bias
LAYER1_CASES = [(B, n, k, dt, False, True) for (B, n, k) in [(32, 64, 32), (32, 64, 96), (64, 128, 64), (224, 64, 160),
                                                             (256, 1024, 704)] for dt in (BF, HF)]
LAYER1_CASES += [
    (64, 128, 96, BF, True, True),        # fp32 output
    (32, 64, 32, HF, False, False),       # bias = NULL
    (64, 96, 96, BF, False, True),        # n % 32 == 0 with n / 2 = 48: three tiles of the online half (the header: n % 32 == 0)
    (64, 96, 32, HF, False, True),
]

# layer 2: A, K, hidden k, B, dtype, n = A K rounded up to, fp32 out, bias.  Every (A, K), k and B with both dtypes.
LAYER2_CASES = [
    (1, 1, 32, 32, BF, 16, True, True),
    (1, 1, 96, 64, HF, 16, True, True),
    (2, 16, 96, 64, BF, 16, True, True),
    (2, 16, 64, 224, HF, 16, True, True),
    (3, 17, 64, 224, BF, 16, True, True),
    (3, 17, 512, 256, HF, 16, True, True),
    (20, 51, 512, 256, BF, 64, True, True),      # the 2-player learner's launch: 140 + 1 024 units, walking
    (20, 51, 512, 256, HF, 16, True, True),
    (48, 51, 32, 32, HF, 64, True, True),        # n = 2 496 as FusedLearner pads it (2 448 = 153 tiles otherwise)
    (48, 51, 96, 256, BF, 16, True, True),
    (64, 64, 64, 64, BF, 16, True, True),
    (64, 64, 32, 224, HF, 16, True, True),
    (30, 7, 512, 224, BF, 16, True, True),
    (30, 7, 96, 32, HF, 16, True, True),
    (5, 33, 32, 256, BF, 16, True, True),
    (5, 33, 64, 64, HF, 16, True, True),
    (20, 51, 96, 224, BF, 16, False, True),      # 16-bit output
    (5, 33, 96, 224, HF, 16, False, True),
    (48, 51, 64, 256, BF, 16, True, False),      # bias = NULL
    (3, 17, 32, 64, HF, 16, True, False),
    (30, 7, 32, 32, BF, 16, False, False),       # both
    (64, 64, 512, 256, HF, 64, True, True),
    (2, 16, 32, 256, BF, 64, False, True),
    (1, 1, 64, 224, HF, 64, True, True),
]
WALKING = (20, 51, 256, 1024)       # A, K, B, n of the launch whose wavefronts walk more than one unit
