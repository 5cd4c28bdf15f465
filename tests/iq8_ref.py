"""numpy restatement of the conversion rule of the integer IQ formats (include/tempest_hip.h, TSDR_IQ_*), and the quantisers the
8-bit tests use.  One rounding per component -- the f32 product by scale:

    sc16 / sc8   ComplexF32(f32(I) * scale, f32(Q) * scale)
    uc8          ComplexF32((f32(I) - 127.5f) * scale, (f32(Q) - 127.5f) * scale)      (the subtraction is exact in f32)
"""
import numpy as np

DTYPES = {"sc16": np.int16, "sc8": np.int8, "uc8": np.uint8}
OFFSETS = {"sc16": 0.0, "sc8": 0.0, "uc8": 127.5}
CODES = {"cf32": 0, "sc16": 1, "sc8": 2, "uc8": 3}
BYTES = {"cf32": 8, "sc16": 4, "sc8": 2, "uc8": 2}
FULL_SCALE = {"sc16": 2047.0, "sc8": 127.0, "uc8": 127.0}   # (12 bits in int16, as tests/test_sc16_gpu.py quantises)


def expand(q, fmt, scale):
    """interleaved integer components (2*n) -> complex64[n], as every loader of the library forms them"""
    q = np.asarray(q)
    assert q.dtype == DTYPES[fmt] and q.size % 2 == 0
    v = (q.astype(np.float32) - np.float32(OFFSETS[fmt])) * np.float32(scale)
    assert v.dtype == np.float32
    return v.view(np.complex64)


def quantise(z, fmt):
    """complex64 capture -> (integer components, scale): full scale at the capture's peak component"""
    x = np.ascontiguousarray(z).view(np.float32)
    peak = float(np.max(np.abs(x))) or 1.0
    scale = np.float32(peak / FULL_SCALE[fmt])
    if fmt == "uc8":
        q = np.clip(np.round(x / scale + np.float32(127.5)), 0, 255).astype(np.uint8)
    else:
        q = np.round(x / scale).astype(DTYPES[fmt])
    return q, scale
