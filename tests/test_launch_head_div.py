"""The multiply-shift division of the kernels' launch heads (kernels.h magic_div_make / magic_div), on the CPU.

The GEMM and attention kernels turn a workgroup id into tile indices with divisions by launch constants (column
tiles per row, query blocks per sequence, heads). The launchers pass a multiplier and a shift for each divisor, and
refuse grids outside the range the constants are used for: numerators below kMagicMaxN, divisors up to kMagicMaxD
(f5h_debug_magic_div_sweep reports both). The library walks that whole rectangle -- every numerator with every
divisor -- against `/` and `%` (no device needed); the cases split the divisors so that each stays short.
"""

import ctypes

import pytest

from f5_tts_amd import _lib

CHUNKS = 8


def _limits():
    lim = (ctypes.c_uint32 * 2)()
    assert _lib.lib().f5h_debug_magic_div_sweep(0, 1, 1, lim) == 0
    return int(lim[0]), int(lim[1])


def test_launch_limits_cover_the_shapes_in_use():
    """2^20 workgroups and 2^11 column tiles / query blocks / heads: the all-steps AdaLN table GEMM has
    22 * 6 * 1024 / 128 = 1056 column tiles, the widest in the engine."""
    n_end, d_max = _limits()
    assert n_end >= 1 << 20 and d_max >= 1 << 11, (n_end, d_max)


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_magic_div_exact_over_the_launch_range(chunk):
    n_end, d_max = _limits()
    step = (d_max + CHUNKS - 1) // CHUNKS
    lo, hi = 1 + chunk * step, min(d_max, (chunk + 1) * step)
    bad = _lib.lib().f5h_debug_magic_div_sweep(n_end, lo, hi, None)
    assert bad == 0, (lo, hi, bad)


def test_magic_div_sweep_rejects_bad_ranges():
    L = _lib.lib()
    assert L.f5h_debug_magic_div_sweep(16, 0, 4, None) == -1   # divisor 0
    assert L.f5h_debug_magic_div_sweep(16, 5, 4, None) == -1   # empty divisor range
    assert L.f5h_debug_magic_div_sweep(1 << 31, 1, 1, None) == -1   # numerators past 2^31 (the sum would carry)
