"""Inputs shared by the wire-format tests (CPU branch and HIP kernel)."""
import struct

import torch


def f32(bits: int) -> float:
    return struct.unpack('<f', struct.pack('<I', bits))[0]


# ±0, the smallest subnormal, exact ties (to even: 1 + 2^-8 rounds down to 1, 1 + 3 * 2^-8 up
# to 1 + 2^-6), just off the ties, the largest bf16, the largest fp32 (-> inf), ±inf, and
# subnormals around the smallest bf16 subnormal (2^-133)
SPECIAL_BITS = [
    0x00000000, 0x80000000, 0x00000001, 0x80000001,
    0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,
    0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,
    0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7fffff,
    0x7f800000, 0xff800000,
    0x00008000, 0x00008001, 0x00007fff, 0x00018000, 0x007fffff, 0x00800000,
]
NAN_BITS = [0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f80ffff]


def _from_bits(patterns) -> torch.Tensor:
    bits = torch.tensor(patterns, dtype=torch.int64)
    return (bits - (bits >= 2 ** 31) * 2 ** 32).to(torch.int32).view(torch.float32)


def special_values() -> torch.Tensor:
    """The finite / infinite special values as a float32 tensor (no NaN)."""
    return _from_bits(SPECIAL_BITS)


def nan_values() -> torch.Tensor:
    return _from_bits(NAN_BITS)


def spread(n: int, seed: int) -> torch.Tensor:
    """``n`` float32 values over the whole exponent range (random bit patterns, NaN and
    inf patterns replaced by finite ones)."""
    gen = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64)
    x = bits.to(torch.int32).view(torch.float32).clone()
    x[~torch.isfinite(x)] = 1.5
    return x


def mixed(seed: int = 0):
    """A message of every kind of tensor: fp32 (rounded), int64 / bf16 / bool (verbatim)."""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(3, 5, generator=gen),
            torch.randint(-2 ** 40, 2 ** 40, (7,), generator=gen),
            torch.randn(9, generator=gen).to(torch.bfloat16),
            torch.rand(11, generator=gen) > 0.5,
            torch.randn(2, 2, 2, generator=gen)]
