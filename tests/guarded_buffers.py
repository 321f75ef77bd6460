"""Guarded device buffers of the kernel matrices (tests/test_hip_conv_matrix.py, test_hip_groupnorm_matrix.py, test_hip_attention_matrix.py):
stray reads and writes of a launch show in the values.  Every input lies inside a larger allocation whose guards hold NaN -- an
element read from outside the tensor poisons what is computed from it; every output is pre-filled with NaN between guard rows of a
fixed bit pattern -- an element never written stays NaN, a row written outside the tensor changes a guard.  Nothing is read or
written outside an allocation.  A plain module: no fixtures, no test."""
import torch

GUARD_BITS = {torch.float32: 0x5a5a5a5a, torch.float16: 0x5a5a}
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16}


class GuardedInput:
    """values [rows, cols] of one operand inside a larger device allocation: NaN guards of >= `unit` elements (one object's worth),
    rounded up to a multiple of 256 bytes, before and behind"""

    def __init__(self, dev, values, dtype, unit):
        esize = torch.empty(0, dtype=dtype).element_size()
        g = (unit * esize + 255) // 256 * 256 // esize
        self.whole = torch.full((2 * g + values.numel(),), float('nan'), dtype=dtype, device=dev)
        self.view = self.whole[g:g + values.numel()].view(values.shape)
        self.view.copy_(values.to(dtype))
        self.before = self.whole.clone()

    def unchanged(self):
        it = INT_OF[self.whole.dtype]
        return torch.equal(self.whole.view(it), self.before.view(it))


class GuardedOutput:
    """[rows, cols] of NaN between two blocks of 128 guard rows (a multiple of 256 bytes for every width) of a fixed bit pattern"""
    G = 128

    def __init__(self, dev, rows, cols, dtype):
        self.it, self.bits = INT_OF[dtype], GUARD_BITS[dtype]
        self.whole = torch.empty(rows + 2 * self.G, cols, dtype=dtype, device=dev)
        self.whole.view(self.it).fill_(self.bits)
        self.view = self.whole[self.G:self.G + rows]
        self.view.fill_(float('nan'))

    def guards_unchanged(self):
        w = self.whole.view(self.it)
        return bool((w[:self.G] == self.bits).all()) and bool((w[-self.G:] == self.bits).all())

    def refill(self):
        self.view.fill_(float('nan'))
