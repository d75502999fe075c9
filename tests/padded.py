"""Output buffers with a pitch, an offset base and guard columns (a plain helper module, shared by
test_gpu_ragged.py and test_gpu_dense_ragged.py)."""


def _torch():
    import torch

    return torch


class _Padded:
    """A column-major rows x cols matrix with leading dimension ld inside a buffer prefilled with a
    NaN bit pattern: base one element past the allocation, one guard column before and one after."""

    def __init__(self, rows, cols, ld, dtype):
        torch = _torch()
        self.idt = torch.int64 if dtype == torch.float64 else torch.int32
        self.pattern = 0x7FF8000000012345 if dtype == torch.float64 else 0x7FC12345
        self.rows, self.cols, self.ld = rows, cols, ld
        self.flat = torch.full((1 + (cols + 2) * ld,), self.pattern, dtype=self.idt, device="cuda")
        self.grid = self.flat[1:].view(cols + 2, ld)          # row j: column j - 1 of the matrix
        self.mat = self.grid[1:cols + 1, :rows].view(dtype).t()
        assert self.mat.stride() == (1, ld)
        assert self.mat.data_ptr() == self.flat.data_ptr() + (1 + ld) * self.flat.element_size()

    def padding_untouched(self):
        torch = _torch()
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        keep[1:].view(self.cols + 2, self.ld)[1:self.cols + 1, :self.rows] = False
        return bool((self.flat[keep] == self.pattern).all())
