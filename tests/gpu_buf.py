"""Guarded device buffers shared by the GPU tests that call kernels through
the C ABI: an array on the device between NaN guard elements (integer guards
for an integer array), and bitwise comparison.
"""
import numpy as np

GUARD = 2  # elements: keeps the array 16-byte aligned


class Buf:
    """A [z][y][x] array on the device between NaN guards, `off` elements
    (8 bytes each) past 16-byte alignment."""

    def __init__(self, arr, off=0):
        import torch
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        self.shape, self.n, self.lo = arr.shape, arr.size, GUARD + off
        self.host = np.full(self.lo + self.n + GUARD, np.nan)
        self.host[self.lo:self.lo + self.n] = arr.ravel()
        self.t = torch.from_numpy(self.host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.lo

    def get(self):
        """the array now; the guards must hold their bits"""
        import torch
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        hi = self.lo + self.n
        assert same_bits(a[:self.lo], self.host[:self.lo]) and same_bits(a[hi:], self.host[hi:]), "guard overwritten"
        return a[self.lo:hi].reshape(self.shape)

    def unchanged(self):
        return same_bits(self.get().ravel(), self.host[self.lo:self.lo + self.n])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def nans(shape):
    return np.full(tuple(shape)[::-1], np.nan)


class IntBuf:
    """An integer array (any numpy integer type, bytes included) on the
    device between `nguard` guard elements of its own type."""

    def __init__(self, arr, guard=-77, nguard=16):
        import torch
        arr = np.ascontiguousarray(arr)
        assert arr.dtype.kind in "iu" and arr.ndim == 1
        self.n, self.lo = arr.size, nguard
        self.host = np.full(self.n + 2 * nguard, guard, dtype=arr.dtype)
        self.host[self.lo:self.lo + self.n] = arr
        self.t = torch.from_numpy(self.host.copy()).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.host.itemsize * self.lo

    def get(self):
        """the array now; the guards must hold their values"""
        import torch
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        hi = self.lo + self.n
        assert np.array_equal(a[:self.lo], self.host[:self.lo]) and np.array_equal(a[hi:], self.host[hi:]), \
            "guard overwritten"
        return a[self.lo:hi]

    def unchanged(self):
        return np.array_equal(self.get(), self.host[self.lo:self.lo + self.n])
