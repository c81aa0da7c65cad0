"""Test infrastructure: tensors carved out of sentinel-filled device buffers (the `Planes` of tests/test_batchnorm_gpu.py for any
number of dimensions and several tensors per buffer).  An Arena is one flat buffer with GUARD sentinel elements in front of and
behind its span; `carve` hands out strided views of it, the ones marked `out` being what a kernel may write.  `seal` remembers the
buffer, `intact` says that nothing but the `out` views has changed since -- inputs, gaps between planes and guard bands alike."""
import torch

GUARD = 64                      # a multiple of 4: a dense view stays 16-byte aligned
SENTINEL = -777.25


def contiguous_strides(shape):
    st, n = [], 1
    for s in reversed(shape):
        st.append(n)
        n *= s
    return tuple(reversed(st))


class Arena:
    def __init__(self, span, device):
        self.buf = torch.full((GUARD + int(span) + GUARD,), SENTINEL, dtype=torch.float32, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.span = int(span)
        self.writable = torch.zeros_like(self.buf, dtype=torch.bool)
        self.snap = None

    def carve(self, shape, strides=None, offset=0, fill=None, out=False):
        strides = tuple(strides) if strides is not None else contiguous_strides(shape)
        assert offset >= 0 and offset + sum((s - 1) * st for s, st in zip(shape, strides)) < self.span
        view = self.buf.as_strided(tuple(shape), strides, GUARD + offset)
        if fill is not None:
            view.copy_(fill)
        if out:
            self.writable.as_strided(tuple(shape), strides, GUARD + offset).fill_(True)
        return view

    def seal(self):
        self.snap = self.buf.clone()

    def restore(self):
        self.buf.copy_(self.snap)

    def intact(self):
        return bool((self.buf[~self.writable] == self.snap[~self.writable]).all())


def dense(shape, device, fill=None, out=False):
    """an Arena holding one contiguous tensor -> (arena, view)"""
    n = 1
    for s in shape:
        n *= s
    a = Arena(n, device)
    return a, a.carve(shape, fill=fill, out=out)
