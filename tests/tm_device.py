"""Device-side plumbing shared by tests/test_gpu_tm_kernels.py and tests/test_gpu_bwd_pair_kernels.py: operands inside larger
allocations whose margin rows hold 1024.0, outputs as column windows of wider prefilled arrays between sentinel guards, and the
comparison that names the first wrong (b, t, column).  Nothing here launches a kernel."""
import torch

import tm_cases as C

DEV = "cuda"
GUARD = 1024
SENT = 12288.0              # exact in bf16, fp16 and fp32


def lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Rows:
    """A (B, T, stride) operand in the storage dtype inside a larger allocation whose margin rows hold 1024.0: a read that should
    have been a zero changes an output by a visible amount."""

    def __init__(self, values, dtype, margin_rows):
        B, T, stride = values.shape
        td = C.TORCH_DT[dtype]
        self.stride, self.es = stride, 4 if dtype == "fp32" else 2
        self.buf = torch.full((2 * margin_rows + B * T, stride), C.MARGIN, dtype=td, device=DEV)
        self.mid = self.buf[margin_rows:margin_rows + B * T]
        self.mid.copy_(values.reshape(B * T, stride).to(td))

    def at(self, col=0):
        return self.mid.data_ptr() + col * self.es


class Window:
    """An output of `rows` x `width` as the columns [col0, col0 + width) of a wider array between GUARD sentinels.  The window starts as
    NaN (an element the kernel does not write fails the comparison), the other columns as small integers that must survive."""

    def __init__(self, rows, col0, width, td, init=None):
        self.rows, self.col0, self.width = rows, col0, width
        self.stride = col0 + width + C.PAD
        n = rows * self.stride
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=td, device=DEV)
        pre = ((torch.arange(n) * 7) % 5 + 1).to(torch.float32).view(rows, self.stride)
        pre[:, col0:col0 + width] = float("nan") if init is None else init.reshape(rows, width)
        self.pre = pre.to(td)
        self.t = self.buf[GUARD:GUARD + n].view(rows, self.stride)
        self.t.copy_(self.pre)
        self.es = self.t.element_size()

    def ptr(self):
        return self.t.data_ptr() + self.col0 * self.es

    def result(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[b.numel() - GUARD:] == SENT).all()), f"{what}: a guard region was written"
        t = b[GUARD:b.numel() - GUARD].view(self.rows, self.stride)
        keep = torch.ones(self.stride, dtype=torch.bool)
        keep[self.col0:self.col0 + self.width] = False
        assert torch.equal(_bits(t[:, keep].contiguous()), _bits(self.pre[:, keep].contiguous())), f"{what}: columns outside the output window were written"
        return t[:, self.col0:self.col0 + self.width].float()

    def untouched(self):
        b = self.buf.cpu()
        n = b.numel() - 2 * GUARD
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()) and torch.equal(_bits(b[GUARD:GUARD + n]), _bits(self.pre.view(-1)))


class Flat:
    """A contiguous array (no stride in the ABI) between GUARD sentinels, starting as `init` (NaN where the kernel must write)."""

    def __init__(self, init, td):
        n = init.numel()
        self.shape, self.pre = init.shape, init.to(td)
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=td, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.copy_(self.pre.view(-1))

    def ptr(self):
        return self.t.data_ptr()

    def result(self, what):
        b = self.buf.cpu()
        n = b.numel() - 2 * GUARD
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{what}: a guard region was written"
        return b[GUARD:GUARD + n].view(self.shape).float()

    def untouched(self):
        b = self.buf.cpu()
        n = b.numel() - 2 * GUARD
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()) and torch.equal(_bits(b[GUARD:GUARD + n]), _bits(self.pre.view(-1)))


def upload(x, dtype):
    return x.to(C.TORCH_DT[dtype]).to(DEV).contiguous()


def first_difference(got, want, T, what):
    """got, want: (B * T, columns) fp32 on the CPU; values compare as floats, so -0.0 equals 0.0 -- None if equal"""
    if torch.equal(got, want):
        return None
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    pos = bad.nonzero()
    r, col = pos[0].tolist()
    return (f"{what}: {len(pos)} of {got.numel()} elements differ, first at (b {r // T}, t {r % T}, column {col}): got {float(got[r, col])}, "
            f"want {float(want[r, col])}")
