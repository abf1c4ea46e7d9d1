"""What the "padded / guarded operand" GPU tests share: the case-seed hash, the strided layout and its geometry, the guarded buffer with its
"everything outside the logical region kept its bits" check, the guarded 0x5A byte region (blob, workspace), the margin-report fixture and
the 16-bit bit-pattern helpers.  numpy only at import time (the *_cases.py files import their GPU twin on a machine without a device):
torch is imported inside the functions that need it.  Host construction and upload are separate steps everywhere, and the checks are pure
numpy functions of the read-back array (tests/test_guard_testlib.py holds them without a device)."""
import numpy as np

import parity_testlib as pl


def seed(salt, *xs):
    """The case seed: a hash of the file's salt and the case's names and numbers."""
    s = salt
    for x in xs:
        s = s * 1000003 + (sum(map(ord, x)) if isinstance(x, str) else int(x))
    return s % (1 << 32)


# ---------------------------------------------------------------------------------------------
# the strided layout
# ---------------------------------------------------------------------------------------------
class Layout:
    """Where the logical operands lie: element offsets of the bases, lda = k + lda_pad, strideX = its contiguous value + gapX
    (gapB None: one shared B, strideB = 0); rs: an fp8 row_scale (the 1-byte file)."""

    def __init__(self, lda_pad=0, gapA=0, gapB=None, gapC=0, offA=0, offB=0, offC=0, batch=2, alpha=1.0, beta=0.0, rs=False):
        self.lda_pad, self.gapA, self.gapB, self.gapC = lda_pad, gapA, gapB, gapC
        self.offA, self.offB, self.offC, self.batch, self.alpha, self.beta, self.rs = offA, offB, offC, batch, alpha, beta, rs


class Strided:
    """The geometry of `batch` [m][k] matrices A, nb (1: shared, or batch) blocks of k * n elements B and `batch` [m * n] results C that
    start at the element indices baseA / baseB / baseC of their buffers: lda, the strides sA / sB / sC the call is given, and the index
    maps iA / iB / iC of the logical elements.  How long each buffer is is the caller's decision."""

    def __init__(self, m, n, k, lay, baseA, baseB, baseC):
        self.m, self.n, self.k, self.lay = m, n, k, lay
        self.batch = batch = lay.batch
        self.baseA, self.baseB, self.baseC = baseA, baseB, baseC
        self.lda = lda = k + lay.lda_pad
        self.sA = m * lda + lay.gapA
        self.nb = nb = 1 if lay.gapB is None else batch
        self.sBe = sBe = k * n + (lay.gapB or 0)          # one B's extent in its buffer, also when the one B is shared ...
        self.sB = 0 if lay.gapB is None else sBe          # ... and the call's strideB is 0
        self.sC = m * n + lay.gapC
        self.iA = (baseA + np.arange(batch)[:, None, None] * self.sA + np.arange(m)[None, :, None] * lda + np.arange(k)[None, None, :]).reshape(-1)
        self.iB = (baseB + np.arange(nb)[:, None] * sBe + np.arange(k * n)[None, :]).reshape(-1)
        self.iC = (baseC + np.arange(batch)[:, None] * self.sC + np.arange(m * n)[None, :]).reshape(-1)


# ---------------------------------------------------------------------------------------------
# the guarded buffer
# ---------------------------------------------------------------------------------------------
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}      # what torch takes (it has uint8 and no other unsigned type)


def outside_mask(n, idx):
    """[n] bool: True where an element is none of the logical elements idx (an index array or a slice)."""
    outside = np.ones(n, dtype=bool)
    outside[idx] = False
    return outside


def changed_outside(got, want, idx):
    """The indices outside the logical elements at which the read-back array differs from what was sent."""
    return np.flatnonzero(outside_mask(got.size, idx) & (got != want))


class Guarded:
    """`n` elements of 1, 2, 4 or 8 bytes, kept as bits and filled with `fill` (NaN around an input, a sentinel around an output); the logical
    elements are host[idx] -- an index map, or the `size` elements from `base` on -- and `base` is where the call's pointer points."""

    def __init__(self, n, fill, dtype, base, idx=None, size=None):
        self.host = np.full(n, fill, dtype=dtype)
        self.base, self.idx = base, slice(base, base + size) if idx is None else idx

    @classmethod
    def around(cls, payload, fill, front, back):
        """A contiguous payload (any 1-, 2-, 4- or 8-byte type: taken as bits) with `front` guard elements before and `back` behind it."""
        payload = np.ascontiguousarray(payload)
        payload = payload.view(UNSIGNED[payload.dtype.itemsize]).reshape(-1)
        g = cls(front + payload.size + back, fill, payload.dtype, front, size=payload.size)
        g.host[g.idx] = payload
        return g

    @property
    def outside(self):
        return outside_mask(self.host.size, self.idx)

    def to_device(self):
        import torch
        self.dev = torch.from_numpy(self.host.view(SIGNED[self.host.itemsize])).cuda()
        assert self.dev.data_ptr() % 16 == 0   # so that the base alignment is the offset's
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.host.itemsize * self.base

    def read(self):
        """The whole device buffer as bits, after a synchronize: ONE copy -- every check below takes it as an argument."""
        import torch
        torch.cuda.synchronize()
        return self.dev.cpu().numpy().view(self.host.dtype)

    def unchanged(self):
        return np.array_equal(self.read(), self.host)

    def assert_outside_kept(self, said, got=None):
        """The read-back buffer, after asserting that everything outside the logical elements kept its bits.  said(n, first): the caller's
        message, from how many elements changed and the buffer indices of the first eight of them."""
        got = self.read() if got is None else got
        changed = changed_outside(got, self.host, self.idx)
        assert changed.size == 0, said(changed.size, changed[:8])
        return got

    def result(self, said, got=None):
        """The logical elements as bits, after asserting that everything outside them kept its bits."""
        return self.assert_outside_kept(said, got)[self.idx]


# ---------------------------------------------------------------------------------------------
# the guarded byte region: a blob, a workspace
# ---------------------------------------------------------------------------------------------
BYTE = 0x5A


def bytes_outside_written(h, off, nbytes):
    """Whether a byte before `off` or from off + nbytes on no longer holds 0x5A."""
    return not ((h[:off] == BYTE).all() and (h[off + nbytes:] == BYTE).all())


class ByteRegion:
    """Exactly `nbytes` bytes of 0x5A at `off` bytes from a base aligned to `align`, `back` more behind them: all of it is `dev`, the
    region itself `p` / `ptr`."""
    OUTSIDE, WRITTEN = "bytes outside the reported size were written", "the region was written"     # a subclass says what it is

    def __init__(self, nbytes, off, back, align):
        import torch
        self.nbytes, self.off = nbytes, off
        self.dev = torch.full((off + nbytes + back,), BYTE, dtype=torch.uint8, device="cuda")
        assert self.dev.data_ptr() % align == 0
        self.p = self.dev[off:]

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.off

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()

    def check(self, what, untouched=False):
        """The region's bytes, after asserting that the guards (untouched: and the region) hold what they held."""
        h = self.read()
        assert not bytes_outside_written(h, self.off, self.nbytes), f"{what}: {self.OUTSIDE}"
        if untouched:
            assert (h == BYTE).all(), f"{what}: {self.WRITTEN}"
        return h[self.off:self.off + self.nbytes]


WS_GUARD = 256                 # bytes behind (and, with an offset base, in front of) a workspace


class Workspace(ByteRegion):
    """`nbytes` bytes of 0x5A at `off` bytes from a 256-byte aligned base, WS_GUARD more behind them."""
    OUTSIDE, WRITTEN = "bytes outside the reported workspace size were written", "the workspace was written"

    def __init__(self, nbytes, off=0):
        ByteRegion.__init__(self, nbytes, off, WS_GUARD, 256)

    def flag(self):
        return int(self.read()[self.off:self.off + 4].view(np.int32)[0])


# ---------------------------------------------------------------------------------------------
# the margin report of a module: its slice of the session's MARGINS, appended to the session's report
# ---------------------------------------------------------------------------------------------
def margin_report_fixture(header, fmt="  {r:6.3f}  {w}", per_first_word=False):
    """The module-scoped autouse fixture.  header: the first line, `{n}` the number of comparisons.  Then every comparison, worst first; with
    per_first_word the worst comparison per first word of its name (the entry point or class: the header says which), then `worst first:`
    and the 25 worst."""
    import pytest

    @pytest.fixture(scope="module", autouse=True)
    def _margin_report():
        start = len(pl.MARGINS)
        yield
        mine = pl.MARGINS[start:]
        if not mine:
            return
        lines = [header.format(n=len(mine))]
        worst_first = sorted(mine, key=lambda t: -t[1])
        if not per_first_word:
            lines += [fmt.format(r=r, w=w) for w, r in worst_first]
        else:
            for word in sorted({w.split()[0] for w, _ in mine}):
                w, r = max(((w, r) for w, r in mine if w.split()[0] == word), key=lambda t: t[1])
                lines.append(fmt.format(r=r, w=w))
            lines.append("worst first:")
            lines += [fmt.format(r=r, w=w) for w, r in worst_first[:25]]
        pl.write_margin_report(lines)

    return _margin_report


# ---------------------------------------------------------------------------------------------
# the 16-bit types as bit patterns; ty: "f16" or "bf16"
# ---------------------------------------------------------------------------------------------
NAN16 = {"f16": 0x7E00, "bf16": 0x7FC0}       # a quiet NaN
INF16 = {"f16": 0x7C00, "bf16": 0x7F80}


def f32_of(bits, ty):
    """uint16 bit patterns -> their exact float32 values"""
    bits = np.asarray(bits, dtype=np.uint16)
    if ty == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def f64_of(bits, ty):
    return f32_of(bits, ty).astype(np.float64)


def rne16(x, ty):
    """float32 -> the 16-bit type, round to nearest even, as uint16 bit patterns (a NaN becomes a NaN)"""
    x = np.asarray(x, dtype=np.float32)
    if ty == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    b = x.view(np.uint32)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(NAN16["bf16"]), r)


def is_nan16(bits, ty):
    return (np.asarray(bits) & 0x7FFF) > INF16[ty]


# Two roundings of an fp64 result to the output type, NOT the same thing:
def round_bits(x, ty):
    """fp64 values that are EXACT in fp32 (the caller's premise, not checked), rounded once to nearest even: bf16 by torch's conversion
    from float32, f16 by numpy's from float64."""
    import torch
    if ty == "bf16":
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
    return np.ascontiguousarray(x).astype(np.float16).view(np.uint16)


def round_once(ref, ty):
    """The fp64 reference rounded ONCE to the output type, as bits.  bf16: through fp32, which must hold the value exactly -- ASSERTED here,
    where round_bits takes it on trust; f16 overflows to inf silently."""
    if ty == "f16":
        with np.errstate(over="ignore"):
            return ref.astype(np.float16).view(np.uint16)
    f = ref.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), ref)
    return rne16(f, ty)


# Two ways of letting +0 and -0 compare equal, NOT the same thing on a NaN:
def canon16(b):
    """16-bit patterns with -0 turned into +0, by pattern: a NaN keeps its payload."""
    return np.where(b == 0x8000, np.uint16(0), b)


def canon32(got_bits):
    """fp32 patterns with -0 turned into +0, by adding +0 in fp32: a signalling NaN comes out quiet."""
    return pl.bits(got_bits.view(np.float32) + np.float32(0.0))


def dev_bits(h, ty):
    """Bit patterns (uint16; "f32": uint32) -> a device tensor of the type."""
    import torch
    t = torch.from_numpy(h.view(SIGNED[h.itemsize]).copy()).cuda().view({"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[ty])
    assert t.data_ptr() % 16 == 0      # so that a base's alignment is its offset's
    return t


def host_bits(t):
    """A device tensor of 2- or 4-byte elements -> its bit patterns."""
    import torch
    torch.cuda.synchronize()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy().view(UNSIGNED[t.element_size()])
