"""Blocked-ELL on the 16-bit matrix cores, without a GPU: the four entry points are exported and declared, every argument-error and
size-limit status is returned before any device work, and batched::spmm instantiates for fp32 and the 16-bit element types."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sm_spmm_bell_f16", "sm_spmm_bell_bf16", "sm_spmm_bell_batched_f16", "sm_spmm_bell_batched_bf16"]
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
# stand-ins for device pointers: never dereferenced, the status is decided before any HIP call
P = ctypes.c_void_p(0x1000)


def test_symbols_exported_and_declared(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)


def _single(pkg, sfx, values=P, idx=P, rows=8, cols=8, bs=2, ell_cols=4, B=P, C=P, n=8):
    fn = getattr(pkg.lib(), "sm_spmm_bell_" + sfx)
    return fn(values, idx, rows, cols, bs, ell_cols, B, C, n, 1.0, 0.0, None)


def _batched(pkg, sfx, values=True, idx=True, rows=8, cols=8, bs=2, ell_cols=4, B=P, C=True, n=8, batch=3, null_at=None):
    Arr = ctypes.c_void_p * max(batch, 1)

    def table(present, which):
        if not present:
            return None
        return Arr(*[None if (null_at == (which, i)) else 0x1000 for i in range(max(batch, 1))])

    fn = getattr(pkg.lib(), "sm_spmm_bell_batched_" + sfx)
    return fn(table(values, "v"), table(idx, "i"), rows, cols, bs, ell_cols, B, table(C, "c"), n, batch, 1.0, 0.0, None)


@pytest.mark.parametrize("sfx", ["f16", "bf16"])
def test_single_statuses_without_a_device(pkg, sfx):
    for kw in (dict(values=None), dict(idx=None), dict(B=None), dict(C=None), dict(bs=0), dict(bs=3, ell_cols=4)):
        assert _single(pkg, sfx, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    for kw in (dict(rows=BIG), dict(cols=BIG), dict(n=BIG)):
        assert _single(pkg, sfx, **kw) == NOT_SUPPORTED, kw
    # nothing to do: success without touching the (fake) pointers
    assert _single(pkg, sfx, rows=0) == 0
    assert _single(pkg, sfx, n=0) == 0


@pytest.mark.parametrize("sfx", ["f16", "bf16"])
def test_batched_statuses_without_a_device(pkg, sfx):
    for kw in (dict(values=False), dict(idx=False), dict(C=False), dict(B=None), dict(bs=0), dict(bs=3, ell_cols=4),
               dict(null_at=("v", 2)), dict(null_at=("i", 0)), dict(null_at=("c", 1))):
        assert _batched(pkg, sfx, **kw) == INVALID, kw
    for kw in (dict(rows=BIG), dict(cols=BIG), dict(n=BIG)):
        assert _batched(pkg, sfx, **kw) == NOT_SUPPORTED, kw
    assert _batched(pkg, sfx, rows=0) == 0
    assert _batched(pkg, sfx, n=0) == 0
    assert _batched(pkg, sfx, batch=0) == 0


def test_batched_spmm_instantiates_for_every_element_type(tmp_path):
    src = tmp_path / "bell_types.cpp"
    src.write_text("""
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <sparsify.me/spmm.hxx>
using namespace sparsifyme;
template <typename T>
float call(ell_t<T, memory_space_t::device>* As, T* B, T** Cs) { return batched::spmm(As, B, Cs, 4, 4, 4, 1); }
template float call<float>(ell_t<float, memory_space_t::device>*, float*, float**);
template float call<__half>(ell_t<__half, memory_space_t::device>*, __half*, __half**);
template float call<_Float16>(ell_t<_Float16, memory_space_t::device>*, _Float16*, _Float16**);
template float call<__bf16>(ell_t<__bf16, memory_space_t::device>*, __bf16*, __bf16**);
template float call<__hip_bfloat16>(ell_t<__hip_bfloat16, memory_space_t::device>*, __hip_bfloat16*, __hip_bfloat16**);
// ell_t<__half> copies between memory spaces
void copy(ell_t<__half, memory_space_t::device>& d, const ell_t<__half, memory_space_t::host>& h) { d = h; }
""")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-c",
                          str(src), "-o", str(tmp_path / "bell_types.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
