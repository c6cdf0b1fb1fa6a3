"""Host-side checks of the wide dense-block entry (odil_dense_block_xty_wide): the header, the binding's list and the
built library name it, its workspace stays within the bound that csrc/dense_block.hip states, its arguments are
validated before anything touches the device, and the solver's column limit is the kernel's."""

import os
import re
from ctypes import c_int, c_int64, c_size_t, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["odil_dense_block_wide_workspace_bytes", "odil_dense_block_xty_wide_f64", "odil_dense_block_xty_wide_f32"]
BOUND = 64 << 20  # "64 MiB" in the header comment of csrc/dense_block.hip and in include/odil_hip.h


def test_wide_entry_is_declared_bound_and_exported():
    from odil_amd import _lib

    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b{}\s*\(".format(name), header), name
        assert name in _lib.EXPORTED, name
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_wide_workspace_stays_within_the_stated_bound():
    from odil_amd import _lib

    source = open(os.path.join(ROOT, "odil_amd", "csrc", "dense_block.hip")).read()
    assert "64 MiB" in source[:source.index("#include")]  # the bound is stated where the issue of memory is decided
    lib = _lib.load()
    size = lib.odil_dense_block_wide_workspace_bytes
    assert 0 < size(1024, 1024) <= BOUND
    for px, py in [(1, 1), (64, 65), (65, 65), (97, 98), (141, 142), (200, 1), (1, 1000), (1024, 1), (1000, 1023)]:
        assert 64 * 64 * 8 <= size(px, py) <= BOUND, (px, py)
    for px, py in [(0, 5), (5, 0), (1025, 5), (5, 1025), (-1, -1)]:
        assert size(px, py) == 0, (px, py)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_wide_entry_validates_on_the_host(suffix):
    """Column counts outside 1 .. 1024, row strides below the column counts, null pointers, n < 1 and a workspace that
    is too small are ODIL_E_INVAL before any launch (the pointers are dummies); the narrow entry keeps its 64."""
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_dense_block_xty_wide_" + suffix)
    x, y, out, ws = (c_void_p(16 * k) for k in range(1, 5))
    big = c_size_t(BOUND)

    def call(x=x, y=y, n=100, px=100, py=101, ldx=101, ldy=101, out=out, ws=ws, nbytes=big):
        return fn(x, y, c_int64(n), c_int(px), c_int(py), c_int64(ldx), c_int64(ldy), out, ws, nbytes, None)

    for kw in (dict(px=0), dict(py=0), dict(px=1025, ldx=1025), dict(py=1025, ldy=1025), dict(n=0), dict(ldx=99),
               dict(ldy=100), dict(x=None), dict(y=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -1, kw
        assert b"dense_block_xty_wide" in lib.odil_last_error(), kw
    assert call(nbytes=c_size_t(lib.odil_dense_block_wide_workspace_bytes(100, 101) - 8)) == -1
    assert b"workspace" in lib.odil_last_error()
    narrow = getattr(lib, "odil_dense_block_xty_" + suffix)
    assert narrow(x, y, c_int64(100), c_int(65), c_int(1), c_int64(65), c_int64(1), out, ws, None) == -1


def test_solver_limit_is_the_kernels():
    from odil_amd import linsolver, ops

    assert linsolver.DENSE_COLUMNS_MAX + 1 == ops.DENSE_WIDE_COLUMNS == 1024
