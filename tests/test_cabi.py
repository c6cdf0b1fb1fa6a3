"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every
symbol include/odil_hip.h declares (no compute without a GPU), argument validation
works on the host, and the product refuses CPU tensors instead of falling back."""

import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    return sorted(set(re.findall(r"\b(odil_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from odil_amd import _lib

    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 30
    for name in names:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTED) == names
    assert lib.odil_version() >= 100
    assert lib.odil_reduce_workspace_bytes() >= 4096 * 8


SNIPPET = """
/* A comment that names odil_fake(int x); declares nothing,
 * over however many lines. */
#ifdef __cplusplus
extern "C" {
#endif
// nor does int odil_fake2(void); here
const char* odil_text(void);
int odil_none();
#define ODIL_SOMETHING (-1) /* odil_fake3(int y); */
size_t odil_three_lines(double* const* x, const float* const* y,
                        const char* loc, char* buf, int32_t k,
                        size_t n, float a, double b, void* stream);
int64_t odil_count(const int64_t* shape, int *plan, int ndim, int64_t n);
#ifdef __cplusplus
}
#endif
"""


def test_declarations_of_a_snippet():
    from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

    from odil_amd import _lib

    found = _lib.declarations(SNIPPET)
    assert list(found) == ["odil_text", "odil_none", "odil_three_lines", "odil_count"]
    assert found == {
        "odil_text": (c_char_p, []),
        "odil_none": (c_int, []),
        "odil_three_lines": (c_size_t, [c_void_p, c_void_p, c_char_p, c_void_p, c_int32, c_size_t, c_float, c_double,
                                        c_void_p]),
        "odil_count": (c_int64, [c_void_p, c_void_p, c_int, c_int64]),
    }
    assert _lib.declarations("") == {} and _lib.declarations("/* int odil_fake(void); */\n#define X 1\n") == {}


@pytest.mark.parametrize("bad", [
    "int odil_bad(struct foo x);",
    "int odil_bad(const double* u, struct foo* x);",
    "int odil_bad(int);",  # a parameter without a name
    "int odil_bad(const int n);",
    "int odil_bad(char c);",
    "int odil_bad(void* const p);",
    "int odil_bad(double** x);",
    "int odil_bad(int (*f)(int));",
    "int odil_bad(int n, ...);",
    "void odil_bad(int n);",
    "double odil_bad(void);",
    "unsigned odil_bad(void);",
    "int other_bad(int n);",
    "struct odil_bad { int n; };",
    "typedef int odil_bad;",
    "int odil_bad(int n)",  # no semicolon
    "int odil_bad(int n); int odil_bad(int n);",  # declared twice
])
def test_declarations_refuse_what_they_do_not_understand(bad):
    """Nothing outside the header's subset of C is skipped: a declaration that is not understood must not become a
    function without argument types."""
    from odil_amd import _lib

    with pytest.raises(ValueError, match="bad"):
        _lib.declarations("int odil_good(int n);\n" + bad + "\n")


def test_a_missing_header_is_reported_by_load(monkeypatch, tmp_path):
    from odil_amd import _lib

    missing = str(tmp_path / "include" / "odil_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", missing)
    monkeypatch.setattr(_lib, "_declared", None)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.OdilHipError, match=re.escape(missing)):
        _lib.load()


def test_literal_signatures_of_six_entry_points():
    """Written out from include/odil_hip.h by hand, not by the parser: the two longest argument lists and one entry point
    of every other kind (host query, no parameters, no type suffix, float64 only)."""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_void_p

    from odil_amd import _lib

    P, I, L = c_void_p, c_int, c_int64
    expected = {
        "odil_stencil_solve_batch_f32": (I, [P, L, P, P, I, I, I, P, L, P, L, P, L, L, P, L, I, P, I, P, I, I, I, I, c_float,
                                             P, L, P, P]),
        "odil_poisson_small_epochs_batch_f64": (I, [P, P, P, P, P, P, P, I, L, L, P, I, I, P, P, L, I, c_double, c_double,
                                                    c_double, P, P, L, P, L, P]),
        "odil_tile_sched_units": (L, [L, L, L, I, L, I, P, L]),
        "odil_last_error": (c_char_p, []),
        "odil_narrow_scale": (I, [P, P, L, c_double, P, P]),
        "odil_bmg_coarse_chol_f64": (I, [P, L, L, c_double, P, P, P, P]),
    }
    assert len(expected["odil_stencil_solve_batch_f32"][1]) == 29
    assert len(expected["odil_poisson_small_epochs_batch_f64"][1]) == 26
    lib = _lib.load()
    for name, (restype, argtypes) in expected.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_every_exported_function_is_typed():
    """Every entry point carries argument types (an empty list, not None, where it has no parameters) and the header's
    return type; the return type and the number of parameters are read here by a regex of this test's own."""
    from ctypes import c_char_p, c_int, c_int64, c_size_t

    from odil_amd import _lib

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    returns = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "const char*": c_char_p}
    derived = _lib.declarations(open(os.path.join(ROOT, "include", "odil_hip.h")).read())
    assert sorted(derived) == sorted(_lib.EXPORTED) and len(_lib.EXPORTED) >= 159
    for name in _lib.EXPORTED:
        fn = getattr(lib, name)
        (returned, parameters), = re.findall(r"^((?:const )?\w+\*?) {}\(([^()]*)\);".format(name), text, flags=re.M)
        count = 0 if parameters.strip() in ("", "void") else parameters.count(",") + 1
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
        assert fn.restype is returns[returned], name
        assert (fn.restype, list(fn.argtypes)) == derived[name], name


# the parameters that are `double` in the _f64 AND the _f32 prototype: `denom` of the slab forms (a count of cells)
DOUBLE_IN_BOTH = {
    "odil_poisson_residual_slab": [8],
    "odil_poisson_residual_restrict_slab": [9],
    "odil_poisson_residual_synth": [8],
    "odil_stencil_var_residual_restrict_slab": [9],
}
F64_ONLY = ["odil_bmg_coarse_dense", "odil_bmg_coarse_chol"]


def test_f64_and_f32_twins_take_the_same_arguments():
    """The header's own two copies of every typed entry point: equal once c_double and c_float are exchanged."""
    from ctypes import c_double, c_float

    from odil_amd import _lib

    lib = _lib.load()
    swap = {c_double: c_float, c_float: c_double}
    bases = sorted({name[:-4] for name in _lib.EXPORTED if name.endswith(("_f64", "_f32"))})
    assert len(bases) >= 70 and set(DOUBLE_IN_BOTH) <= set(bases) and set(F64_ONLY) <= set(bases)
    for base in bases:
        assert base + "_f64" in _lib.EXPORTED, base
        if base in F64_ONLY:
            assert base + "_f32" not in _lib.EXPORTED, base
            continue
        wide, narrow = getattr(lib, base + "_f64"), getattr(lib, base + "_f32")
        assert wide.restype is narrow.restype, base
        kept = DOUBLE_IN_BOTH.get(base, [])
        assert [wide.argtypes[i] for i in kept] == [c_double] * len(kept), base
        exchanged = [a if i in kept else swap.get(a, a) for i, a in enumerate(wide.argtypes)]
        assert exchanged == list(narrow.argtypes), base


def test_host_side_validation_reports_errors():
    from ctypes import c_int, c_void_p

    from odil_amd import _lib

    lib = _lib.load()
    # invalid loc string -> ODIL_E_INVAL before anything touches the device
    status = lib.odil_interp_add_f64(
        c_void_p(16), None, c_void_p(16), _lib.i64([4, 4]), c_int(2), b"cx", 1.0, 1.0, None
    )
    assert status == -1
    assert b"loc" in lib.odil_last_error()
    status = lib.odil_poisson_adjoint_f64(c_void_p(16), c_void_p(16), _lib.i64([4] * 5), c_int(5), None, 1.0, None)
    assert status == -1


def test_bmg_host_side_validation():
    """odil_bmg_apply / odil_bmg_transfer reject malformed level descriptors, transfer codes, modes and aliasing with
    ODIL_E_INVAL before anything touches the device (the pointers are dummies)."""
    from ctypes import c_int, c_void_p

    from odil_amd import _lib

    lib = _lib.load()
    coef, table, x, b, dinv, y = (c_void_p(16 * k) for k in range(1, 7))

    def desc(nf, off, n, ebeg):
        return _lib.i64([nf] + off + [v for s in n for v in s] + ebeg)

    def apply(d, mode=0, x=x, y=y):
        return lib.odil_bmg_apply_f64(coef, table, d, x, b, dinv, y, c_int(mode), 0.5, None)

    def transfer(fd, cd, code, mode=0, src=x, out=y):
        codes = None if code is None else (c_int * len(code))(*code)
        return lib.odil_bmg_transfer_f64(fd, cd, codes, src, b, out, c_int(mode), None)

    good = ([0, 12, 15], [(1, 3, 4), (1, 1, 3)], [0, 2, 3])  # two fields, 12 + 3 unknowns, 3 table entries
    bad_desc = {
        "no fields": desc(0, [0], [], [0]),
        "nine fields": desc(9, list(range(10)), [(1, 1, 1)] * 9, [0] * 10),
        "empty extent": desc(2, [0, 0, 3], [(1, 0, 4), (1, 1, 3)], [0, 2, 3]),
        "offsets off the shapes": desc(2, [0, 12, 16], *good[1:]),
        "sizes off the shapes": desc(2, [0, 11, 14], *good[1:]),
        "ebeg decreasing": desc(2, good[0], good[1], [0, 2, 1]),
    }
    for what, d in bad_desc.items():
        for mode in range(4):
            assert apply(d, mode) == -1, (what, mode)
        assert b"bmg_apply" in lib.odil_last_error(), what
    ok = desc(2, *good)
    for mode in (-1, 4):
        assert apply(ok, mode) == -1, mode
    for mode in (0, 1, 2):
        assert apply(ok, mode, x=y) == -1, mode  # x aliasing y
    # transfers: fine (1, 3, 4) / (1, 1, 3) by codes (0, 0, 1) and (0, 0, 2) -> coarse (1, 3, 2) / (1, 1, 2)
    fine, coarse = desc(2, *good), desc(2, [0, 6, 8], [(1, 3, 2), (1, 1, 2)], [0, 2, 3])
    code = [0, 0, 1, 0, 0, 2]
    for what, d in bad_desc.items():
        assert transfer(d, coarse, code) == -1, what
        assert transfer(fine, d, code, mode=1) == -1, what
    for mode in (-1, 2):
        assert transfer(fine, coarse, code, mode) == -1, mode
    for mode in (0, 1):
        assert transfer(fine, coarse, code, mode, src=y, out=y) == -1, mode  # in aliasing out
    assert transfer(fine, coarse, None) == -1
    assert transfer(fine, desc(1, [0, 12], [(1, 3, 4)], [0, 2]), code[:3]) == -1  # field counts differ
    assert transfer(fine, coarse, [0, 0, 2, 0, 0, 2]) == -1  # code 2 on an even fine extent
    # code 1 on an odd fine extent: (1, 3, 4) -> (1, 1, 4) along axis 1
    odd = desc(2, [0, 4, 7], [(1, 1, 4), (1, 1, 3)], [0, 2, 3])
    assert transfer(fine, odd, [0, 1, 0, 0, 0, 0]) == -1
    # code 2 with coarse extent 1 (fine extent 1)
    one = desc(2, [0, 12, 13], [(1, 3, 4), (1, 1, 1)], [0, 2, 3])
    assert transfer(one, one, [0, 0, 0, 0, 0, 2]) == -1
    assert b"transfer code" in lib.odil_last_error()
    # code 0 on an axis whose extent changes
    assert transfer(fine, coarse, [0, 0, 0, 0, 0, 2]) == -1


def test_stencil_host_side_validation():
    """odil_stencil_apply / _csr_assemble / _stencil_march and the solver reductions refuse malformed shift lists,
    extents, diagonal slots, axes, directions, sizes and null pointers with ODIL_E_INVAL before anything touches the
    device (the pointers are dummies)."""
    from ctypes import c_double, c_int, c_int64, c_void_p

    from odil_amd import _lib

    lib = _lib.load()
    coeffs, x, y, w = (c_void_p(16 * k) for k in range(1, 5))
    shape = [4, 5]
    good = [(0, 0), (-1, 0), (-2, 1)]  # diagonal, then two shifts pointing back along axis 0

    def flat(shifts):
        return _lib.i64([v for s in shifts for v in s] or [0])

    for fn in (lib.odil_stencil_apply_f64, lib.odil_stencil_apply_f32):
        def apply(shifts=good, nshift=None, shp=shape, ndim=None, c=coeffs, xx=x, yy=y, shifts_ptr=True):
            nshift = len(shifts) if nshift is None else nshift
            ndim = len(shp) if ndim is None else ndim
            return fn(c, flat(shifts) if shifts_ptr else None, c_int(nshift), xx, yy, _lib.i64(shp or [1]),
                      c_int(ndim), c_int(0), None)

        assert apply(nshift=0) == -1
        assert apply([(0, 0)] * 33) == -1
        assert apply(shifts_ptr=False) == -1
        assert apply(shp=[4, 0]) == -1 and b"extent" in lib.odil_last_error()
        assert apply([(0,)], shp=[], ndim=0) == -1
        assert apply([(0,) * 5], shp=[2] * 5) == -1
        for c, xx, yy in ((None, x, y), (coeffs, None, y), (coeffs, x, None)):
            assert apply(c=c, xx=xx, yy=yy) == -1
            assert b"null pointer" in lib.odil_last_error()

    for fn in (lib.odil_csr_assemble_f64, lib.odil_csr_assemble_f32):
        def assemble(shifts=good, nshift=None, shp=shape, ptrs=(coeffs, x, y, w)):
            nshift = len(shifts) if nshift is None else nshift
            c, indptr, indices, data = ptrs
            return fn(c, flat(shifts), c_int(nshift), _lib.i64(shp), c_int(len(shp)), c_int64(3 << 31), indptr,
                      indices, data, None)

        assert assemble(nshift=0) == -1
        assert assemble([(0, 0)] * 33) == -1
        assert assemble(shp=[0, 5]) == -1
        for k in range(4):
            ptrs = [coeffs, x, y, w]
            ptrs[k] = None
            assert assemble(ptrs=ptrs) == -1, k

    for fn in (lib.odil_stencil_march_f64, lib.odil_stencil_march_f32):
        def march(shifts=good, diag=0, axis=0, direction=1, nshift=None, shp=shape, c=coeffs, b=x, out=y):
            nshift = len(shifts) if nshift is None else nshift
            return fn(c, flat(shifts), c_int(nshift), c_int(diag), b, out, _lib.i64(shp), c_int(len(shp)),
                      c_int(axis), c_int(direction), None)

        assert march(nshift=0) == -1
        assert march([(0, 0)] + [(-1, 0)] * 32) == -1
        for diag in (-1, 3):
            assert march(diag=diag) == -1, diag
        assert march(diag=1) == -1 and b"not the diagonal" in lib.odil_last_error()
        for axis in (-1, 2):
            assert march(axis=axis) == -1, axis
        assert march(direction=0) == -1
        for c, b, out in ((None, x, y), (coeffs, None, y), (coeffs, x, None)):
            assert march(c=c, b=b, out=out) == -1
        # neighbours that are not in an earlier level: same level, the wrong direction, a whole period back
        for bad in ((0, 1), (1, 0), (-4, 0)):
            assert march([(0, 0), (-1, 0), bad]) == -1, bad
            assert b"earlier level" in lib.odil_last_error()
        assert march(direction=-1) == -1  # the good shifts point forward
        assert march([(0, 0), (-1, 0)], axis=1) == -1  # no component along axis 1

    part, out = c_void_p(64), c_void_p(128)
    for n in (0, -1):
        assert lib.odil_lbfgs_probe_f64(x, y, c_int64(n), part, out, None) == -1
        assert lib.odil_lbfgs_probe_f32(x, y, c_int64(n), part, out, None) == -1
        assert lib.odil_max_abs_diff_f64(x, y, c_int64(n), part, out, None) == -1
        assert lib.odil_max_abs_diff_f32(x, y, c_int64(n), part, out, None) == -1
    assert lib.odil_lbfgs_probe_f64(None, y, c_int64(8), part, out, None) == -1
    assert lib.odil_max_abs_diff_f64(x, None, c_int64(8), part, out, None) == -1
    assert lib.odil_narrow_scale(x, None, c_int64(8), c_double(1.0), None, None) == -1
    assert lib.odil_widen_axpy(x, y, c_int64(-1), c_double(1.0), None, None) == -1


def test_no_cpu_fallback():
    from odil_amd import _lib, ops

    with pytest.raises(_lib.OdilHipError):
        ops.interp_add(torch.zeros(4, 4, dtype=torch.float64), "cc")
    with pytest.raises(_lib.OdilHipError):
        ops.adam_step(*[torch.zeros(8) for _ in range(4)], 0.1, 0.1, 0.001, 1e-7)
