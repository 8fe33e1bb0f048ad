"""Host side of GMRES on a block of right-hand sides (spal_*_gmres_block_*): the entry points exist, null
arguments answer before anything else, restart and the block's geometry are checked before a handle is looked at, the
Python refusals fire before a device copy is made, and nothing falls back to the CPU.  None of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

# spal_{csr,csc}_gmres_block_{f64,f32} and spal_{csr,csc}_gmres_block_dev_{f64,f32}
NAMES = [f"spal_{fmt}_gmres_block_{form}{sfx}" for fmt in ("csr", "csc") for form in ("", "dev_") for sfx in ("f64", "f32")]


def test_the_entry_points_are_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    assert len(NAMES) == len(set(NAMES)) == 8
    for n in NAMES:
        assert n in names
        assert hasattr(lib, n)


def _args(name, handle, k=1, ldb=1, ldx=1, restart=5, b=True, x=True, info=True):
    u, buf = C.c_uint64, (C.c_double * 8)()
    infos = (sp.matrix._KrylovInfoC * 2)()
    args = [handle, None, u(k), buf if b else None, u(ldb)]                                   # a, m, k, b, ldb
    if "_dev_" in name:
        args += [buf if x else None, u(ldx), u(restart), C.c_double(1e-8), u(5), None]         # x, ldx, restart, tol, maxit, stream
    else:
        args += [u(4), buf if x else None, u(ldx), u(4), u(restart), C.c_double(1e-8), u(5)]   # b_rows, x, ldx, x_rows, ...
    return args + [infos if info else None]


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_invalid(name):
    lib = _ffi.lib()
    fn = getattr(lib, name)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)      # never looked at: the null check comes first
    prefix = name.split("_gmres_block")[0].encode() + b"_gmres_block: null argument"
    for kw in (dict(handle=None), dict(handle=fake, b=False), dict(handle=fake, x=False), dict(handle=fake, info=False)):
        handle = kw.pop("handle")
        assert fn(*_args(name, handle, **kw)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert lib.spal_last_error().startswith(prefix), lib.spal_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_restart_and_the_geometry_are_checked_before_the_handle_is_looked_at(name):
    """restart outside 1 .. 256, k == 0 and ld < k need nothing of the handle: a block of zeros stands in for one"""
    lib = _ffi.lib()
    fn = getattr(lib, name)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    prefix = name.split("_gmres_block")[0].encode() + b"_gmres_block: "
    for kw, text in ((dict(k=0), b"k = 0"), (dict(k=3, ldb=2, ldx=3), b"ldb = 2 is less than k = 3"),
                     (dict(k=3, ldb=3, ldx=1), b"ldx = 1 is less than k = 3"),
                     (dict(restart=0), b"restart = 0 must be 1 .. 256"), (dict(restart=257), b"restart = 257 must be 1 .. 256"),
                     (dict(k=1 << 32, ldb=1 << 32, ldx=1 << 32), b"does not fit 32 bits")):
        assert fn(*_args(name, fake, **kw)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        msg = lib.spal_last_error()
        assert msg.startswith(prefix) and text in msg, msg


def test_krylov_tile_three_is_refused():
    """the option's value is judged before the handle is touched"""
    lib = _ffi.lib()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    for bad in (3, -1, 64):
        assert lib.spal_csr_set_option(fake, b"krylov_tile", C.c_int64(bad)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert b"krylov_tile must be 0 (automatic) or one of 1, 2, 4, 8, 16, 32" in lib.spal_last_error()


@pytest.mark.parametrize("cls", [sp.CsrMatrix, sp.CscMatrix])
def test_bad_shapes_panic_before_the_device(cls):
    sq = cls(3, 3, [0, 1, 2, 3], [0, 1, 2], np.array([1.0, 2.0, 4.0]))
    with pytest.raises(sp.Panic, match=r"gmres_block: B has shape \(3,\)"):
        sq.gmres_block(np.ones(3))
    with pytest.raises(sp.Panic, match=r"B has shape \(4, 2\) but the matrix has 3 rows"):
        sq.gmres_block(np.ones((4, 2)))
    with pytest.raises(sp.Panic, match=r"B has shape \(3, 2, 2\)"):
        sq.gmres_block(np.ones((3, 2, 2)))
    with pytest.raises(sp.Panic, match=r"X0 has shape \(3, 3\) but B \(3, 2\)"):
        sq.gmres_block(np.ones((3, 2)), X0=np.ones((3, 3)))
    with pytest.raises(sp.Panic, match=r"X0 has shape \(3,\)"):
        sq.gmres_block(np.ones((3, 2)), X0=np.ones(3))
    for bad in (0, 257, -1):
        with pytest.raises(sp.Panic, match=rf"gmres_block: restart = {bad} must be 1 \.\. 256"):
            sq.gmres_block(np.ones((3, 2)), restart=bad)
    with pytest.raises(TypeError, match="precond_sweeps needs M"):
        sq.gmres_block(np.ones((3, 2)), precond_sweeps=2)
    assert not sq._dev             # no device copy was made
    # gmres itself keeps its one 1-D right-hand side: a block is refused there as it always was
    with pytest.raises(sp.Panic, match=r"gmres: b has shape \(3, 2\)"):
        sq.gmres(np.ones((3, 2)))
    assert not sq._dev
    ptr = [0, 1, 2] if cls is sp.CsrMatrix else [0, 1, 1, 2]
    rect = cls(2, 3, ptr, [0, 1] if cls is sp.CscMatrix else [0, 2], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"gmres_block: the matrix is not square \(2 x 3\)"):
        rect.gmres_block(np.ones((2, 4)))
    assert not rect._dev


def test_no_cpu_fallback_for_a_block():
    if sp.device_count() > 0:
        pytest.skip("a GPU is present: the no-device error path cannot be exercised")
    a = sp.CsrMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.array([1.0, 2.0, 4.0]))
    with pytest.raises(sp.SpalError) as e:
        a.gmres_block(np.ones((3, 2)))
    assert e.value.status == _ffi.SPAL_ERR_NO_DEVICE
