"""What the GPU tests of the model-eval entries (include/blsq.h, blsq_model_eval*_dev) share: the context fixture, device
copies, the call of an entry by argument NAME through ``_abi.MODEL_EVAL_ARGS``, the count of the entries a fit reaches,
and the comparison of two fits.  Not collected as a test."""
import numpy as np
import pytest

from bounded_lsq import _abi, models

DEVICE_INPUTS = ("t", "y", "w", "X", "Pfix", "mask")


@pytest.fixture(scope="module")
def ctx():
    c = _abi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    """Two arrays of one shape and type with every bit equal (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Dev:
    """Device copies of a test's arrays, freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        if a is None:
            return None
        p = self.ctx.to_device(np.ascontiguousarray(a))
        self.ptrs.append(p)
        return p

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _host(a, dtype, ptr_type):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(ptr_type)


def i32(a):
    """-> (the int32 array, its pointer); the array must outlive the pointer's use."""
    return _host(a, np.int32, _abi.c_int32_p)


def f64(a):
    return _host(a, np.float64, _abi.c_double_p)


# the arguments that are host pointers, read during the call: name -> i32 or f64
HOST_TABLES = {k: (f64 if t is _abi.c_double_p else i32) for k, t in _abi.MODEL_EVAL_TYPES.items()
               if t in (_abi.c_int32_p, _abi.c_double_p)}


def call(ctx, entry, strict=False, **named):
    """`entry` with its arguments by name (``_abi.MODEL_EVAL_ARGS``) -> the return code.  Every value is passed as it
    is, consistent or not; a host table (fam, cnt, shared, pmap, tie_ratio, tie_offset) given as a sequence or an array
    becomes a pointer to a copy that lives until the entry returns.  strict=False: the names `entry` does not take are
    dropped, which is how a test calls an older entry with the same arguments less the new ones."""
    held = []
    for k, v in named.items():
        if k in HOST_TABLES and isinstance(v, (list, tuple, np.ndarray)):
            held.append(HOST_TABLES[k](v))
            named[k] = held[-1][1]
    return getattr(ctx.lib, entry)(ctx.h, *_abi.model_eval_args(entry, named, strict))


def run(ctx, entry, f_shape, J_shape, want_f=True, want_J=False, fill=np.nan, dev=None, strict=False, **named):
    """``call`` on host arrays -> (rc, f or None, J or None), and (rc, None, None) for rc != 0.  t, y, w, X, Pfix and
    mask (int32) given as arrays are uploaded; a device pointer or None goes through.  f and J are allocated in their
    shapes filled with `fill` where wanted, NULL otherwise.  Everything uploaded here is freed; `dev`: a ``Dev`` of the
    caller's to upload into instead, which the caller closes."""
    d = Dev(ctx) if dev is None else dev
    try:
        for k in DEVICE_INPUTS:
            if isinstance(named.get(k), (list, tuple, np.ndarray)):
                named[k] = d.up(np.asarray(named[k], dtype=np.int32) if k == "mask" else named[k])
        named["f"] = d.up(np.full(f_shape, fill)) if want_f else None
        named["J"] = d.up(np.full(J_shape, fill)) if want_J else None
        rc = call(ctx, entry, strict, **named)
        if rc != 0:
            return rc, None, None
        return (0, ctx.to_host(named["f"], f_shape, np.float64) if want_f else None,
                ctx.to_host(named["J"], J_shape, np.float64) if want_J else None)
    finally:
        if dev is None:
            d.close()


def model_args(M):
    """model, ncomp, fam, cnt of a named model or a ``CompositeModel``, by name."""
    if isinstance(M, models.CompositeModel):
        return dict(model=-1, ncomp=len(M.components), fam=M.fam_ids, cnt=M.counts)
    return dict(model=M.id, ncomp=0, fam=None, cnt=None)


def w_stride(w, m):
    """The stride of weights given per problem (2-D), 0 for shared ones and for None."""
    return m if (w is not None and np.ndim(w) == 2) else 0


class Counting:
    """``ctx.lib`` with the calls of its blsq_model_eval* entries counted by name in ``counts`` (`names`: only those,
    each from 0)."""

    def __init__(self, lib, names=None):
        self._lib, self._all, self.counts = lib, names is None, dict.fromkeys(names or (), 0)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in self.counts or (self._all and name.startswith("blsq_model_eval")):
            def counted(*a):
                self.counts[name] = self.counts.get(name, 0) + 1
                return fn(*a)
            return counted
        return fn


def count_entries(ctx, monkeypatch, names=None):
    """Put a ``Counting`` in the place of ``ctx.lib`` for the rest of the test -> its ``counts``."""
    proxy = Counting(ctx.lib, names)
    monkeypatch.setattr(ctx, "lib", proxy)
    return proxy.counts


def normalised(pcov, free):
    C = pcov[:, free][:, :, free]
    d = np.sqrt(np.einsum("bii->bi", C))
    return C / (d[:, :, None] * d[:, None, :])


def agree(a, b, what, rtol_p=1e-6, atol_p=1e-9):
    """Two fits (popt, pcov, ...) of one problem: popt to rtol 1e-6 / atol 1e-9 and the normalised pcov to 1e-6, over
    the free parameters (those whose variance in `a` is positive in every problem)."""
    free = np.flatnonzero(np.all(np.einsum("bii->bi", a[1]) > 0, axis=0))
    np.testing.assert_allclose(b[0], a[0], rtol=rtol_p, atol=atol_p, err_msg=str(what))
    np.testing.assert_allclose(normalised(b[1], free), normalised(a[1], free), rtol=0, atol=1e-6, err_msg=str(what))
