"""Fixed and tied parameters of a curve fit: the parameter map.

A model with n parameters is fitted over ``nf <= n`` solver variables through an integer map ``pmap`` (n,) and a
per-problem template ``Pfix`` (..., n):

    P_full[..., j]  = X[..., pmap[j]]     if pmap[j] >= 0
                    = Pfix[..., j]        if pmap[j] == -1        (a fixed parameter)
    f_map           = f(P_full)
    J_map[..., k]   = sum over {j : pmap[j] == k}, in ascending j, of J_full[..., j]          k = 0 .. nf - 1

The first column of a slot is taken as it is and the later ones are added to it one by one: a sequential float64 sum.
Columns of fixed parameters are dropped.  The functions of ``ParamMap`` below ARE this definition, in the way
``_models.py`` is the definition of the formulas: the mapped kernel instances (csrc/model_kernels.hip,
blsq_model_eval_map_dev) compute the same numbers bit for bit.

A tie ``{j: i}`` makes p_j a copy of p_i.  The parameter i that a group follows is its *leader*: it is neither fixed
nor itself tied, its value is the group's solver variable and its ``p0`` is the group's start.  Slots are numbered in
ascending order of the leaders.  Needs neither the library nor a GPU.
"""
import numpy as np

__all__ = ['ParamMap']


class ParamMap:
    """The map of n model parameters onto nf solver variables.

    fixed : None, a boolean mask (n,) or a sequence of indices: parameters held at their template value
    tied  : None or a dict ``{j: i}``: p_j is p_i.  i must be free (not fixed, not a key of `tied`), j != i.
    ValueError (naming the index) for an index outside 0 .. n - 1, a key or target of `tied` that is fixed, a target
    that is itself a key, j == i, and a map that leaves nothing to fit.

    Attributes: ``n``, ``nf``, ``pmap`` (n,) int32 (-1: fixed, else the slot), ``leaders`` (nf,) (the parameter whose
    value is solver variable k), ``fixed`` (n,) bool, ``tied`` (the dict), ``identity`` (nothing fixed, nothing tied).
    """

    def __init__(self, n, fixed=None, tied=None):
        n = int(n)
        if n < 1:
            raise ValueError("`n` must be positive.")
        fx = np.zeros(n, dtype=bool)
        if fixed is not None:
            a = np.asarray(fixed)
            if a.dtype == bool:
                if a.shape != (n,):
                    raise ValueError("a boolean `fixed` must have shape (n,) = (%d,), not %s." % (n, a.shape))
                fx = a.copy()
            else:
                for j in np.atleast_1d(a).ravel().tolist() if a.size else []:
                    if int(j) != j or not 0 <= int(j) < n:
                        raise ValueError("`fixed` index %r is outside 0 .. %d." % (j, n - 1))
                    fx[int(j)] = True
        td = {}
        for j, i in (dict(tied) if tied else {}).items():
            for what, v in (("key", j), ("target", i)):
                if int(v) != v or not 0 <= int(v) < n:
                    raise ValueError("`tied` %s %r is outside 0 .. %d." % (what, v, n - 1))
            td[int(j)] = int(i)
        for j, i in td.items():
            if j == i:
                raise ValueError("`tied` ties parameter %d to itself." % j)
            if fx[j]:
                raise ValueError("`tied` key %d is also fixed." % j)
            if fx[i]:
                raise ValueError("`tied` target %d (of parameter %d) is fixed." % (i, j))
            if i in td:
                raise ValueError("`tied` target %d (of parameter %d) is itself tied to %d." % (i, j, td[i]))
        leaders = [j for j in range(n) if not fx[j] and j not in td]
        if not leaders:
            raise ValueError("every parameter is fixed: nothing is left to fit (nf = 0).")
        slot = {j: k for k, j in enumerate(leaders)}
        pmap = np.full(n, -1, dtype=np.int32)
        for j in range(n):
            if not fx[j]:
                pmap[j] = slot[td.get(j, j)]
        self.n, self.nf = n, len(leaders)
        self.pmap = pmap
        self.leaders = np.asarray(leaders, dtype=np.intp)
        self.fixed = fx
        self.tied = td
        self.identity = self.nf == n
        self._free = np.flatnonzero(pmap >= 0)

    def __repr__(self):
        return "ParamMap(n=%d, nf=%d, pmap=%s)" % (self.n, self.nf, self.pmap.tolist())

    def _last(self, a, width, name):
        a = np.asarray(a)
        if a.ndim < 1 or a.shape[-1] != width:
            raise ValueError("`%s` must have %d entries along its last axis, not shape %s." % (name, width, a.shape))
        return a

    def group(self, k):
        """The members of slot k, ascending."""
        return np.flatnonzero(self.pmap == k)

    def reduce_x(self, P):
        """(..., n) -> (..., nf): the leaders' columns."""
        return self._last(P, self.n, "P")[..., self.leaders]

    def expand_x(self, X, Pfix):
        """(..., nf) and the template (..., n) -> (..., n): copies only.  Of `Pfix` the fixed columns are read."""
        X = self._last(X, self.nf, "X")
        Pfix = self._last(Pfix, self.n, "Pfix")
        out = np.empty(np.broadcast_shapes(X.shape[:-1], Pfix.shape[:-1]) + (self.n,),
                       dtype=np.result_type(X.dtype, Pfix.dtype))
        out[...] = Pfix
        out[..., self._free] = X[..., self.pmap[self._free]]
        return out

    def reduce_jac(self, J_full):
        """(..., m, n) -> (..., m, nf): per slot the sequential sum of its columns in ascending j."""
        J_full = self._last(J_full, self.n, "J_full")
        out = np.empty(J_full.shape[:-1] + (self.nf,), dtype=J_full.dtype)
        started = np.zeros(self.nf, dtype=bool)
        for j in range(self.n):
            k = self.pmap[j]
            if k < 0:
                continue
            if started[k]:
                out[..., k] = out[..., k] + J_full[..., j]
            else:
                out[..., k] = J_full[..., j]
                started[k] = True
        return out

    def reduce_bounds(self, lb, ub):
        """(..., n) bounds -> (..., nf): the box of a slot is the intersection of its members' boxes; bounds of fixed
        parameters are ignored.  ValueError naming the group where the intersection is empty."""
        lb = self._last(lb, self.n, "lb").astype(float)
        ub = self._last(ub, self.n, "ub").astype(float)
        lo = np.empty(lb.shape[:-1] + (self.nf,))
        hi = np.empty(ub.shape[:-1] + (self.nf,))
        for k in range(self.nf):
            g = self.group(k)
            lo[..., k] = np.max(lb[..., g], axis=-1)
            hi[..., k] = np.min(ub[..., g], axis=-1)
        lo_b, hi_b = np.broadcast_arrays(lo, hi)
        if np.any(lo_b > hi_b):
            k = int(np.argwhere(lo_b > hi_b)[0][-1])
            raise ValueError("the bounds of the tied parameters %s do not intersect." % self.group(k).tolist())
        return lo, hi

    def expand_cov(self, C):
        """(..., nf, nf) -> (..., n, n) = T C T^T with T the 0/1 matrix of the map: zero rows and columns for fixed
        parameters, copies for tied ones.  No arithmetic."""
        C = self._last(C, self.nf, "C")
        if C.ndim < 2 or C.shape[-2] != self.nf:
            raise ValueError("`C` must have shape (..., nf, nf).")
        out = np.zeros(C.shape[:-2] + (self.n, self.n), dtype=C.dtype)
        s = self.pmap[self._free]
        out[..., self._free[:, None], self._free[None, :]] = C[..., s[:, None], s[None, :]]
        return out

    def expand_mask(self, mask):
        """active_mask (..., nf) -> (..., n): 0 for a fixed parameter, the leader's value for a tied one."""
        mask = self._last(mask, self.nf, "mask")
        out = np.zeros(mask.shape[:-1] + (self.n,), dtype=mask.dtype)
        out[..., self._free] = mask[..., self.pmap[self._free]]
        return out

    def matrix(self):
        """T (n, nf): T[j, pmap[j]] = 1."""
        T = np.zeros((self.n, self.nf))
        T[self._free, self.pmap[self._free]] = 1.0
        return T

    # ---- numpy callables over the solver's variables -------------------------------------------------------------
    def wrap_f(self, f, Pfix):
        """``f(xdata, P)`` over all n parameters -> ``g(xdata, X)`` over the nf variables."""
        return lambda xdata, X: f(xdata, self.expand_x(X, Pfix))

    def wrap_jac(self, jac, Pfix):
        """``jac(xdata, P) -> (..., m, n)`` -> ``g(xdata, X) -> (..., m, nf)``."""
        return lambda xdata, X: self.reduce_jac(np.asarray(jac(xdata, self.expand_x(X, Pfix))))
