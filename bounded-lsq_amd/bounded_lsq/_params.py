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

Affine ties.  A tie ``{j: (i, ratio)}`` or ``{j: (i, ratio, offset)}`` makes
p_j = ratio * p_i + offset, with `ratio` (default 1, not 0) and `offset` (default 0) Python floats shared by all
problems.  With ratio[j] and offset[j] the pair of parameter j ((1, 0) for a leader, a fixed parameter and a plain tie):

    P_full[..., j]  = ratio[j] * X[..., pmap[j]] + offset[j]     the product first, then the sum; where the pair is
                                                                 (1, 0) the plain copy above (so -0.0 stays -0.0)
    J_map[..., k]   = sum over {j : pmap[j] == k}, in ascending j, of ratio[j] * J_full[..., j]

The first column of a slot is taken as it is after its multiply; a key below its leader arrives first and carries its
ratio.  The affine kernel instances (blsq_model_eval_tie_dev) compute these numbers bit for bit.
"""
import numpy as np

__all__ = ['ParamMap', 'GlobalMap']


class ParamMap:
    """The map of n model parameters onto nf solver variables.

    fixed : None, a boolean mask (n,) or a sequence of indices: parameters held at their template value
    tied  : None or a dict ``{j: i}``: p_j is p_i.  i must be free (not fixed, not a key of `tied`), j != i.  A value
            may also be a tuple ``(i, ratio)`` or ``(i, ratio, offset)`` (``(i,)`` is ``i``): p_j = ratio * p_i + offset.
    ValueError (naming the index) for an index outside 0 .. n - 1, a key or target of `tied` that is fixed, a target
    that is itself a key, j == i, and a map that leaves nothing to fit; (naming the key) for a ratio that is 0 or not
    finite, an offset that is not finite and a tuple of the wrong length.

    Attributes: ``n``, ``nf``, ``pmap`` (n,) int32 (-1: fixed, else the slot), ``leaders`` (nf,) (the parameter whose
    value is solver variable k), ``fixed`` (n,) bool, ``tied`` (the dict ``{j: i}`` of ints, whatever form the values
    had), ``identity`` (nothing fixed, nothing tied), ``ratio`` (n,) and ``offset`` (n,) float64 (1 and 0 for leaders,
    fixed parameters and plain ties), ``affine`` (some pair differs from (1, 0)).
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
        td, pairs = {}, {}
        for j, i in (dict(tied) if tied else {}).items():
            r, d = 1.0, 0.0
            if isinstance(i, (tuple, list)):
                if not 1 <= len(i) <= 3:
                    raise ValueError("`tied` value of key %r must be i, (i, ratio) or (i, ratio, offset), not %d "
                                     "entries." % (j, len(i)))
                i, r, d = (tuple(i) + (1.0, 0.0)[len(i) - 1:])
            for what, v in (("key", j), ("target", i)):
                if int(v) != v or not 0 <= int(v) < n:
                    raise ValueError("`tied` %s %r is outside 0 .. %d." % (what, v, n - 1))
            r, d = float(r), float(d)
            if r == 0.0 or not np.isfinite(r):
                raise ValueError("`tied` ratio %r of key %d must be finite and not 0." % (r, int(j)))
            if not np.isfinite(d):
                raise ValueError("`tied` offset %r of key %d must be finite." % (d, int(j)))
            td[int(j)] = int(i)
            pairs[int(j)] = (r, d)
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
        self.ratio, self.offset = np.ones(n), np.zeros(n)
        for j, (r, d) in pairs.items():
            self.ratio[j], self.offset[j] = r, d
        self._aff = np.flatnonzero((self.ratio != 1.0) | (self.offset != 0.0))  # the members that are no plain copy
        self.affine = bool(self._aff.size)

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
        """(..., nf) and the template (..., n) -> (..., n): copies, and for a member whose (ratio, offset) is not (1, 0)
        ``ratio * X[..., k] + offset``, the product first.  Of `Pfix` the fixed columns are read."""
        X = self._last(X, self.nf, "X")
        Pfix = self._last(Pfix, self.n, "Pfix")
        out = np.empty(np.broadcast_shapes(X.shape[:-1], Pfix.shape[:-1]) + (self.n,),
                       dtype=np.result_type(X.dtype, Pfix.dtype))
        out[...] = Pfix
        out[..., self._free] = X[..., self.pmap[self._free]]
        if self.affine:
            a = self._aff
            out[..., a] = self.ratio[a] * X[..., self.pmap[a]] + self.offset[a]
        return out

    def reduce_jac(self, J_full):
        """(..., m, n) -> (..., m, nf): per slot the sequential sum, in ascending j, of ``ratio[j]`` times column j (a
        column whose ratio is 1 is taken as it is)."""
        J_full = self._last(J_full, self.n, "J_full")
        out = np.empty(J_full.shape[:-1] + (self.nf,), dtype=J_full.dtype)
        started = np.zeros(self.nf, dtype=bool)
        for j in range(self.n):
            k = self.pmap[j]
            if k < 0:
                continue
            col = J_full[..., j] if self.ratio[j] == 1.0 else self.ratio[j] * J_full[..., j]
            if started[k]:
                out[..., k] = out[..., k] + col
            else:
                out[..., k] = col
                started[k] = True
        return out

    def reduce_bounds(self, lb, ub):
        """(..., n) bounds -> (..., nf): the box of a slot is the intersection of its members' boxes; bounds of fixed
        parameters are ignored.  A member with (ratio r, offset d) constrains the slot to [(lb - d) / r, (ub - d) / r],
        the ends swapped for r < 0.  ValueError naming the group where the intersection is empty."""
        lb = self._last(lb, self.n, "lb").astype(float)
        ub = self._last(ub, self.n, "ub").astype(float)
        if self.affine:
            lb, ub = np.broadcast_arrays(lb, ub)
            lb, ub = lb.copy(), ub.copy()
            for j in self._aff:
                lo_j, hi_j = (lb[..., j] - self.offset[j]) / self.ratio[j], (ub[..., j] - self.offset[j]) / self.ratio[j]
                lb[..., j], ub[..., j] = (lo_j, hi_j) if self.ratio[j] > 0 else (hi_j, lo_j)
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
        """(..., nf, nf) -> (..., n, n) = T C T^T with T the matrix of the map (``matrix()``): zero rows and columns for
        fixed parameters, ``ratio[j] * ratio[l] * C[k_j, k_l]`` for tied ones.  Without affine ties: copies, no
        arithmetic."""
        C = self._last(C, self.nf, "C")
        if C.ndim < 2 or C.shape[-2] != self.nf:
            raise ValueError("`C` must have shape (..., nf, nf).")
        out = np.zeros(C.shape[:-2] + (self.n, self.n), dtype=C.dtype)
        s = self.pmap[self._free]
        out[..., self._free[:, None], self._free[None, :]] = C[..., s[:, None], s[None, :]]
        if self.affine:
            out = (self.ratio[:, None] * self.ratio[None, :]) * out
        return out

    def expand_mask(self, mask):
        """active_mask (..., nf) -> (..., n): 0 for a fixed parameter, the leader's value for a tied one, times the sign
        of its ratio (under a negative ratio the member sits on its other bound)."""
        mask = self._last(mask, self.nf, "mask")
        out = np.zeros(mask.shape[:-1] + (self.n,), dtype=mask.dtype)
        out[..., self._free] = mask[..., self.pmap[self._free]]
        if self.affine:
            neg = np.flatnonzero(self.ratio < 0)
            out[..., neg] = -out[..., neg]
        return out

    def matrix(self):
        """T (n, nf): T[j, pmap[j]] = ratio[j] (1 without affine ties)."""
        T = np.zeros((self.n, self.nf))
        T[self._free, self.pmap[self._free]] = self.ratio[self._free]
        return T

    # ---- numpy callables over the solver's variables -------------------------------------------------------------
    def wrap_f(self, f, Pfix):
        """``f(xdata, P)`` over all n parameters -> ``g(xdata, X)`` over the nf variables."""
        return lambda xdata, X: f(xdata, self.expand_x(X, Pfix))

    def wrap_jac(self, jac, Pfix):
        """``jac(xdata, P) -> (..., m, n)`` -> ``g(xdata, X) -> (..., m, nf)``."""
        return lambda xdata, X: self.reduce_jac(np.asarray(jac(xdata, self.expand_x(X, Pfix))))


class GlobalMap:
    """The map of a global fit: S data sets of one model, fitted together, share some parameters.

    Every data set has the n parameters of the model and the ``ParamMap(n, fixed, tied)`` in ``self.pm`` (nf slots).  A
    slot is *shared* iff its leader is in `shared`: it is then ONE solver variable for the whole group; every other slot
    is *local*, one variable per data set.  The group is one dense problem of ``M = S m`` rows and ``nv = ns + S nl``
    variables (ns shared slots, nl local ones), ordered

        the shared slots in ascending slot order, then the local slots of data set 0 in ascending slot order, then those
        of data set 1, ...

    ``column(k, s)`` is the variable of slot k in data set s.  The methods below ARE the definition, in the way
    ``ParamMap``'s are: blsq_model_eval_global_dev (csrc/model_kernels.hip) computes the same numbers bit for bit.
    Affine ties (``tied={j: (i, ratio, offset)}``) act inside every data set through ``self.pm``; the
    rules of `shared` do not change, and the kernel entry is then blsq_model_eval_tie_dev.

    shared : a boolean mask (n,) or a sequence of indices.  ValueError (naming the index) for an index outside
             0 .. n - 1, a fixed index, a tied key whose leader is not in `shared`, and an empty `shared` (nothing is
             shared: S independent fits, which ``curve_fit_batch`` solves).  Everything shared (nl = 0) is valid.

    Attributes: ``n``, ``S``, ``pm``, ``nf``, ``ns``, ``nl``, ``nv``, ``slot_shared`` (nf,) bool, ``shared_slots`` (ns,),
    ``local_slots`` (nl,), ``cols`` (S, nf) (``cols[s, k] == column(k, s)``).  Needs neither the library nor a GPU.
    """

    def __init__(self, n, S, shared, fixed=None, tied=None):
        self.pm = pm = ParamMap(n, fixed, tied)
        if int(S) != S or int(S) < 1:
            raise ValueError("`S` must be a positive integer.")
        self.n, self.S, self.nf = pm.n, int(S), pm.nf
        a = np.asarray(shared)
        if a.dtype == bool:
            if a.shape != (pm.n,):
                raise ValueError("a boolean `shared` must have shape (n,) = (%d,), not %s." % (pm.n, a.shape))
            idx = np.flatnonzero(a).tolist()
        else:
            idx = []
            for j in np.atleast_1d(a).ravel().tolist() if a.size else []:
                if int(j) != j or not 0 <= int(j) < pm.n:
                    raise ValueError("`shared` index %r is outside 0 .. %d." % (j, pm.n - 1))
                idx.append(int(j))
        if not idx:
            raise ValueError("`shared` is empty: nothing is shared between the data sets, so they are independent "
                             "fits; use `curve_fit_batch`.")
        members = set(idx)
        for j in sorted(members):
            if pm.fixed[j]:
                raise ValueError("`shared` index %d is fixed." % j)
            if j in pm.tied and pm.tied[j] not in members:
                raise ValueError("`shared` index %d is tied to parameter %d, which is not shared." % (j, pm.tied[j]))
        self.slot_shared = np.array([int(j) in members for j in pm.leaders], dtype=bool)
        self.shared_slots = np.flatnonzero(self.slot_shared)
        self.local_slots = np.flatnonzero(~self.slot_shared)
        self.ns, self.nl = len(self.shared_slots), len(self.local_slots)
        self.nv = self.ns + self.S * self.nl
        rank = np.empty(pm.nf, dtype=np.intp)
        rank[self.shared_slots] = np.arange(self.ns)
        rank[self.local_slots] = self.ns + np.arange(self.nl)
        self.cols = rank[None, :] + np.where(self.slot_shared, 0, self.nl)[None, :] * np.arange(self.S)[:, None]

    def __repr__(self):
        return "GlobalMap(n=%d, S=%d, ns=%d, nl=%d, nv=%d)" % (self.n, self.S, self.ns, self.nl, self.nv)

    def column(self, k, s):
        """The solver variable of slot k in data set s."""
        if not 0 <= int(k) < self.nf or not 0 <= int(s) < self.S:
            raise ValueError("slot %r / data set %r outside 0 .. %d / 0 .. %d." % (k, s, self.nf - 1, self.S - 1))
        return int(self.cols[int(s), int(k)])

    def _sets(self, a, width, name):
        a = np.asarray(a)
        if a.ndim < 2 or a.shape[-2:] != (self.S, width):
            raise ValueError("`%s` must have shape (..., S, %d) = (..., %d, %d), not %s."
                             % (name, width, self.S, width, a.shape))
        return a

    def reduce_x(self, P):
        """(..., S, n) -> (..., nv): the leaders' values; a shared variable takes its start from data set 0."""
        Xs = self.pm.reduce_x(self._sets(P, self.n, "P"))                       # (..., S, nf)
        out = np.empty(Xs.shape[:-2] + (self.nv,), dtype=Xs.dtype)
        out[..., :self.ns] = Xs[..., 0, self.shared_slots]
        for s in range(self.S):
            out[..., self.cols[s, self.local_slots]] = Xs[..., s, self.local_slots]
        return out

    def split_x(self, X):
        """(..., nv) -> (..., S, nf): the nf variables of every data set.  Copies only."""
        X = np.asarray(X)
        if X.ndim < 1 or X.shape[-1] != self.nv:
            raise ValueError("`X` must have %d entries along its last axis, not shape %s." % (self.nv, X.shape))
        return X[..., self.cols]

    def expand_x(self, X, Pfix):
        """(..., nv) and the template (..., S, n) -> (..., S, n): ``ParamMap.expand_x`` of every data set's variables
        (copies; ``ratio * x + offset`` for an affine tie).  Of `Pfix` the fixed columns are read."""
        return self.pm.expand_x(self.split_x(X), self._sets(Pfix, self.n, "Pfix"))

    def reduce_jac(self, J_full):
        """(..., S, m, n) -> (..., S m, nv): data set s fills the rows s m .. s m + m with ``ParamMap.reduce_jac`` of its
        block, scattered into its own columns; every other entry of those rows is +0.0."""
        J_full = np.asarray(J_full)
        if J_full.ndim < 3 or J_full.shape[-3] != self.S or J_full.shape[-1] != self.n:
            raise ValueError("`J_full` must have shape (..., S, m, n) = (..., %d, m, %d), not %s."
                             % (self.S, self.n, J_full.shape))
        Jr = self.pm.reduce_jac(J_full)                                         # (..., S, m, nf)
        m = Jr.shape[-2]
        out = np.zeros(Jr.shape[:-1] + (self.nv,), dtype=Jr.dtype)
        for s in range(self.S):
            out[..., s, :, :][..., self.cols[s]] = Jr[..., s, :, :]
        return out.reshape(Jr.shape[:-3] + (self.S * m, self.nv))

    def reduce_bounds(self, lb, ub):
        """(..., S, n) bounds -> (..., nv): per data set ``ParamMap.reduce_bounds``; the box of a shared variable is the
        intersection over the data sets as well.  ValueError where an intersection is empty."""
        lo_s, hi_s = self.pm.reduce_bounds(self._sets(lb, self.n, "lb"), self._sets(ub, self.n, "ub"))
        lo = np.empty(lo_s.shape[:-2] + (self.nv,))
        hi = np.empty(hi_s.shape[:-2] + (self.nv,))
        lo[..., :self.ns] = np.max(lo_s[..., self.shared_slots], axis=-2)
        hi[..., :self.ns] = np.min(hi_s[..., self.shared_slots], axis=-2)
        for s in range(self.S):
            lo[..., self.cols[s, self.local_slots]] = lo_s[..., s, self.local_slots]
            hi[..., self.cols[s, self.local_slots]] = hi_s[..., s, self.local_slots]
        if np.any(lo[..., :self.ns] > hi[..., :self.ns]):
            k = int(self.shared_slots[int(np.argwhere(lo[..., :self.ns] > hi[..., :self.ns])[0][-1])])
            raise ValueError("the bounds of the shared parameters %s do not intersect over the data sets."
                             % self.pm.group(k).tolist())
        return lo, hi

    def expand_cov(self, C):
        """(..., nv, nv) -> (..., S, n, n): the block ``T_s C T_s^T`` of every data set (``ParamMap.expand_cov`` of the
        rows and columns of its variables: copies, times the ratios of affine ties).  The cross-data-set terms stay in
        `C`."""
        C = np.asarray(C)
        if C.ndim < 2 or C.shape[-2:] != (self.nv, self.nv):
            raise ValueError("`C` must have shape (..., nv, nv) = (..., %d, %d), not %s." % (self.nv, self.nv, C.shape))
        return np.stack([self.pm.expand_cov(C[..., c[:, None], c[None, :]]) for c in self.cols], axis=-3)

    def expand_mask(self, mask):
        """active_mask (..., nv) -> (..., S, n): 0 for a fixed parameter, its variable's value otherwise (times the sign
        of the ratio of an affine tie)."""
        return self.pm.expand_mask(self.split_x(mask))

    def matrix(self):
        """T (S n, nv): row s n + j has ``ratio[j]`` (1 without affine ties) in the column of parameter j of data set s
        (nothing where j is fixed)."""
        T = np.zeros((self.S * self.n, self.nv))
        Tp = self.pm.matrix()
        for s in range(self.S):
            T[s * self.n:(s + 1) * self.n, self.cols[s]] = Tp
        return T

    # ---- numpy callables over the solver's variables -------------------------------------------------------------
    def wrap_f(self, f, Pfix):
        """``f(xdata, P (G S, n)) -> (G S, m)`` -> ``g(xdata, X (G, nv)) -> (G, S m)``; `Pfix` (G, S, n)."""
        def g(xdata, X):
            P = self.expand_x(X, Pfix)
            F = np.asarray(f(xdata, P.reshape(-1, self.n)))
            return F.reshape(P.shape[:-2] + (self.S * F.shape[-1],))
        return g

    def wrap_jac(self, jac, Pfix):
        """``jac(xdata, P (G S, n)) -> (G S, m, n)`` -> ``g(xdata, X (G, nv)) -> (G, S m, nv)``."""
        def g(xdata, X):
            P = self.expand_x(X, Pfix)
            J = np.asarray(jac(xdata, P.reshape(-1, self.n)))
            return self.reduce_jac(J.reshape(P.shape[:-2] + (self.S,) + J.shape[-2:]))
        return g
