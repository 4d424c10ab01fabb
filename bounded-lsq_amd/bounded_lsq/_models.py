"""Built-in fit models (``bounded_lsq.models``): five closed-form families that ``curve_fit_batch`` evaluates on the GPU
(blsq_model_eval_dev of include/blsq.h, csrc/model_kernels.hip).

Parameter order is fixed and a constant offset ``c`` is always last:

    name          model                                                        n        xdata
    poly          sum_{k<n} p_k t^k                                            >= 1     (m,) or (B, m)
    exp_sum       sum_k a_k exp(-r_k t) + c            (a_1, r_1, ..., c)      2K + 1   (m,) or (B, m)
    gauss_sum     sum_k a_k exp(-z_k^2 / 2) + c,  z_k = (t - mu_k) / s_k       3K + 1   (m,) or (B, m)
                                                       (a_1, mu_1, s_1, ..., c)
    lorentz_sum   sum_k a_k / (1 + z_k^2) + c          same parameters         3K + 1   (m,) or (B, m)
    gauss2d       a exp(-((u-u0)^2 + (v-v0)^2) / (2 s^2)) + c   (a, u0, v0, s, c)   5   (2, m) or (B, 2, m)

The numpy functions ``MODELS[name].f(xdata, P) -> (B, m)`` and ``.jac(xdata, P) -> (B, m, n)`` below ARE the definition
of each model: the kernel evaluates the same formulas operation by operation (it is compiled without contraction), so
the two differ by the last bit of exp() only.  They are vectorised over the batch, keep the dtype of their inputs
(np.longdouble inputs give a longdouble reference) and check nothing: a non-finite value (s = 0) passes through.
They are also the ``driver='host'`` route of ``curve_fit_batch(f='name')``.

Composite models (``compose``; blsq_model_eval_comp_dev).  ``compose('gauss*2+lorentz+poly*2')`` is a sum of
components chosen at run time, each ``family`` or ``family*K`` (K >= 1) of

    family    term                                                             parameters per term
    gauss     a exp(-z^2 / 2),  z = (t - mu) / s                               3: (a, mu, s)
    lorentz   a / (1 + z^2)                                                    3: (a, mu, s)
    pvoigt    a [G + eta (L - G)],  G = exp(-ln2 z^2),  L = 1 / (1 + z^2)      4: (a, mu, s, eta)   (s: the HWHM of both)
    exp       a exp(-r t)                                                      2: (a, r)
    poly      ``poly*d``: p_0 + p_1 t + ... + p_{d-1} t^{d-1} by Horner        1: d coefficients

with no implicit offset (a constant is ``poly*1``), at most 8 components and 1 <= n <= 64.  The parameters are the
concatenation of the components' slices in spec order; a component's value is the sum of its terms in ascending order,
the model the sequential sum of the component values.  The terms are computed by the functions the five families use, so
``gauss*K+poly*1`` is ``gauss_sum`` bit for bit (and likewise lorentz, exp and ``poly*n``).  Wherever a name is taken
(``curve_fit_batch``, ``DeviceModel``, ``DeviceFit``, ``evaluate``) a spec string or a ``CompositeModel`` is as well
(``resolve``).

Poisson maximum likelihood (``estimator='poisson'``; blsq_model_eval_est_dev).  For counts y >= 0 and a
model value mu > 0 the residual of a fit becomes the deviance residual ``r = sign(mu - y) sqrt(D)``,
``D = 2 [mu - y + y ln(y / mu)]``, so that ``sum r^2`` is the Poisson deviance and its minimiser the maximum-likelihood
estimate; the Jacobian row is the model's row times ``c = dr / dmu``.  ``poisson_transform(mu, y) -> (r, c)`` IS the
definition, in a form that neither cancels nor divides 0 by 0 at mu == y, and the kernel follows it operation by
operation; ``poisson_residual`` and ``poisson_jacobian`` wrap any ``f(xdata, P)`` / ``jac(xdata, P)`` with it: the
``driver='host'`` route and the route of a callable.  Nothing is checked: mu <= 0 passes through as IEEE arithmetic gives
it, so the bounds of a fit must keep the model positive.

Bin-integrated models (``binned=True``; blsq_model_eval_bin_dev).  ``binned(name)`` is the model whose row i
is the integral of the point-sampled model over the bin [lo_i, hi_i] (gauss2d: over a pixel): the expected content of a
histogram channel for a model read as a density, with the same parameters in the same order and the integrals of the
columns as its Jacobian.  Its numpy ``f`` / ``jac`` ARE the definition (closed forms: ``erf_diff`` switches to erfc where
both edges lie in one tail, atan2 for the Lorentzian, ``psi_pair`` with a series through r = 0 for a decay); the BINNED
kernel instances follow them operation by operation.

Missing data (``nan_policy='omit'``; blsq_model_eval_nan_dev).  Point i of problem b is omitted iff
``ydata[b, i]`` is NaN: its residual and its Jacobian row are exactly 0, and its `sigma` entry and abscissa are never
looked at.  ``omit_residual`` / ``omit_jacobian`` ARE the definition (``np.where(isnan(ydata), 0, .)``, applied
outermost) and the route of ``driver='host'`` and of callables; the OMIT kernel instances produce the same zeros without
evaluating the row.  ``count_observed`` gives the points each problem keeps and ``pad_ragged`` turns data sets of
unequal length into the NaN-padded batch the policy takes.

Global fits (``global_map=``; blsq_model_eval_global_dev).  With a ``bounded_lsq.GlobalMap`` a
``DeviceModel`` / ``DeviceFit`` evaluates G groups of S data sets, a group being one problem of S m rows over the
nv = ns + S nl variables of the map; ``GlobalMap`` IS the definition of the layout and the kernel follows it bit for bit.
One coordinate and point sampling only.

Affine ties (``tied={j: (i, ratio, offset)}``; blsq_model_eval_tie_dev).  Where the ``ParamMap`` of a fit
(``param_map``, or ``global_map.pm``) has ``affine`` set, ``DeviceModel`` hands its ``ratio`` and ``offset`` to the one
entry that takes them, for batch and global fits and under every flag above; ``ParamMap`` IS the definition
(``expand_x``: ratio * x + offset; ``reduce_jac``: the columns times their ratios) and the kernel follows it bit for bit.

Instrument response (``response=``, ``response_origin=``; blsq_response_apply_dev).  The model is convolved
with a measured kernel h before it meets the data: ``apply_response(g, h, origin)`` IS the definition,
``mu[i] = sum_k h[k] g[i + origin - k]`` with the terms outside [0, m) dropped, over the SAMPLE INDEX: a uniform grid,
and h sampled at its spacing, are the caller's business.  ``response_residual`` / ``response_jacobian`` wrap any
``f(xdata, P)`` / ``jac(xdata, P)`` with it: the ``driver='host'`` route and the route of a callable.  On the device
the convolution is a second stage behind the model kernel, which is called as ``evaluate`` calls it; data, weights,
estimator and omission are applied by the second stage.

Expression models (``expression``; blsq_expr_eval_dev).  ``expression('a*exp(-t/tau)+c', ('a', 'tau',
'c'))`` is a model given as a formula: an ``ExprModel``, compiled on the host into a short program that a kernel of its
own interprets per row, with the exact Jacobian from a reverse sweep.  bounded_lsq/_expr.py has the language and the
numpy interpreter that IS the definition.  An ``ExprModel`` is taken wherever a ``CompositeModel`` is, except by
``binned=True`` and by global fits (ValueError).

Separable fits (``separable=True``; blsq_varpro_expand_dev, blsq_varpro_reduce_dev).  The parameters a model
is linear in (``linear_params``: amplitudes, polynomial coefficients, offsets) are projected out, so that the solver sees
the others alone: bounded_lsq/_varpro.py has the scheme and ``varpro_reduce``, which IS the definition; on the device
the projection is a second stage behind the model kernel, which is called for the raw Jacobian at unit linear parameters.
"""
import re

import numpy as np

from . import _abi
from ._expr import ExprModel, expression
from ._varpro import (VARPRO_MAX_NL, VARPRO_PIVOT_TOL, linear_params, varpro_reduce, varpro_expand, separable_residual,
                      separable_jacobian, separable_coefficients, separable_global_map, separable_global_residual,
                      separable_global_jacobian, separable_global_coefficients, separable_global_cov)

MAX_N = 64                                   # BLSQ_MODEL_MAX_N
MAX_COMP = 8                                 # BLSQ_MODEL_MAX_COMP
LN2 = 0.6931471805599453

ESTIMATORS = ('lse', 'poisson')              # BLSQ_EST_*
SAMPLING = ('point', 'bin')                  # BLSQ_SAMPLE_*
NAN_POLICIES = ('propagate', 'omit')         # BLSQ_NAN_*
POISSON_U0 = 0.25                            # |u| below which phi(u) is its series
POISSON_TERMS = 26                           # ... of this many terms
RESPONSE_MAX_L = 1024                        # BLSQ_RESPONSE_MAX_L

__all__ = ['MODELS', 'NAMES', 'MAX_N', 'MAX_COMP', 'TERMS', 'get', 'compose', 'resolve', 'CompositeModel', 'evaluate',
           'DeviceModel', 'DeviceFit', 'ESTIMATORS', 'POISSON_U0', 'POISSON_TERMS', 'check_estimator',
           'poisson_transform', 'poisson_residual', 'poisson_jacobian', 'binned', 'bin_rows', 'BinnedModel', 'erf_diff',
           'psi_pair', 'PSI_X0', 'PSI_TERMS', 'SAMPLING', 'NAN_POLICIES', 'check_nan_policy', 'omit_residual',
           'omit_jacobian', 'count_observed', 'pad_ragged', 'RESPONSE_MAX_L', 'check_response', 'apply_response',
           'response_residual', 'response_jacobian', 'expression', 'ExprModel', 'VARPRO_MAX_NL', 'VARPRO_PIVOT_TOL',
           'linear_params', 'varpro_reduce', 'varpro_expand', 'separable_residual', 'separable_jacobian',
           'separable_coefficients', 'check_separable', 'separable_global_map', 'separable_global_residual',
           'separable_global_jacobian', 'separable_global_coefficients', 'separable_global_cov']


def _tp(xdata, P):
    """t broadcastable against the (B, 1) parameter columns, and P, in their common floating dtype."""
    P = np.asarray(P)
    t = np.asarray(xdata)
    dt = np.result_type(P.dtype, t.dtype, np.float64)
    return t.astype(dt, copy=False), P.astype(dt, copy=False)


def _col(P, k):
    return P[:, k, np.newaxis]


def _poly_f(xdata, P):
    t, P = _tp(xdata, P)
    n = P.shape[1]
    acc = np.broadcast_to(_col(P, n - 1), np.broadcast(_col(P, 0), t).shape)       # Horner
    for k in range(n - 2, -1, -1):
        acc = acc * t + _col(P, k)
    return acc


def _poly_jac(xdata, P):
    t, P = _tp(xdata, P)
    B, n = P.shape
    J = np.empty((B, t.shape[-1], n), dtype=P.dtype)
    pw = np.ones_like(t)
    for k in range(n):                                             # t^k by repeated product
        J[:, :, k] = pw
        pw = pw * t
    return J


def _exp_terms(t, P, K=None):
    """k, e (d / da), g (the term) of the K decays at the front of P (default: all but the offset)."""
    for k in range((P.shape[1] - 1) // 2 if K is None else K):
        a, r = _col(P, 2 * k), _col(P, 2 * k + 1)
        e = np.exp(-(r * t))
        yield k, e, a * e


def _exp_f(xdata, P):
    t, P = _tp(xdata, P)
    acc = None
    for k, e, g in _exp_terms(t, P):
        acc = g if acc is None else acc + g
    return acc + _col(P, -1)


def _exp_jac(xdata, P):
    t, P = _tp(xdata, P)
    B, n = P.shape
    J = np.empty((B, t.shape[-1], n), dtype=P.dtype)
    for k, e, g in _exp_terms(t, P):
        J[:, :, 2 * k] = e
        J[:, :, 2 * k + 1] = -(t * g)
    J[:, :, n - 1] = 1.0
    return J


def _peak_terms(t, P, lorentz, K=None):
    """k, e (d / da), g (the term), dmu, z of the K peaks at the front of P (default: all but the offset)."""
    for k in range((P.shape[1] - 1) // 3 if K is None else K):
        a, mu, s = _col(P, 3 * k), _col(P, 3 * k + 1), _col(P, 3 * k + 2)
        z = (t - mu) / s
        if lorentz:
            e = 1.0 / (1.0 + z * z)
            g = a * e
            dmu = (((2.0 * g) * e) * z) / s
        else:
            e = np.exp(-0.5 * (z * z))
            g = a * e
            dmu = (g * z) / s
        yield k, e, g, dmu, z


def _peak_f(lorentz):
    def f(xdata, P):
        t, P = _tp(xdata, P)
        acc = None
        for k, e, g, dmu, z in _peak_terms(t, P, lorentz):
            acc = g if acc is None else acc + g
        return acc + _col(P, -1)
    return f


def _peak_jac(lorentz):
    def jac(xdata, P):
        t, P = _tp(xdata, P)
        B, n = P.shape
        J = np.empty((B, t.shape[-1], n), dtype=P.dtype)
        for k, e, g, dmu, z in _peak_terms(t, P, lorentz):
            J[:, :, 3 * k] = e
            J[:, :, 3 * k + 1] = dmu
            J[:, :, 3 * k + 2] = dmu * z
        J[:, :, n - 1] = 1.0
        return J
    return jac


def _g2_parts(xdata, P):
    t, P = _tp(xdata, P)
    du = t[..., 0, :] - _col(P, 1)
    dv = t[..., 1, :] - _col(P, 2)
    s = _col(P, 3)
    r2 = du * du + dv * dv
    s2 = s * s
    e = np.exp(-0.5 * (r2 / s2))
    return P, du, dv, s, r2, s2, e, _col(P, 0) * e


def _g2_f(xdata, P):
    P, du, dv, s, r2, s2, e, g = _g2_parts(xdata, P)
    return g + _col(P, 4)


def _g2_jac(xdata, P):
    P, du, dv, s, r2, s2, e, g = _g2_parts(xdata, P)
    J = np.empty(e.shape + (5,), dtype=P.dtype)
    J[:, :, 0] = e
    J[:, :, 1] = (g * du) / s2
    J[:, :, 2] = (g * dv) / s2
    J[:, :, 3] = (g * r2) / (s2 * s)
    J[:, :, 4] = 1.0
    return J


class Model:
    """One row of the registry: ``id`` (BLSQ_MODEL_*), ``coords`` (rows of xdata per point), the rule for n
    (``n_per_term == 0``: n == n_base; otherwise n = n_base + K * n_per_term, K >= 1) and the numpy ``f`` / ``jac``."""

    def __init__(self, id, name, coords, n_base, n_per_term, f, jac):
        self.id, self.name, self.coords, self.n_base, self.n_per_term = id, name, coords, n_base, n_per_term
        self.f, self.jac = f, jac

    def terms(self, n):
        """Number of terms K for n parameters; ValueError if n does not fit the model."""
        n = int(n)
        if self.n_per_term == 0:
            ok, K = n == self.n_base, 1
        else:
            K, rem = divmod(n - self.n_base, self.n_per_term)
            ok = n > self.n_base and rem == 0
        if not ok or not 1 <= n <= MAX_N:
            raise ValueError("model '%s' does not take n = %d parameters (%s, n <= %d)." % (self.name, n, self.rule(), MAX_N))
        return K

    def rule(self):
        if self.n_per_term == 0:
            return "n = %d" % self.n_base
        if self.n_base == 0 and self.n_per_term == 1:
            return "n >= 1"
        return "n = %d K + %d" % (self.n_per_term, self.n_base)

    def check_xdata(self, xdata, B, m):
        """xdata as a float64 array of shape (m,) / (B, m) — (2, m) / (B, 2, m) for two coordinates; ValueError
        otherwise.  Returns (array, per_problem)."""
        x = np.asarray(xdata, dtype=np.float64)
        shared = (m,) if self.coords == 1 else (self.coords, m)
        if x.shape == (B,) + shared:
            return np.ascontiguousarray(x), True
        if x.shape == shared:
            return np.ascontiguousarray(x), False
        raise ValueError("`xdata` of model '%s' must have shape %s or %s, not %s."
                         % (self.name, shared, (B,) + shared, x.shape))


MODELS = {m.name: m for m in (
    Model(0, 'poly', 1, 0, 1, _poly_f, _poly_jac),
    Model(1, 'exp_sum', 1, 1, 2, _exp_f, _exp_jac),
    Model(2, 'gauss_sum', 1, 1, 3, _peak_f(False), _peak_jac(False)),
    Model(3, 'lorentz_sum', 1, 1, 3, _peak_f(True), _peak_jac(True)),
    Model(4, 'gauss2d', 2, 5, 0, _g2_f, _g2_jac),
)}
NAMES = tuple(MODELS)


def get(name):
    """The registry row of `name`; ValueError for anything else."""
    if not isinstance(name, str) or name not in MODELS:
        raise ValueError("unknown model %r: a built-in model is one of %s." % (name, ", ".join(NAMES)))
    return MODELS[name]


# ---- composite models ----------------------------------------------------------------------------------------------
def _pvoigt_terms(t, P, K):
    """k, h (d / da), g (the term), dmu, z, a d (d / deta) of the K pseudo-Voigt peaks at the front of P."""
    for k in range(K):
        a, mu, s, eta = (_col(P, 4 * k + i) for i in range(4))
        z = (t - mu) / s
        q = z * z
        G = np.exp(-(LN2 * q))
        L = 1.0 / (1.0 + q)
        d = L - G
        h = G + eta * d
        g = a * h
        lg = LN2 * G
        u = lg + eta * (L * L - lg)
        dmu = (((2.0 * a) * u) * z) / s
        yield k, h, g, dmu, z, a * d


def _fill_exp(t, P, K, J):
    acc = None
    for k, e, g in _exp_terms(t, P, K):
        acc = g if acc is None else acc + g
        if J is not None:
            J[:, :, 2 * k] = e
            J[:, :, 2 * k + 1] = -(t * g)
    return acc


def _fill_peak(lorentz):
    def fill(t, P, K, J):
        acc = None
        for k, e, g, dmu, z in _peak_terms(t, P, lorentz, K):
            acc = g if acc is None else acc + g
            if J is not None:
                J[:, :, 3 * k] = e
                J[:, :, 3 * k + 1] = dmu
                J[:, :, 3 * k + 2] = dmu * z
        return acc
    return fill


def _fill_pvoigt(t, P, K, J):
    acc = None
    for k, h, g, dmu, z, deta in _pvoigt_terms(t, P, K):
        acc = g if acc is None else acc + g
        if J is not None:
            J[:, :, 4 * k] = h
            J[:, :, 4 * k + 1] = dmu
            J[:, :, 4 * k + 2] = dmu * z
            J[:, :, 4 * k + 3] = deta
    return acc


def _fill_poly(t, P, K, J):
    if J is not None:
        J[:, :, :] = _poly_jac(t, P)
    return _poly_f(t, P)


class Term:
    """One row of the term table: ``id`` (BLSQ_TERM_*), ``name``, ``n_per_term``, the names of a term's parameters and
    ``fill(t, P, K, J) -> value``: the component's value for its slice P (B, K n_per_term), its columns written into the
    view J (B, m, K n_per_term) unless J is None."""

    def __init__(self, id, name, n_per_term, params, fill):
        self.id, self.name, self.n_per_term, self.params, self.fill = id, name, n_per_term, params, fill


TERMS = {t.name: t for t in (
    Term(0, 'gauss', 3, ('a', 'mu', 's'), _fill_peak(False)),
    Term(1, 'lorentz', 3, ('a', 'mu', 's'), _fill_peak(True)),
    Term(2, 'pvoigt', 4, ('a', 'mu', 's', 'eta'), _fill_pvoigt),
    Term(3, 'exp', 2, ('a', 'r'), _fill_exp),
    Term(4, 'poly', 1, None, _fill_poly),
)}


class CompositeModel:
    """A sum of components ``((family, K), ...)``, built by ``compose``; offers what a ``Model`` offers its callers:
    ``name`` (the canonical spec), ``coords`` (1), ``n``, ``terms``, ``check_xdata``, the numpy ``f`` / ``jac`` — and
    ``components`` and ``param_names``."""

    coords = 1
    check_xdata = Model.check_xdata

    def __init__(self, components):
        self.components = tuple((str(fam), int(K)) for fam, K in components)
        self.name = "+".join("%s*%d" % c for c in self.components)
        self.n = sum(K * TERMS[fam].n_per_term for fam, K in self.components)
        names, seen = [], {}                     # 'gauss1.mu': the second gauss term of the spec; 'poly0.p2'
        for fam, K in self.components:
            T = TERMS[fam]
            for k in range(1 if T.params is None else K):
                i = seen[fam] = seen.get(fam, -1) + 1
                names += (["%s%d.p%d" % (fam, i, d) for d in range(K)] if T.params is None
                          else ["%s%d.%s" % (fam, i, q) for q in T.params])
        self.param_names = tuple(names)
        self.fam_ids = np.array([TERMS[fam].id for fam, K in self.components], dtype=np.int32)
        self.counts = np.array([K for fam, K in self.components], dtype=np.int32)

    def terms(self, n):
        """The total number of terms; ValueError unless n is the spec's n."""
        if int(n) != self.n:
            raise ValueError("model '%s' does not take n = %d parameters (n = %d)." % (self.name, int(n), self.n))
        return int(self.counts.sum())

    def rule(self):
        return "n = %d" % self.n

    def _walk(self, xdata, P, want_J):
        t, P = _tp(xdata, P)
        if P.shape[1] != self.n:
            raise ValueError("model '%s' does not take n = %d parameters (n = %d)." % (self.name, P.shape[1], self.n))
        J = np.empty((P.shape[0], t.shape[-1], self.n), dtype=P.dtype) if want_J else None
        acc, o = None, 0
        for fam, K in self.components:
            T = TERMS[fam]
            w = K * T.n_per_term
            v = T.fill(t, P[:, o:o + w], K, None if J is None else J[:, :, o:o + w])
            acc = v if acc is None else acc + v
            o += w
        return acc, J

    def f(self, xdata, P):
        return self._walk(xdata, P, False)[0]

    def jac(self, xdata, P):
        return self._walk(xdata, P, True)[1]

    def __repr__(self):
        return "CompositeModel(%r)" % self.name


def compose(spec):
    """The ``CompositeModel`` of `spec`: components ``family`` or ``family*K`` (K >= 1) joined by ``+``, whitespace
    ignored; ValueError naming the offending piece otherwise."""
    if not isinstance(spec, str):
        raise ValueError("a composite model is given as a string such as 'gauss*2+poly*1', not %r." % (spec,))
    pieces = re.sub(r"\s+", "", spec).split("+")
    if len(pieces) > MAX_COMP:
        raise ValueError("composite model %r has %d components, more than %d." % (spec, len(pieces), MAX_COMP))
    comps = []
    for piece in pieces:
        if not piece:
            raise ValueError("composite model %r has an empty component." % spec)
        fam, star, count = piece.partition("*")
        if fam not in TERMS:
            raise ValueError("unknown family %r in composite model %r: a family is one of %s."
                             % (fam, spec, ", ".join(TERMS)))
        K = 1
        if star:
            if not re.fullmatch(r"[+-]?[0-9]+", count):
                raise ValueError("component %r of composite model %r: the count must be an integer K >= 1." % (piece, spec))
            K = int(count)
        if K < 1:
            raise ValueError("component %r of composite model %r: K must be at least 1." % (piece, spec))
        comps.append((fam, K))
    M = CompositeModel(comps)
    if M.n > MAX_N:
        raise ValueError("composite model %r has n = %d parameters, more than %d." % (spec, M.n, MAX_N))
    return M


def resolve(f):
    """A ``CompositeModel`` or an ``ExprModel`` as it is; a string holding ``+`` or ``*`` through ``compose``; anything
    else through ``get``."""
    if isinstance(f, (CompositeModel, ExprModel)):
        return f
    if isinstance(f, str) and ("+" in f or "*" in f):
        return compose(f)
    return get(f)


def resolvable(model):
    """What ``resolve`` turns back into `model`: the object itself for an ``ExprModel`` (its name is no spec), the name
    otherwise."""
    return model if isinstance(model, ExprModel) else model.name


# ---- bin-integrated models -------------------------------------------------------------------------------------------
# (BINNED instances of csrc/model_kernels.hip, blsq_model_eval_bin_dev)
SQRT_HALF = 0.7071067811865476               # 1 / sqrt(2): erf argument of a gauss edge
SQRT_PI_2 = 1.2533141373155001               # sqrt(pi / 2): integral of exp(-z^2 / 2) over the line, halved
SQRT_LN2 = 0.8325546111576977                # sqrt(ln 2): erf argument of the Gaussian part of a pvoigt edge
PV_GNORM = 1.0644670194312262                # sqrt(pi / ln 2) / 2
PSI_X0 = 0.5                                 # |r w| below which psi and psi' are their series
PSI_TERMS = 16                               # ... of this many terms


def _fact(k):
    """k! as a float (exact for k <= 18)."""
    v = 1.0
    for i in range(2, k + 1):
        v *= i
    return v


def erf_diff(xl, xh):
    """erf(xh) - erf(xl) without the cancellation of a tail: both arguments positive: erfc(xl) - erfc(xh); both negative:
    erfc(-xh) - erfc(-xl); otherwise the plain difference.  scipy.special's float64 erf / erfc are the definition; another
    dtype is computed in float64 and cast back."""
    from scipy import special
    xl, xh = np.broadcast_arrays(np.asarray(xl), np.asarray(xh))
    dt = np.result_type(xl.dtype, np.float64)
    a, b = xl.astype(np.float64), xh.astype(np.float64)
    up = special.erfc(a) - special.erfc(b)
    dn = special.erfc(-b) - special.erfc(-a)
    mid = special.erf(b) - special.erf(a)
    return np.where((a > 0) & (b > 0), up, np.where((a < 0) & (b < 0), dn, mid)).astype(dt, copy=False)


def psi_pair(x):
    """psi(x) = -expm1(-x) / x (psi(0) = 1) and its derivative psi'(x) = (x exp(-x) + expm1(-x)) / x^2 (-1 / 2 at 0): as
    written where |x| >= PSI_X0, by PSI_TERMS terms of the series sum_k (-x)^k / (k + 1)! and
    -sum_k (k + 1) (-x)^k / (k + 2)! (Horner) below."""
    x = np.asarray(x)
    dt = np.result_type(x.dtype, np.float64)
    x = x.astype(dt, copy=False)
    one = dt.type(1)
    with np.errstate(all='ignore'):
        T = PSI_TERMS
        ps = np.full(x.shape, (-one) ** (T - 1) / dt.type(_fact(T)))
        dp = np.full(x.shape, (-one) ** T * dt.type(T) / dt.type(_fact(T + 1)))
        for k in range(T - 2, -1, -1):                                   # Horner
            ps = ps * x + (-one) ** k / dt.type(_fact(k + 1))
            dp = dp * x + (-one) ** (k + 1) * dt.type(k + 1) / dt.type(_fact(k + 2))
        em = np.expm1(-x)
        small = np.abs(x) < PSI_X0
        ps = np.where(small, ps, -em / x)
        dp = np.where(small, dp, (x * np.exp(-x) + em) / (x * x))
    return ps, dp


def _bfill_peak(lorentz):
    def fill(lo, hi, P, K, J):
        acc = None
        for k in range(K):
            a, mu, s = _col(P, 3 * k), _col(P, 3 * k + 1), _col(P, 3 * k + 2)
            zl = (lo - mu) / s
            zh = (hi - mu) / s
            if lorentz:
                el = 1.0 / (1.0 + zl * zl)
                eh = 1.0 / (1.0 + zh * zh)
                da = s * np.arctan2((hi - lo) / s, 1.0 + zh * zl)
            else:
                el = np.exp(-0.5 * (zl * zl))
                eh = np.exp(-0.5 * (zh * zh))
                da = (s * SQRT_PI_2) * erf_diff(zl * SQRT_HALF, zh * SQRT_HALF)
            g = a * da
            acc = g if acc is None else acc + g
            if J is not None:
                J[:, :, 3 * k] = da
                J[:, :, 3 * k + 1] = a * (el - eh)
                J[:, :, 3 * k + 2] = g / s - a * (zh * eh - zl * el)
        return acc
    return fill


def _bfill_pvoigt(lo, hi, P, K, J):
    acc = None
    for k in range(K):
        a, mu, s, eta = (_col(P, 4 * k + i) for i in range(4))
        zl = (lo - mu) / s
        zh = (hi - mu) / s
        ql = zl * zl
        qh = zh * zh
        Gl = np.exp(-(LN2 * ql))
        Gh = np.exp(-(LN2 * qh))
        Ll = 1.0 / (1.0 + ql)
        Lh = 1.0 / (1.0 + qh)
        IG = (s * PV_GNORM) * erf_diff(zl * SQRT_LN2, zh * SQRT_LN2)
        IL = s * np.arctan2((hi - lo) / s, 1.0 + zh * zl)
        d = IL - IG
        h = IG + eta * d
        g = a * h
        acc = g if acc is None else acc + g
        if J is not None:
            mG = Gl - Gh
            uG = zh * Gh - zl * Gl
            J[:, :, 4 * k] = h
            J[:, :, 4 * k + 1] = a * (mG + eta * ((Ll - Lh) - mG))
            J[:, :, 4 * k + 2] = g / s - a * (uG + eta * ((zh * Lh - zl * Ll) - uG))
            J[:, :, 4 * k + 3] = a * d
    return acc


def _bfill_exp(lo, hi, P, K, J):
    acc = None
    w = hi - lo
    for k in range(K):
        a, r = _col(P, 2 * k), _col(P, 2 * k + 1)
        ps, dp = psi_pair(r * w)
        wE = w * np.exp(-(r * lo))
        da = wE * ps
        g = a * da
        acc = g if acc is None else acc + g
        if J is not None:
            J[:, :, 2 * k] = da
            J[:, :, 2 * k + 1] = (a * wE) * (w * dp - lo * ps)
    return acc


def _bfill_poly(lo, hi, P, K, J):
    n = P.shape[1]
    ph, pl = hi, lo
    acc = None
    for k in range(n):                                             # hi^(k+1), lo^(k+1) by repeated product
        c = (ph - pl) / (k + 1)
        if J is not None:
            J[:, :, k] = c
        v = _col(P, k) * c
        acc = v if acc is None else acc + v
        ph, pl = ph * hi, pl * lo
    return acc


_BFILL = {'gauss': _bfill_peak(False), 'lorentz': _bfill_peak(True), 'pvoigt': _bfill_pvoigt, 'exp': _bfill_exp,
          'poly': _bfill_poly}
_FAMILY_TERM = {'exp_sum': 'exp', 'gauss_sum': 'gauss', 'lorentz_sum': 'lorentz'}


def bin_rows(edges):
    """Contiguous bin edges (m + 1,) or (B, m + 1) as rows ``lo, hi``: (2, m) or (B, 2, m)."""
    e = np.asarray(edges)
    if e.ndim not in (1, 2) or e.shape[-1] < 2:
        raise ValueError("`xdata`: bin edges must have shape (m + 1,) or (B, m + 1) with m >= 1, not %s." % (e.shape,))
    return np.ascontiguousarray(np.stack([e[..., :-1], e[..., 1:]], axis=-2))


class BinnedModel:
    """The bin-integrated form of a ``Model`` or ``CompositeModel`` (``binned``): the value of row i is the
    integral of the point-sampled model over the bin [lo_i, hi_i] (gauss2d: over the pixel [ulo, uhi] x [vlo, vhi]), the
    expected content of the bin for a model read as a density.  Parameters, their order and ``n`` are the base model's;
    the Jacobian columns are the integrals of its columns.  Offers what the base offers: ``name``, ``n`` (a composite),
    ``terms``, ``check_xdata``, the numpy ``f`` / ``jac``, ``param_names`` (a composite), and ``base``.

    ``f`` and ``jac`` take the edges as rows: (2, m) or (B, 2, m) ``lo, hi`` — (4, m) or (B, 4, m)
    ``ulo, uhi, vlo, vhi`` for gauss2d — or, 1-D, the m + 1 contiguous edges shared by all problems (``bin_rows`` turns
    (B, m + 1) into rows; ``check_xdata``, which knows m, takes every form).  They check nothing."""

    binned = True

    def __init__(self, base):
        self.base, self.name, self.coords = base, base.name, base.coords
        for attr in ('n', 'param_names', 'components', 'fam_ids', 'counts', 'id'):
            if hasattr(base, attr):
                setattr(self, attr, getattr(base, attr))

    def terms(self, n):
        return self.base.terms(n)

    def rule(self):
        return self.base.rule()

    def _components(self, n):
        if isinstance(self.base, CompositeModel):
            return self.base.components
        self.base.terms(n)
        if self.base.name == 'poly':
            return (('poly', n),)
        fam = _FAMILY_TERM[self.base.name]
        return ((fam, (n - 1) // TERMS[fam].n_per_term), ('poly', 1))

    def _rows(self, xdata, P):
        x, P = _tp(xdata, P)
        if x.ndim == 1 and self.coords == 1:
            return [x[:-1], x[1:]], P
        return [x[..., r, :] for r in range(2 * self.coords)], P

    def _walk(self, xdata, P, want_J):
        (lo, hi), P = self._rows(xdata, P)
        n = P.shape[1]
        J = np.empty((P.shape[0], lo.shape[-1], n), dtype=P.dtype) if want_J else None
        acc, o = None, 0
        for fam, K in self._components(n):
            w = K * TERMS[fam].n_per_term
            v = _BFILL[fam](lo, hi, P[:, o:o + w], K, None if J is None else J[:, :, o:o + w])
            acc = v if acc is None else acc + v
            o += w
        return acc, J

    def _g2(self, xdata, P, want_J):
        (ulo, uhi, vlo, vhi), P = self._rows(xdata, P)
        a, u0, v0, s, c = (_col(P, k) for k in range(5))
        zul, zuh = (ulo - u0) / s, (uhi - u0) / s
        zvl, zvh = (vlo - v0) / s, (vhi - v0) / s
        c1 = s * SQRT_PI_2
        Iu = c1 * erf_diff(zul * SQRT_HALF, zuh * SQRT_HALF)
        Iv = c1 * erf_diff(zvl * SQRT_HALF, zvh * SQRT_HALF)
        da = Iu * Iv
        ww = (uhi - ulo) * (vhi - vlo)
        val = a * da + c * ww
        if not want_J:
            return val, None
        eul, euh = np.exp(-0.5 * (zul * zul)), np.exp(-0.5 * (zuh * zuh))
        evl, evh = np.exp(-0.5 * (zvl * zvl)), np.exp(-0.5 * (zvh * zvh))
        J = np.empty(val.shape + (5,), dtype=P.dtype)
        J[:, :, 0] = da
        J[:, :, 1] = (a * (eul - euh)) * Iv
        J[:, :, 2] = (a * (evl - evh)) * Iu
        J[:, :, 3] = a * ((Iu / s - (zuh * euh - zul * eul)) * Iv + Iu * (Iv / s - (zvh * evh - zvl * evl)))
        J[:, :, 4] = ww
        return val, J

    def f(self, xdata, P):
        return (self._g2 if self.coords == 2 else self._walk)(xdata, P, False)[0]

    def jac(self, xdata, P):
        return (self._g2 if self.coords == 2 else self._walk)(xdata, P, True)[1]

    def check_xdata(self, xdata, B, m):
        """The edges as a float64 array of rows, (2 coords, m) or (B, 2 coords, m), from any accepted form: contiguous
        edges (m + 1,) / (B, m + 1) (one coordinate only) or rows (2, m) / (B, 2, m) — (4, m) / (B, 4, m) for gauss2d.
        ValueError for another shape, and for the first bin whose edges are not finite or have lo >= hi.  Returns
        (array, per_problem)."""
        x = np.asarray(xdata, dtype=np.float64)
        R = 2 * self.coords
        if self.coords == 1 and x.shape in ((m + 1,), (B, m + 1)):
            x = bin_rows(x)
        if x.shape == (B, R, m):
            per_problem = True
        elif x.shape == (R, m):
            per_problem = False
        else:
            forms = ("(m + 1,), (B, m + 1), (2, m) or (B, 2, m)" if self.coords == 1 else "(4, m) or (B, 4, m)")
            raise ValueError("`xdata` of binned model '%s' must have shape %s with B = %d, m = %d, not %s."
                             % (self.name, forms, B, m, np.shape(xdata)))
        x = np.ascontiguousarray(x)
        for c in range(self.coords):
            lo, hi = x[..., 2 * c, :], x[..., 2 * c + 1, :]
            with np.errstate(invalid='ignore'):
                bad = ~(np.isfinite(lo) & np.isfinite(hi) & (lo < hi))
            if bad.any():
                idx = tuple(int(i) for i in np.argwhere(bad)[0])
                where = "bin %d" % idx[-1] + (" of problem %d" % idx[0] if per_problem else "")
                raise ValueError("`xdata` of binned model '%s': %s%s has lo = %r, hi = %r; bin edges must be finite "
                                 "with lo < hi." % (self.name, where, " (coordinate %d)" % c if self.coords > 1 else "",
                                                    float(lo[idx]), float(hi[idx])))
        return x, per_problem

    def __repr__(self):
        return "BinnedModel(%r)" % self.name


def binned(model):
    """The ``BinnedModel`` of a name, a composite spec, a ``Model`` or a ``CompositeModel`` (a ``BinnedModel`` as it is)."""
    if isinstance(model, BinnedModel):
        return model
    check_expr_model(model, binned=True)
    return BinnedModel(model if isinstance(model, Model) else resolve(model))


# ---- the Poisson estimator -------------------------------------------------------------------------------------------
def check_estimator(estimator):
    """`estimator` if it is one of ``ESTIMATORS``; ValueError otherwise."""
    if not isinstance(estimator, str) or estimator not in ESTIMATORS:
        raise ValueError("unknown estimator %r: `estimator` must be 'lse' or 'poisson'." % (estimator,))
    return estimator


def poisson_transform(mu, y):
    """The deviance residual r and c = dr / dmu of counts `y` >= 0 under model values `mu` > 0 (broadcast against each
    other; the result has their common floating dtype, so np.longdouble in gives a longdouble reference).

        D = 2 [mu - y + y ln(y / mu)]    r = sign(mu - y) sqrt(D)    c = (1 - y / mu) / r   (1 / sqrt(mu) at mu == y)

    evaluated, with d = mu - y, as
        y > 0:   u = d / y,  phi(u) = (u - log1p(u)) / u^2,  s = sqrt(2 phi / y),  r = d s,  c = 1 / (mu s)
        y == 0:  r = sqrt(2 mu),  c = 1 / r
    where phi is computed as written for |u| >= POISSON_U0 and by POISSON_TERMS terms of its series
    1/2 - u/3 + u^2/4 - ... (Horner) below: no cancellation, and r == 0 exactly with a finite c at mu == y.
    The relative error of r and c in float64 is a few eps for mu >= y / 2 and grows like eps y / mu below (u is formed
    from d / y, which forgets mu where mu << y): DESIGN.md 7m has the figures.  Nothing is checked: mu <= 0 (and a
    negative or non-finite y) passes through as IEEE arithmetic gives it."""
    mu, y = np.asarray(mu), np.asarray(y)
    dt = np.result_type(mu.dtype, y.dtype, np.float64)
    mu, y = np.broadcast_arrays(mu.astype(dt, copy=False), y.astype(dt, copy=False))
    one = dt.type(1)
    with np.errstate(all='ignore'):                # (both sides of every branch are evaluated; np.where picks)
        d = mu - y
        u = d / y
        phi = np.full(u.shape, (-one) ** (POISSON_TERMS - 1) / dt.type(POISSON_TERMS + 1))
        for k in range(POISSON_TERMS - 2, -1, -1):                       # Horner
            phi = phi * u + (-one) ** k / dt.type(k + 2)
        phi = np.where(np.abs(u) < POISSON_U0, phi, (u - np.log1p(u)) / (u * u))
        s = np.sqrt((2 * phi) / y)
        r0 = np.sqrt(2 * mu)
        pos = y > 0
        r = np.where(pos, d * s, r0)
        c = np.where(pos, one / (mu * s), one / r0)
    return r, c


def poisson_residual(f, ydata):
    """``f(xdata, P) -> (B, m)`` -> ``g(xdata, P)``: the deviance residuals of `ydata` (B, m) under the model."""
    return lambda xdata, P: poisson_transform(np.asarray(f(xdata, P)), ydata)[0]


def poisson_jacobian(f, jac, ydata):
    """``jac(xdata, P) -> (B, m, n)`` -> the Jacobian of ``poisson_residual(f, ydata)``: ``c[:, :, None] * J``.  A
    `jac` that already went through a parameter map is multiplied after the map's column sums."""
    def g(xdata, P):
        c = poisson_transform(np.asarray(f(xdata, P)), ydata)[1]
        return c[:, :, np.newaxis] * np.asarray(jac(xdata, P))
    return g


# ---- missing data --------------------------------------------------------------------------------------------------
def check_nan_policy(nan_policy):
    """`nan_policy` if it is one of ``NAN_POLICIES``; ValueError otherwise."""
    if not isinstance(nan_policy, str) or nan_policy not in NAN_POLICIES:
        raise ValueError("unknown NaN policy %r: `nan_policy` must be 'propagate' or 'omit'." % (nan_policy,))
    return nan_policy


def omit_residual(fres, ydata):
    """``fres(...) -> (B, m)`` -> the same function with exactly 0 wherever `ydata` (B, m) is NaN.  `fres` is the whole
    residual (after `sigma`, the Poisson transform and a parameter map) with any signature; what it returns at an
    omitted point is discarded, NaN included."""
    omitted = np.isnan(np.asarray(ydata, dtype=float))

    def g(*args):
        with np.errstate(invalid='ignore'):
            r = np.asarray(fres(*args))
        return np.where(omitted, r.dtype.type(0), r)
    return g


def omit_jacobian(jres, ydata):
    """``jres(...) -> (B, m, n)`` -> the same function with rows of exactly 0 wherever `ydata` (B, m) is NaN: the
    Jacobian of ``omit_residual``."""
    omitted = np.isnan(np.asarray(ydata, dtype=float))[:, :, np.newaxis]

    def g(*args):
        with np.errstate(invalid='ignore'):
            J = np.asarray(jres(*args))
        return np.where(omitted, J.dtype.type(0), J)
    return g


def count_observed(ydata):
    """The number of points of each problem that ``nan_policy='omit'`` keeps: (B,) int32, the entries of `ydata` (B, m)
    that are not NaN."""
    y = np.asarray(ydata, dtype=float)
    if y.ndim != 2:
        raise ValueError("`ydata` must have shape (B, m).")
    return np.sum(~np.isnan(y), axis=1).astype(np.int32)


def pad_ragged(xs, ys):
    """Data sets of unequal length as one batch for ``nan_policy='omit'``: `xs` and `ys` are sequences of B 1-D arrays,
    pair b of one length m_b >= 1.  Returns ``(xdata (B, m), ydata (B, m))`` with m = max m_b: x is padded by repeating
    its last value (a finite abscissa, never used) and y with NaN.  One coordinate and point sampling only; a pair of
    different lengths, an empty pair or an array that is not 1-D is a ValueError."""
    xs, ys = list(xs), list(ys)
    if len(xs) != len(ys) or not xs:
        raise ValueError("`xs` and `ys` must be sequences of the same, non-zero number of arrays.")
    pairs = []
    for b, (x, y) in enumerate(zip(xs, ys)):
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        if x.ndim != 1 or y.ndim != 1 or x.size == 0:
            raise ValueError("data set %d: x and y must be 1-D and not empty." % b)
        if x.size != y.size:
            raise ValueError("data set %d: x has %d points, y has %d." % (b, x.size, y.size))
        pairs.append((x, y))
    m = max(x.size for x, y in pairs)
    xdata = np.empty((len(pairs), m))
    ydata = np.full((len(pairs), m), np.nan)
    for b, (x, y) in enumerate(pairs):
        xdata[b, :x.size] = x
        xdata[b, x.size:] = x[-1]
        ydata[b, :y.size] = y
    return xdata, ydata


# ---- instrument response ---------------------------------------------------------------------------------------------
def check_response(response, origin=0, B=None):
    """The kernel of an instrument response as a contiguous float64 array (L,) or (B, L), and `origin` as an int.
    ValueError unless: `response` is 1-D, or 2-D with B rows (`B` None: any number); 1 <= L <= RESPONSE_MAX_L; every
    entry is finite and not all are zero; `origin` is an integer with 0 <= origin < L.  L may exceed m."""
    try:
        h = np.asarray(response, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("`response` must be an array of numbers of shape (L,) or (B, L).") from None
    if h.ndim not in (1, 2) or (h.ndim == 2 and B is not None and h.shape[0] != B):
        raise ValueError("`response` must have shape (L,) or (B, L)%s, not %s."
                         % ("" if B is None else " with B = %d" % B, h.shape))
    h = np.ascontiguousarray(h)
    L = h.shape[-1]
    if not 1 <= L <= RESPONSE_MAX_L:
        raise ValueError("`response` has L = %d taps: L must be in 1 .. %d." % (L, RESPONSE_MAX_L))
    if not np.all(np.isfinite(h)):
        raise ValueError("`response` must be finite.")
    if not np.any(h):
        raise ValueError("`response` must not be all zero.")
    if isinstance(origin, (bool, np.bool_)) or not isinstance(origin, (int, np.integer)):
        raise ValueError("`response_origin` must be an integer, not %r." % (origin,))
    if not 0 <= origin < L:
        raise ValueError("`response_origin` = %d: it must be in 0 .. L - 1 = %d." % (origin, L - 1))
    return h, int(origin)


def apply_response(g, h, origin=0):
    """The model values `g` (..., m) — or one Jacobian column moved to the last axis — convolved with the kernel `h`
    of shape (L,), or (B, L) matching the leading axis of `g`:

        mu[..., i] = sum_{k = 0}^{L - 1} h[k] * g[..., i + origin - k]

    where a term whose index i + origin - k lies outside [0, m) is dropped: ``np.convolve(g, h)[origin : origin + m]``
    with zeros past the end.  ``origin=0`` is the causal convolution of a decay with an instrument response function
    (whose delay lives in `h`); ``origin=L // 2`` with odd L is ``np.convolve(g, h, 'same')``, a centred resolution
    kernel.  The convolution is over the sample index: a uniform grid, and `h` sampled at its spacing, are the caller's
    business.  The taps are added in ascending k; the result has the common floating dtype of `g` and `h` (np.longdouble
    in gives a longdouble reference).  `h` and `origin` are checked by ``check_response``; L may exceed m."""
    g, hh = np.asarray(g), np.asarray(h)
    check_response(hh, origin, g.shape[0] if hh.ndim == 2 and g.ndim >= 1 else None)
    dt = np.result_type(g.dtype, hh.dtype, np.float64)
    g, hh = g.astype(dt, copy=False), hh.astype(dt, copy=False)
    if hh.ndim == 2 and g.ndim < 2:
        raise ValueError("a per-problem `response` (B, L) needs model values of shape (B, ..., m).")
    m, L = g.shape[-1], hh.shape[-1]
    mu = np.zeros(g.shape, dtype=dt)
    for k in range(L):
        s = origin - k                                         # mu[i] takes g[i + s]
        lo, hi = max(0, -s), min(m, m - s)
        if lo >= hi:
            continue
        hk = hh[k] if hh.ndim == 1 else hh[:, k].reshape((-1,) + (1,) * (g.ndim - 1))
        mu[..., lo:hi] += hk * g[..., lo + s:hi + s]
    return mu


def response_residual(f, h, origin=0):
    """``f(xdata, P) -> (B, m)`` -> the same model convolved with the response: ``apply_response(f(xdata, P), h, origin)``."""
    return lambda xdata, P: apply_response(np.asarray(f(xdata, P)), h, origin)


def response_jacobian(jac, h, origin=0):
    """``jac(xdata, P) -> (B, m, n)`` -> the Jacobian of ``response_residual``: every column convolved along the points.
    A `jac` that already went through a parameter map is convolved after the map's column sums."""
    def g(xdata, P):
        J = np.asarray(jac(xdata, P))
        return np.moveaxis(apply_response(np.moveaxis(J, 1, -1), h, origin), -1, 1)
    return g


def check_response_model(model, B, m, xdata=None, binned=False, global_map=None):
    """What a fit through an instrument response does not take, as ValueErrors."""
    if global_map is not None:
        raise ValueError("`response` is not supported in a global fit.")
    if model is not None and model.coords != 1:
        raise ValueError("model '%s' has %d coordinates: `response` is a convolution along one coordinate."
                         % (model.name, model.coords))
    if binned and np.shape(xdata) not in ((m + 1,), (B, m + 1)):
        raise ValueError("`response` with `binned=True` needs contiguous bins, edges of shape (m + 1,) or (B, m + 1): "
                         "a convolution over bins with gaps (rows lo, hi) is not defined.")


def check_expr_model(model, binned=False, global_fit=False):
    """What an ``ExprModel`` does not take, as ValueErrors: bin integration and global fits."""
    if isinstance(model, ExprModel):
        if binned:
            raise ValueError("`binned=True` is not supported with the expression model '%s': a formula is not "
                             "integrated over its bins." % model.name)
        if global_fit:
            raise ValueError("the expression model '%s' is not supported in a global fit." % model.name)


def check_separable(model, n, param_map=None, estimator='lse', nan_policy='propagate', global_map=None, response=None):
    """``linear_params(model, n)`` after what a separable fit does not take, as ValueErrors: a parameter
    map, the Poisson estimator, omission and an instrument response (an ``ExprModel`` and a model without a non-linear
    parameter are refused by ``linear_params``).  A `global_map` is the ``GlobalMap`` over the n - nl
    NON-LINEAR parameters (``separable_global_map``), without fixed or tied slots."""
    for what, given in (("`fixed` / `tied` (a parameter map)", param_map is not None),
                        ("estimator='poisson'", estimator != 'lse'), ("nan_policy='omit'", nan_policy != 'propagate'),
                        ("`response`", response is not None)):
        if given:
            raise ValueError("%s is not yet supported with `separable=True`." % what)
    lin, owner = linear_params(model, n)
    if global_map is not None:
        gm = global_map
        if gm.n != owner.size - lin.size or gm.nf != gm.n or gm.pm.affine:
            raise ValueError("`global_map` of a separable fit must be the GlobalMap over the %d non-linear parameters "
                             "(models.separable_global_map), without fixed or tied ones." % (owner.size - lin.size))
    return lin, owner


def check_global(model, binned=False, param_map=None):
    """What a global fit does not take, as ValueErrors."""
    check_expr_model(model, global_fit=True)
    if binned:
        raise ValueError("`binned=True` is not supported in a global fit.")
    if model.coords != 1:
        raise ValueError("model '%s' has %d coordinates: a global fit takes the models of one coordinate."
                         % (model.name, model.coords))
    if param_map is not None:
        raise ValueError("`param_map` must be None with `global_map`: the GlobalMap carries its ParamMap.")


def global_xdata(xdata, G, S, m):
    """`xdata` of a global fit — (m,) shared, (S, m) per data set or (G, S, m) per group and data set — as a contiguous
    float64 array with its group stride and data-set stride in doubles; ValueError for another shape."""
    x = np.ascontiguousarray(xdata, dtype=np.float64)
    if x.shape == (G, S, m):
        return x, S * m, m
    if x.shape == (S, m):
        return x, 0, m
    if x.shape == (m,):
        return x, 0, 0
    raise ValueError("`xdata` of a global fit must have shape (m,), (S, m) or (G, S, m) = %s, %s or %s, not %s."
                     % ((m,), (S, m), (G, S, m), x.shape))


def sigma_weights(sigma, lead, m, omitted=None):
    """The weights ``1 / sigma`` of problems of shape `lead` + (m,) — `lead` is (B,), or (G, S) for the data sets of
    global fits — and whether there is one set per problem.  `sigma` of shape `lead` + (m,), or of its last two or more
    axes ((S, m)), is always read as per problem: the weights come back in the full shape, with 1 for sigma wherever
    `omitted` (a mask of that shape, or None) is true — such a point is never read, anything may stand there.  A scalar
    gives the 0-d weight and (m,) the (m,) weights all problems share.  ValueError for another shape."""
    sg = np.asarray(sigma, dtype=np.float64)
    full = tuple(lead) + (m,)
    if sg.ndim >= 2 and sg.shape == full[-sg.ndim:]:
        sg = np.broadcast_to(sg, full)
        return 1.0 / (sg if omitted is None else np.where(omitted, 1.0, sg)), True
    if sg.size == 1:
        return 1.0 / sg.reshape(()), False
    if sg.shape != (m,):
        raise ValueError("`sigma` has incorrect shape.")
    return 1.0 / sg, False


class DeviceModel:
    """Model `name` (a name, a composite spec, a ``CompositeModel`` or an ``ExprModel``) with its data resident on the GPU: the device callbacks of ``OuterDriver.run_device``.

    Uploads t = xdata, y = ydata (None: 0, plain prediction) and w = 1 / sigma (None: 1; sigma a scalar, (m,) or
    (B, m)) once.  ``fun_dev(x_ptr, f_ptr, reps)`` and ``jac_dev(x_ptr, J_ptr, mask_ptr)`` launch the kernel on the
    context's stream — the stream of every driver on that context, so no synchronisation is needed in between.
    ``bounds_dev`` is the (lb_ptr, ub_ptr) pair the finite-difference route asks for, after ``set_bounds(lb, ub)``.
    ``close()`` frees the buffers (also run when the context closes).

    With a ``ParamMap`` (`param_map`, and the template `Pfix` (B, n) holding the values of its fixed parameters) the
    callbacks take the nf solver variables and go through blsq_model_eval_map_dev: ``n`` is then nf,
    the width of x and J, and ``n_model`` the number of model parameters; `set_bounds` takes reduced bounds.

    ``estimator='poisson'``: the callbacks give the deviance residuals of the counts `ydata` and their
    Jacobian, through blsq_model_eval_est_dev for every kind of model; `ydata` is then required and `sigma` must be
    None (ValueError).  The bounds must keep the model positive.

    ``binned=True``: the bin-integrated form of the model (``binned``).  `xdata` holds the bin edges in
    any form ``BinnedModel.check_xdata`` takes (checked on the host: finite, lo < hi) and is uploaded as rows; every
    kind of model and both estimators then go through blsq_model_eval_bin_dev.

    ``nan_policy='omit'`` (the default 'propagate' changes nothing): the points where `ydata` is NaN give
    residuals and Jacobian rows of exactly 0, inside the kernel, through blsq_model_eval_nan_dev for every kind of
    model; `ydata` is then required, and a `sigma` of shape (B, m) may hold anything at those points.

    ``global_map=`` a ``GlobalMap``: B groups of ``global_map.S`` data sets of `m` points each, every
    group one problem.  ``B`` is then the number of groups G, ``m`` becomes S m, ``n`` becomes nv (the width of x and
    J) and ``n_model`` stays the model's n; `xdata` is (m,), (S, m) or (G, S, m), `ydata` (G, S, m), `sigma` a scalar,
    (m,), (S, m) or (G, S, m), `Pfix` (G, S, n) (required where a parameter is fixed), `set_bounds` takes the reduced
    bounds, and the callbacks go through blsq_model_eval_global_dev alone.  `param_map` must be None (the map has its
    own), the model must have one coordinate and `binned` must be False (ValueError).

    Affine ties: where ``param_map.affine`` (``global_map.pm.affine``) is true the callbacks go through
    blsq_model_eval_tie_dev alone, whatever the other flags are, with the map's ``ratio`` and ``offset``; otherwise
    through the entry they went through before that one existed.

    ``response=`` a kernel (L,) or (B, L), with ``response_origin=``: the model convolved with it
    (``apply_response``, over the sample index).  The entry above is then bound as ``evaluate`` binds it — without
    `ydata`, `sigma`, the estimator and the omission — and writes raw model values and the raw Jacobian into two scratch
    buffers of this object; blsq_response_apply_dev, launched behind it on the same stream, convolves them and applies
    what was withheld.  One coordinate, no `global_map`, and `binned` with contiguous edges only (ValueError).

    An ``ExprModel``: the callbacks go through blsq_expr_eval_dev alone, with the program of
    ``model.bind(param_map)`` (fixed and tied parameters are leaves of the program: the entry takes no map), under
    every flag above but `binned` and `global_map` (ValueError).

    ``separable=True``: the linear parameters of the model (``linear_params``) are projected out.  ``n``
    is then the number of the others, the width of x and J, and ``n_model`` stays n; the entry above is bound as
    ``evaluate`` binds it and writes the raw Jacobian at unit linear parameters into a scratch buffer of this object,
    between blsq_varpro_expand_dev and blsq_varpro_reduce_dev on the same stream: three launches per evaluation, for
    ``fun_dev`` and ``jac_dev`` alike (f needs Phi too); `reps` must be 1.  ``linear_coefficients(x_ptr)`` runs the stage
    at x and returns c (B, nl), ``rank_info(x_ptr)`` its info flags.  `ydata` is required; `binned` and `sigma` compose;
    a map, the Poisson estimator, omission, `response` and an ``ExprModel`` are ValueErrors.

    ``separable=True`` with ``global_map=``: the ``GlobalMap`` over the NON-LINEAR parameters
    (``separable_global_map``).  B is the number of groups G, ``m`` becomes S m and ``n`` becomes nv, as for a global
    fit; `xdata`, `ydata` and `sigma` have its shapes.  An evaluation is blsq_varpro_expand_global_dev, the plain batch
    entry of the model on the G S data sets (raw, as above) and blsq_varpro_reduce_global_dev, which writes Kaufman's
    Jacobian straight into the group's layout; `reps` must be 1.  ``linear_coefficients(x_ptr)`` gives c (G, S, nl) and
    ``covariance_blocks(x_ptr, C_ptr, scale)`` the (G, S, n, n) blocks of the full covariance at x from the reduced
    covariance C [G][nv][nv] (blsq_varpro_cov_blocks_dev)."""

    def __init__(self, ctx, name, B, m, n, xdata, ydata=None, sigma=None, param_map=None, Pfix=None, estimator='lse',
                 binned=False, nan_policy='propagate', global_map=None, response=None, response_origin=0,
                 separable=False):
        model = resolve(name)
        model.terms(n)
        gm = global_map
        check_expr_model(model, binned)
        self.separable = bool(separable)
        if self.separable:
            self.lin, self.owner = check_separable(model, n, param_map, estimator, nan_policy, gm, response)
            if ydata is None:
                raise ValueError("`separable=True` needs `ydata`: the linear parameters are fitted to it.")
        if gm is not None:
            check_global(model, binned, param_map)
        self.response = None
        if response is not None:
            self.response, self.response_origin = check_response(response, response_origin, int(B))
            check_response_model(model, int(B), int(m), xdata, binned, gm)
        self.binned = bool(binned)
        self.estimator = check_estimator(estimator)
        self.nan_policy = check_nan_policy(nan_policy)
        if nan_policy == 'omit' and ydata is None:
            raise ValueError("nan_policy='omit' needs `ydata`: the missing points are its NaN.")
        if estimator == 'poisson':
            if ydata is None:
                raise ValueError("estimator='poisson' needs `ydata`: the counts.")
            if sigma is not None:
                raise ValueError("`sigma` must be None with estimator='poisson'.")
        self.model, self.B, self.n_model = model, int(B), int(n)
        self.param_map, self.global_map = param_map, gm
        sep_global = self.separable and gm is not None       # (its map is over the non-linear parameters: checked above)
        self._B_eval = self.B * gm.S if sep_global else self.B   # the problems of the model entry
        for what, mp in (("param_map", param_map), ("global_map", None if sep_global else gm)):
            if mp is not None and mp.n != self.n_model:
                raise ValueError("`%s` is for %d parameters, the model has %d." % (what, mp.n, self.n_model))
        # what a batch and a global model differ in: `m` stays the m of one data set, `self.m` is the problem's
        B, m = self.B, int(m)
        if gm is None:
            x, per_problem = (BinnedModel(model) if self.binned else model).check_xdata(xdata, B, m)
            self.t_stride = (2 if self.binned else 1) * model.coords * m if per_problem else 0
            self.t_sstride, lead, dims, pm, shared = 0, (B,), "B", param_map, None
            self.m, self.n = m, self.n_model if pm is None else pm.nf
            if self.separable:
                self.n = self.n_model - len(self.lin)
                if m <= len(self.lin):
                    raise ValueError("`separable=True` needs more points than linear parameters: m = %d, nl = %d."
                                     % (m, len(self.lin)))
        elif sep_global:                         # the model entry sees a plain batch of G S data sets
            x, _, sstride = global_xdata(xdata, B, gm.S, m)
            if sstride:
                x = np.ascontiguousarray(np.broadcast_to(x, (B, gm.S, m))).reshape(B * gm.S, m)
            self.t_stride, self.t_sstride = (m if sstride else 0), 0
            lead, dims, pm, shared = (B, gm.S), "G, S", None, None
            self.m, self.n = gm.S * m, gm.nv
            if m <= len(self.lin):
                raise ValueError("`separable=True` needs more points than linear parameters: m = %d, nl = %d."
                                 % (m, len(self.lin)))
        else:
            x, self.t_stride, self.t_sstride = global_xdata(xdata, B, gm.S, m)
            lead, dims, pm = (B, gm.S), "G, S", gm.pm
            shared = np.ascontiguousarray(gm.slot_shared, dtype=np.int32)
            self.m, self.n = gm.S * m, gm.nv
        y = w = None
        if ydata is not None:
            y = np.asarray(ydata, dtype=np.float64)
            if y.shape != lead + (m,):
                raise ValueError("`ydata` must have shape (%s, m)." % dims)
        self.w_stride = 0
        if sigma is not None:
            w, per_problem = sigma_weights(sigma, lead, m, np.isnan(y) if nan_policy == 'omit' else None)
            if per_problem:
                w, self.w_stride = w.reshape(B, self.m), self.m
            else:
                w = np.ascontiguousarray(np.broadcast_to(w, (m,)))
        self.ctx = ctx
        self._bufs = []
        self.d_t = self._upload(x)
        self.d_y = self._upload(None if y is None else np.ascontiguousarray(y.reshape(B, self.m)))
        self.d_w = self._upload(w)
        self.d_Pfix = None
        pmap = None if pm is None else np.ascontiguousarray(pm.pmap, dtype=np.int32)
        if pm is not None:
            if Pfix is None and np.any(pmap < 0):
                raise ValueError("`Pfix` is required when a parameter is fixed.")
            if Pfix is not None:
                Pfix = np.ascontiguousarray(Pfix, dtype=np.float64)
                if Pfix.shape != lead + (self.n_model,):
                    raise ValueError("`Pfix` must have shape (%s, n)." % dims)
                self.d_Pfix = self._upload(Pfix)
        self.bounds_dev = None
        self._bind(m, pm, pmap, shared)
        if self.response is not None:
            self._bind_response()
        if sep_global:
            self._bind_separable_global(m)
        elif self.separable:
            self._bind_separable()
        ctx.adopt(self)

    def _upload(self, a):
        if a is None:
            return None
        p = self.ctx.to_device(a)
        self._bufs.append(p)
        return p

    def set_bounds(self, lb, ub):
        self.bounds_dev = tuple(self._upload(np.ascontiguousarray(np.broadcast_to(a, (self.B, self.n)), dtype=np.float64))
                                for a in (lb, ub))
        return self.bounds_dev

    def _bind(self, m, pm, pmap, shared):
        """The entry of this fit and every argument it takes behind ctx, fixed once the data are uploaded (`self._eval`,
        made here, fills in reps, X, f, J and mask).  The entry is the one of the last flag the fit sets (it takes every kind of
        model and the flags before it); without a flag, the entry of the kind of model.  `m`: the points of one data
        set; `pm`: the ParamMap of the fit (a global fit's own) or None, `pmap` its int32 map; `shared`: the int32 flags of
        the slots a group shares, or None."""
        M, comp = self.model, isinstance(self.model, CompositeModel)
        gm = None if self.separable else self.global_map      # (a separable global fit binds the plain batch entry)
        # behind an instrument response or the projection of a separable fit the entry gives the raw model: data,
        # weights, estimator and omission are withheld
        estimator, nan_policy, d_y, d_w, w_stride = (
            (self.estimator, self.nan_policy, self.d_y, self.d_w, self.w_stride)
            if self.response is None and not self.separable else ('lse', 'propagate', None, None, 0))
        if isinstance(M, ExprModel):                          # the program behind the map, and the one entry that runs it
            prog = M.bind(pm).program
            ops, consts = np.ascontiguousarray(prog.ops, dtype=np.uint64), np.ascontiguousarray(prog.consts)
            self._host = (ops, consts)                        # the host arrays the entry reads: alive with the model
            a = [ESTIMATORS.index(estimator), NAN_POLICIES.index(nan_policy), self.B, 1, m, self.n, self.n_model,
                 M.coords, len(ops), ops.ctypes.data_as(_abi.C.POINTER(_abi.C.c_uint64)), int(prog.root), len(consts),
                 consts.ctypes.data_as(_abi.c_double_p), self.d_t, self.t_stride, d_y, d_w, w_stride, None, self.d_Pfix,
                 None, None, None]
            ctx = self.ctx

            def _eval(x_ptr, reps, f_ptr, J_ptr, mask_ptr):
                a[3] = int(reps)
                a[18] = x_ptr
                a[20:23] = f_ptr, J_ptr, mask_ptr
                ctx.check(ctx.lib.blsq_expr_eval_dev(ctx.h, *a), "blsq_expr_eval_dev")
            self._eval = _eval
            return
        if pm is not None and pm.affine:
            name = "blsq_model_eval_tie_dev"
        elif gm is not None:
            name = "blsq_model_eval_global_dev"
        elif nan_policy != 'propagate':
            name = "blsq_model_eval_nan_dev"
        elif self.binned:
            name = "blsq_model_eval_bin_dev"
        elif estimator != 'lse':
            name = "blsq_model_eval_est_dev"
        elif comp:                                            # with or without a map
            name = "blsq_model_eval_comp_dev"
        else:
            name = "blsq_model_eval_dev" if pm is None else "blsq_model_eval_map_dev"
        tie = name == "blsq_model_eval_tie_dev"
        ratio, offset = ((np.ascontiguousarray(a, dtype=np.float64) for a in (pm.ratio, pm.offset)) if tie
                         else (None, None))
        self._host = (pmap, shared, ratio, offset)            # the host arrays the entry reads: alive with the model

        def host(a, ptr_type=_abi.c_int32_p):
            return None if a is None else a.ctypes.data_as(ptr_type)
        values = dict(
            est=ESTIMATORS.index(estimator), sampling=SAMPLING.index('bin' if self.binned else 'point'),
            nan_policy=NAN_POLICIES.index(nan_policy), model=-1 if comp else M.id,
            ncomp=len(M.components) if comp else 0, fam=host(M.fam_ids) if comp else None,
            cnt=host(M.counts) if comp else None,
            S=0 if gm is None else gm.S, shared=host(shared), t_sstride=self.t_sstride,       # S == 0: a plain batch
            B=self._B_eval, reps=1, m=m, n=self.n_model,
            nf=(self.n_model if self.separable else self.n) if gm is None else gm.nf, pmap=host(pmap),   # nf: per data set
            tie_ratio=host(ratio, _abi.c_double_p), tie_offset=host(offset, _abi.c_double_p),
            t=self.d_t, t_stride=self.t_stride, y=d_y, w=d_w, w_stride=w_stride, X=None,
            Pfix=self.d_Pfix, f=None, J=None, mask=None)
        # strict: the entry chosen above has a slot for everything this fit sets, or this raises
        a, ctx = _abi.model_eval_args(name, values), self.ctx
        at_reps, at_x, at_f, at_J, at_mask = (_abi.MODEL_EVAL_ARGS[name].index(k) for k in ("reps", "X", "f", "J", "mask"))

        def _eval(x_ptr, reps, f_ptr, J_ptr, mask_ptr):       # twice per outer iteration: five stores and the call
            a[at_reps] = int(reps)
            a[at_x] = x_ptr
            a[at_f] = f_ptr
            a[at_J] = J_ptr
            a[at_mask] = mask_ptr
            ctx.check(getattr(ctx.lib, name)(ctx.h, *a), name)
        self._eval = _eval

    def _bind_response(self):
        """The second stage: h uploaded once, the scratch buffers g (grown to the largest `reps` seen) and G (B m n
        doubles, n the solver width; allocated by the first analytic Jacobian), and `self._eval` replaced by the pair of
        launches.  Both go onto the context's stream, so nothing synchronises in between."""
        ctx, inner, h = self.ctx, self._eval, self.response
        B, m, n = self.B, self.m, self.n
        L = h.shape[-1]
        d_h = self._upload(h)
        poisson = self.estimator == 'poisson'
        head = [ESTIMATORS.index(self.estimator), NAN_POLICIES.index(self.nan_policy), B]
        tail = [self.d_y, self.d_w, self.w_stride]
        self._g, self._g_reps, self._G = None, 0, None

        def scratch_g(reps):
            if reps > self._g_reps:                           # (blsq_dev_free waits for the work that reads the old one)
                if self._g is not None:
                    self._bufs.remove(self._g)
                    ctx.free(self._g)
                self._g = ctx.malloc(8 * B * reps * m)
                self._bufs.append(self._g)
                self._g_reps = reps
            return self._g

        def _eval(x_ptr, reps, f_ptr, J_ptr, mask_ptr):
            reps = int(reps)
            g = G = None
            if f_ptr is not None or poisson:                  # (c of the Poisson Jacobian is a function of mu)
                g = scratch_g(reps)
            if J_ptr is not None:
                if self._G is None:
                    self._G = ctx.malloc(8 * B * m * n)
                    self._bufs.append(self._G)
                G = self._G
            inner(x_ptr, reps, g, G, mask_ptr)
            ctx.check(ctx.lib.blsq_response_apply_dev(ctx.h, *head, reps, m, n, L, self.response_origin, d_h,
                                                      L if h.ndim == 2 else 0, g, G, *tail, f_ptr, J_ptr, mask_ptr),
                      "blsq_response_apply_dev")
        self._eval = _eval

    def _bind_separable(self):
        """The stages around the model kernel: the scratch buffers P (B, n) and G (B, m, n), and `self._eval` replaced
        by the three launches expand -> model kernel (Jacobian) -> reduce.  All go onto the context's stream, so nothing
        synchronises in between."""
        ctx, inner = self.ctx, self._eval
        B, m, n, nl = self.B, self.m, self.n_model, len(self.lin)
        lin, owner = (np.ascontiguousarray(a, dtype=np.int32) for a in (self.lin, self.owner))
        self._host_sep = (lin, owner)                         # the host arrays the entries read: alive with the model
        p_lin, p_owner = lin.ctypes.data_as(_abi.c_int32_p), owner.ctypes.data_as(_abi.c_int32_p)
        d_P, d_G = ctx.malloc(8 * B * n), ctx.malloc(8 * B * m * n)
        self._bufs += [d_P, d_G]
        tail = [self.d_y, self.d_w, self.w_stride]

        def _eval(x_ptr, reps, f_ptr, J_ptr, mask_ptr, c_ptr=None, info_ptr=None):
            if int(reps) != 1:
                raise ValueError("`separable=True` evaluates one point per problem: reps must be 1 (finite-difference "
                                 "Jacobians are not supported).")
            ctx.check(ctx.lib.blsq_varpro_expand_dev(ctx.h, B, n, nl, p_lin, x_ptr, d_P), "blsq_varpro_expand_dev")
            inner(d_P, 1, None, d_G, mask_ptr)
            ctx.check(ctx.lib.blsq_varpro_reduce_dev(ctx.h, B, m, n, nl, p_lin, p_owner, d_G, *tail, f_ptr, J_ptr, c_ptr,
                                                     info_ptr, mask_ptr), "blsq_varpro_reduce_dev")
        self._eval = _eval

    def _bind_separable_global(self, m):
        """As ``_bind_separable`` for G groups of S data sets of `m` points: P (G S, n) and G (G S, m, n),
        and expand-global -> model kernel on the G S data sets -> reduce-global, which writes J in the group's layout."""
        ctx, inner, gm = self.ctx, self._eval, self.global_map
        G, S, n, nl = self.B, gm.S, self.n_model, len(self.lin)
        lin, owner = (np.ascontiguousarray(a, dtype=np.int32) for a in (self.lin, self.owner))
        shared = np.zeros(n, dtype=np.int32)
        shared[np.flatnonzero(owner >= 0)[gm.shared_slots]] = 1
        self._host_sep = (lin, owner, shared)                 # the host arrays the entries read: alive with the model
        p_lin, p_owner, p_shared = (a.ctypes.data_as(_abi.c_int32_p) for a in self._host_sep)
        d_P, d_G = ctx.malloc(8 * G * S * n), ctx.malloc(8 * G * S * m * n)
        self._bufs += [d_P, d_G]
        tail = [self.d_y, self.d_w, self.w_stride]            # (w_stride: 0 or S m)
        self._layout_args = (G, S, n, nl, p_lin, p_shared)

        def _eval(x_ptr, reps, f_ptr, J_ptr, mask_ptr, c_ptr=None, info_ptr=None, Sinv_ptr=None, TD_ptr=None):
            if int(reps) != 1:
                raise ValueError("`separable=True` evaluates one point per problem: reps must be 1 (finite-difference "
                                 "Jacobians are not supported).")
            ctx.check(ctx.lib.blsq_varpro_expand_global_dev(ctx.h, G, S, n, nl, p_lin, p_shared, x_ptr, d_P),
                      "blsq_varpro_expand_global_dev")
            inner(d_P, 1, None, d_G, None)                    # (the mask is per group: every data set is evaluated)
            ctx.check(ctx.lib.blsq_varpro_reduce_global_dev(ctx.h, G, S, m, n, nl, p_lin, p_owner, p_shared, d_G, *tail,
                                                            f_ptr, J_ptr, c_ptr, info_ptr, Sinv_ptr, TD_ptr, mask_ptr),
                      "blsq_varpro_reduce_global_dev")
        self._eval = _eval

    def covariance_blocks(self, x_ptr, C_ptr, scale=None, status=None):
        """The blocks (G, S, n, n) of the full covariance of a separable global fit at the device vectors x [G][nv],
        from the covariance C [G][nv][nv] of the reduced group on the device: the stage is run at x for
        Sinv and TD, then blsq_varpro_cov_blocks_dev.  `scale` (G,) or None multiplies group g; `status` (G,) int or
        None: a group with a nonzero entry, like a data set that is rank deficient at x, gets NaN.  Returns
        ``(cov, c (G, S, nl), info (G, S))``."""
        if not (self.separable and self.global_map is not None):
            raise ValueError("the model was not opened with `separable=True` and a `global_map`.")
        ctx, gm = self.ctx, self.global_map
        G, S, n, nl, p_lin, p_shared = self._layout_args
        GS, na = G * S, n - nl
        bufs = [ctx.malloc(8 * GS * nl), ctx.malloc(4 * GS), ctx.malloc(8 * GS * nl * nl), ctx.malloc(8 * GS * nl * na),
                ctx.malloc(8 * GS * n * n)]
        d_c, d_info, d_Sinv, d_TD, d_cov = bufs
        try:
            d_scale = d_status = None
            if scale is not None:
                d_scale = ctx.to_device(np.ascontiguousarray(np.broadcast_to(scale, (G,)), dtype=np.float64))
                bufs.append(d_scale)
            if status is not None:
                d_status = ctx.to_device(np.ascontiguousarray(np.broadcast_to(status, (G,)), dtype=np.int32))
                bufs.append(d_status)
            self._eval(x_ptr, 1, None, None, None, c_ptr=d_c, info_ptr=d_info, Sinv_ptr=d_Sinv, TD_ptr=d_TD)
            ctx.check(ctx.lib.blsq_varpro_cov_blocks_dev(ctx.h, G, S, n, nl, p_lin, p_shared, C_ptr, d_Sinv, d_TD, d_scale,
                                                         d_info, d_status, d_cov), "blsq_varpro_cov_blocks_dev")
            ctx.sync()
            return (ctx.to_host(d_cov, (G, S, n, n), np.float64), ctx.to_host(d_c, (G, S, nl), np.float64),
                    ctx.to_host(d_info, (G, S), np.int32))
        finally:
            for p in bufs:
                ctx.free(p)

    def linear_coefficients(self, x_ptr, with_info=False):
        """c (B, nl) of a separable model at the device vectors x [B][n]: the stage is run there, because the driver's
        last evaluation may have been at a rejected trial point.  ``with_info=True``: ``(c, info)``, info (B,) int32
        with 1 where Phi is rank deficient at x (c is NaN there).  With a `global_map`: c (G, S, nl), info (G, S)."""
        if not self.separable:
            raise ValueError("the model was not opened with `separable=True`.")
        ctx, nl = self.ctx, len(self.lin)
        lead = (self.B,) if self.global_map is None else (self.B, self.global_map.S)
        B = int(np.prod(lead))
        d_c, d_info = ctx.malloc(8 * nl * B), ctx.malloc(4 * B)
        try:
            self._eval(x_ptr, 1, None, None, None, c_ptr=d_c, info_ptr=d_info)
            c = ctx.to_host(d_c, lead + (nl,), np.float64)
            return (c, ctx.to_host(d_info, lead, np.int32)) if with_info else c
        finally:
            ctx.free(d_c)
            ctx.free(d_info)

    def fun_dev(self, x_ptr, f_ptr, reps=1):
        self._eval(x_ptr, reps, f_ptr, None, None)

    def jac_dev(self, x_ptr, J_ptr, mask_ptr=None):
        self._eval(x_ptr, 1, None, J_ptr, mask_ptr)

    def close(self):
        bufs, self._bufs = getattr(self, "_bufs", []), []
        ctx = self.ctx
        if ctx is not None and getattr(ctx, "h", None):
            for p in bufs:
                ctx.free(p)
        self.bounds_dev = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DeviceFit:
    """What ``least_squares_batch(fun=...)`` takes in place of a callable for a fit whose callbacks run on the device:
    a checked (model, data) pair that opens a ``DeviceModel`` on the driver's context.  Built by ``curve_fit_batch``.
    ``n`` is the number of solver variables (the width of x0): the model's n, or nf of `param_map`; ``n_model`` is the
    model's number of parameters.  ``estimator='poisson'``, ``binned=True`` and ``nan_policy='omit'``: as
    ``DeviceModel``.  ``global_map=``: as ``DeviceModel``; `ydata` is (G, S, m), and ``B`` is G, ``m`` is S m and ``n``
    is nv.  ``response=``, ``response_origin=``: as ``DeviceModel`` (checked here, before any GPU is touched).
    ``separable=True``: as ``DeviceModel``; ``n`` is the number of non-linear parameters and ``lin`` / ``owner`` are
    those of ``linear_params``.  With ``global_map=`` as well: the map over the non-linear parameters;
    ``B`` is G, ``m`` is S m and ``n`` is nv."""

    def __init__(self, name, n, xdata, ydata, sigma=None, param_map=None, Pfix=None, estimator='lse', binned=False,
                 nan_policy='propagate', global_map=None, response=None, response_origin=0, separable=False):
        self.model = resolve(name)
        self.model.terms(n)
        gm = self.global_map = global_map
        check_expr_model(self.model, binned)
        self.separable = bool(separable)
        if self.separable:
            self.lin, self.owner = check_separable(self.model, n, param_map, estimator, nan_policy, gm, response)
        if gm is not None:
            check_global(self.model, binned, param_map)
        self.response, self.response_origin = None, 0
        if response is not None:
            check_response_model(self.model, 0, 0, None, False, gm)
            shape = np.shape(ydata)
            if len(shape) != 2:
                raise ValueError("`ydata` must have shape (B, m).")
            self.response, self.response_origin = check_response(response, response_origin, shape[0])
            check_response_model(self.model, shape[0], shape[1], xdata, binned, gm)
            self._xdata_given = xdata            # (contiguous edges stay recognisable to the DeviceModel's own check)
        self.binned = bool(binned)
        self.estimator = check_estimator(estimator)
        self.nan_policy = check_nan_policy(nan_policy)
        if estimator == 'poisson' and sigma is not None:
            raise ValueError("`sigma` must be None with estimator='poisson'.")
        self.ydata = np.ascontiguousarray(ydata, dtype=np.float64)
        if gm is None:
            self.B, self._m_set = self.ydata.shape            # (_m_set: the m of one data set)
        elif self.ydata.ndim != 3 or self.ydata.shape[1] != gm.S:
            raise ValueError("`ydata` must have shape (G, S, m).")
        else:
            self.B, _, self._m_set = self.ydata.shape
        self.n_model = int(n)
        self.param_map, self.Pfix = param_map, Pfix
        mp, what, dims = (param_map, "param_map", "B") if gm is None else (gm, "global_map", "G, S")
        if mp is not None and not (self.separable and gm is not None):    # (that map is over the non-linear ones)
            if mp.n != self.n_model:
                raise ValueError("`%s` is for %d parameters, the model has %d." % (what, mp.n, self.n_model))
            if gm is None or Pfix is not None:                # (a global fit needs it where a parameter is fixed)
                self.Pfix = np.ascontiguousarray(Pfix, dtype=np.float64)
                if self.Pfix.shape != self.ydata.shape[:-1] + (self.n_model,):
                    raise ValueError("`Pfix` must have shape (%s, n)." % dims)
        if gm is None:
            self.m, self.n = self._m_set, self.n_model if param_map is None else param_map.nf
            self.xdata = (BinnedModel(self.model) if self.binned else self.model).check_xdata(xdata, self.B, self.m)[0]
            if self.separable:
                self.n = self.n_model - len(self.lin)
                if self.m <= len(self.lin):
                    raise ValueError("`separable=True` needs more points than linear parameters: m = %d, nl = %d."
                                     % (self.m, len(self.lin)))
        else:
            self.m, self.n = gm.S * self._m_set, gm.nv
            self.xdata = global_xdata(xdata, self.B, gm.S, self._m_set)[0]
            if self.separable and self._m_set <= len(self.lin):
                raise ValueError("`separable=True` needs more points than linear parameters: m = %d, nl = %d."
                                 % (self._m_set, len(self.lin)))
        self.sigma = sigma

    def open_device(self, ctx, lb, ub):
        xdata = self.xdata if self.response is None else self._xdata_given
        dm = DeviceModel(ctx, resolvable(self.model), self.B, self._m_set, self.n_model, xdata, self.ydata, self.sigma,
                         self.param_map, self.Pfix, self.estimator, self.binned, self.nan_policy, self.global_map,
                         **({} if self.response is None
                            else {'response': self.response, 'response_origin': self.response_origin}),
                         **({'separable': True} if self.separable else {}))
        dm.set_bounds(lb, ub)
        return dm


def evaluate(name, xdata, P, ctx=None, binned=False, response=None, response_origin=0):
    """Predictions ``model(xdata; P[b])`` of shape (B, m), computed on the GPU (the kernel with y = NULL, w = NULL).
    P: (B, n); xdata: (m,) / (B, m), or (2, m) / (B, 2, m) for 'gauss2d'.  `name`: a name, a composite spec, a
    ``CompositeModel`` or an ``ExprModel`` (xdata (C, m) / (B, C, m) for its C > 1 coordinates).  ``binned=True``: the
    bin contents of the bin-integrated model; `xdata` is then the m + 1 contiguous edges (1-D) or rows (2, m) /
    (B, 2, m) — (4, m) / (B, 4, m) for 'gauss2d' — as ``BinnedModel.f`` takes them.  ``response=`` (L,) or (B, L) with ``response_origin=``: the prediction convolved with the kernel, over the
    sample index (``apply_response``): what a fit with the same keywords compares with its data."""
    model = resolve(name)
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim != 2:
        raise ValueError("`P` must have shape (B, n).")
    B, n = P.shape
    model.terms(n)
    x = np.asarray(xdata, dtype=np.float64)
    if x.ndim < 1 or x.shape[-1] == 0:
        raise ValueError("`xdata` must not be empty.")
    m = x.shape[-1]
    edges = x                                    # (contiguous edges as given: what a response needs to see)
    if binned:
        if x.ndim == 1 and model.coords == 1:
            x = bin_rows(x)
            m = x.shape[-1]
        BinnedModel(model).check_xdata(x, B, m)
    else:
        model.check_xdata(x, B, m)
    resp = {}
    if response is not None:
        h, origin = check_response(response, response_origin, B)
        check_response_model(model, B, m, edges, binned)
        resp = {'response': h, 'response_origin': origin}
        x = edges
    own = ctx is None
    if own:
        ctx = _abi.Context(0)
    try:
        with DeviceModel(ctx, resolvable(model), B, m, n, x, **({'binned': True} if binned else {}), **resp) as dm:
            d_P = ctx.to_device(P)
            d_f = ctx.malloc(8 * B * m)
            try:
                dm.fun_dev(d_P, d_f, 1)
                return ctx.to_host(d_f, (B, m), np.float64)
            finally:
                ctx.free(d_P)
                ctx.free(d_f)
    finally:
        if own:
            ctx.close()
