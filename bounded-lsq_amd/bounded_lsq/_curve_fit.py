"""`curve_fit`, `curve_fit_batch` and `curve_fit_global`: scipy.optimize.curve_fit's model-fitting front end over this
package's solvers.

``curve_fit`` follows scipy 1.15.3 ``_minpack_py.py::curve_fit`` line by line where its lines apply (the comments cite
them); the solve is this package's ``least_squares`` and ``pcov`` is the pseudo-inverse covariance of the final Jacobian
computed on the GPU (``covariance='pinv'``) where scipy takes an SVD on the host.
"""
import warnings
from collections import namedtuple
from inspect import getfullargspec, signature

import numpy as np
from scipy.linalg import cholesky, solve_triangular, LinAlgError
from scipy.optimize import OptimizeWarning

from ._frontend import least_squares
from ._batch import least_squares_batch
from ._hostmath import prepare_bounds, _initialize_feasible
from . import _models
from ._params import ParamMap, GlobalMap

__all__ = ['curve_fit', 'curve_fit_batch', 'curve_fit_global']

_COV_WARNING = 'Covariance of the parameters could not be estimated'


def _memoize_first(fn):
    """scipy's _lightweight_memoizer: remember the value at the first parameter vector only (the solver and the
    finite-difference Jacobian both evaluate there), and stop looking once another vector has been seen."""
    state = {"params": None, "val": None, "skip": False}

    def wrapped(params):
        if state["skip"]:
            return fn(params)
        if np.all(state["params"] == params):
            return state["val"]
        if state["params"] is not None:
            state["skip"] = True
        val = fn(params)
        if state["params"] is None:
            state["params"] = np.copy(params)
            state["val"] = val
        return val
    return wrapped


def _transform_of(sigma, ysize):
    """None, 1 / sigma (scalar or 1-D errors) or the lower Cholesky factor of a 2-D covariance."""
    if sigma is None:
        return None
    sigma = np.asarray(sigma)
    if sigma.size == 1 or sigma.shape == (ysize,):
        return 1.0 / sigma
    if sigma.shape == (ysize, ysize):
        try:
            return cholesky(sigma, lower=True)
        except LinAlgError as e:
            raise ValueError("`sigma` must be positive definite.") from e
    raise ValueError("`sigma` has incorrect shape.")


def _wrap_func(f, xdata, ydata, transform):
    if transform is None:
        return lambda params: f(xdata, *params) - ydata
    if transform.size == 1 or transform.ndim == 1:
        return lambda params: transform * (f(xdata, *params) - ydata)
    # chi^2 = r^T C^-1 r with C = L L^T: minimise |L^-1 r|^2
    return lambda params: solve_triangular(transform, f(xdata, *params) - ydata, lower=True)


def _wrap_jac(jac, xdata, transform):
    if transform is None:
        return lambda params: jac(xdata, *params)
    if transform.ndim == 0:                  # (a scalar sigma: scipy's wrapper sends it to the triangular solve)
        return lambda params: transform * np.asarray(jac(xdata, *params))
    if transform.ndim == 1:
        return lambda params: transform[:, np.newaxis] * np.asarray(jac(xdata, *params))
    return lambda params: solve_triangular(transform, np.asarray(jac(xdata, *params)), lower=True)


def _check_poisson(estimator, sigma, ydata, omitted=None):
    """True for estimator='poisson' (after its checks of `sigma` and `ydata`), False for 'lse'; ValueError otherwise.
    omitted: the mask of the points ``nan_policy='omit'`` leaves out; the counts are checked at the kept points only."""
    if _models.check_estimator(estimator) == 'lse':
        return False
    if sigma is not None:
        raise ValueError("`sigma` must be None with estimator='poisson': the counts carry their own variance.")
    if omitted is not None:
        ydata = ydata[~omitted]
    if not np.all(np.isfinite(ydata)):
        raise ValueError("`ydata` must be finite with estimator='poisson'.")
    if np.any(ydata < 0):
        raise ValueError("`ydata` must not be negative with estimator='poisson': it holds counts.")
    return True


def _response_single(f, jac, xdata, ydata, sigma, nan_policy, response, response_origin):
    """``curve_fit`` through an instrument response: `f` and a callable `jac` wrapped so that they return the convolved
    model, with `f`'s signature kept (p0=None counts its arguments).  Under 'omit' the wrappers evaluate on the whole
    grid and drop the NaN points of `ydata` after the convolution; the data are shortened here to match."""
    h, origin = _models.check_response(response, response_origin)
    if h.ndim != 1:
        raise ValueError("`response` must have shape (L,) in `curve_fit`: there is one problem.")
    keep = None
    if nan_policy == 'omit':
        y = np.asarray(ydata, float)
        if isinstance(xdata, (list, tuple, np.ndarray)) and np.isnan(np.asarray(xdata, float)).any():
            raise ValueError("`xdata` must not contain NaN with `response` and nan_policy='omit': the model is "
                             "evaluated on the whole grid.")
        if y.ndim == 1 and np.isnan(y).any():
            keep = ~np.isnan(y)
    x_full, user_f, user_jac = xdata, f, jac

    def fc(x, *params):
        mu = _models.apply_response(np.asarray(user_f(x_full, *params), float), h, origin)
        return mu if keep is None else mu[keep]
    fc.__signature__ = signature(user_f)
    jc = jac
    if callable(jac):
        def jc(x, *params):
            J = _models.apply_response(np.asarray(user_jac(x_full, *params), float).T, h, origin).T
            return J if keep is None else J[keep]
    if keep is not None:
        ydata = y[keep]
        if isinstance(xdata, (list, tuple, np.ndarray)):
            xdata = np.asarray(xdata, float)[..., keep]      # (the wrappers do not read it: x_full is the grid)
        if sigma is not None:
            sigma = np.asarray(sigma)
            if sigma.ndim == 1:
                sigma = sigma[keep]
            elif sigma.ndim == 2:
                sigma = sigma[keep][:, keep]
    return fc, jc, xdata, ydata, sigma


def _param_map(n, fixed, tied):
    """The ParamMap of the `fixed` / `tied` keywords, or None where they hold nothing (then nothing changes)."""
    if fixed is None and not tied:
        return None
    pm = ParamMap(n, fixed, tied)
    return None if pm.identity else pm


_NAN_POLICIES = [None, 'raise', 'omit']                  # scipy's list for curve_fit


def _contains_nan(a, nan_policy):
    """scipy's _contains_nan for a float array and curve_fit's policies: its exceptions, in its words."""
    if nan_policy not in _NAN_POLICIES:
        raise ValueError(f"nan_policy must be one of {set(_NAN_POLICIES)}.")
    contains_nan = bool(a.size) and bool(np.isnan(np.max(a)))
    if contains_nan and nan_policy == 'raise':
        raise ValueError("The input contains nan values")
    return contains_nan


def curve_fit(f, xdata, ydata, p0=None, sigma=None, absolute_sigma=False, check_finite=None,
              bounds=(-np.inf, np.inf), method=None, jac=None, full_output=False, fixed=None, tied=None,
              estimator='lse', nan_policy=None, response=None, response_origin=0, **kwargs):
    """Fit ``ydata = f(xdata, *p) + eps`` by non-linear least squares; returns ``(popt, pcov)``.

    Parameters, exceptions, warnings and results are scipy.optimize.curve_fit's (1.15.3):
    p0 None takes the number of parameters from the signature of `f` and starts from 1 (or inside finite bounds);
    sigma may be a scalar, 1-D errors or a 2-D covariance (its Cholesky factor is solved against on the host);
    the residual is ``transform * (f(xdata, *p) - ydata)``, a callable `jac` is transformed the same way and
    ``jac=None`` means '2-point'; ``maxfev`` is renamed to ``max_nfev``; 'args' in kwargs is a ValueError; an
    unsuccessful solve raises ``RuntimeError("Optimal parameters not found: ...")``.  Other keywords go to this
    package's ``least_squares`` (``loss=``, ``f_scale=``, tolerances, ``scaling``, ``options``).

    ``pcov`` is the Moore-Penrose covariance of the final Jacobian over its singular values above
    ``eps * max(m, n) * s_max``, computed on the GPU; unless `absolute_sigma` it is multiplied by
    ``obj_value / (m - n)``, and filled with inf under an ``OptimizeWarning`` where m <= n.
    ``full_output=True`` returns ``(popt, pcov, infodict, mesg, ier)`` with infodict keys ``nfev`` and ``fvec``, and
    ``leverage`` (``least_squares``'s, of the transformed Jacobian) when ``leverage=True`` is among the keywords.

    One deliberate difference from scipy: ``method=None`` always means 'trf' (scipy chooses 'lm' for an unbounded
    problem); ``method='lm'`` raises ``NotImplementedError`` here as in ``least_squares``: there is no MINPACK bridge on
    this step path.

    check_finite, nan_policy : scipy's pair.  `check_finite` None (the default) means True unless a `nan_policy` is
    given.  `nan_policy` None leaves NaN to `check_finite`; 'raise' raises ``ValueError("The input contains nan
    values")`` for a NaN in `xdata` or `ydata`; 'omit' drops the points where either is NaN before the fit, and the
    matching entries of a 1-D `sigma` or rows and columns of a 2-D one (one problem: the points are dropped on the host,
    ``curve_fit_batch`` omits them inside the kernel); 'propagate' is not supported, as in scipy.

    fixed, tied : hold parameters at their `p0` (a boolean mask (n,) or indices) and make parameter j a copy of
    parameter i (``{j: i}``; ``{j: (i, ratio, offset)}``: p_j = ratio * p_i + offset), as ``curve_fit_batch``; `p0` is
    then required (ValueError).  `f` and a callable `jac`
    still take and return all n parameters; the solver works on the nf remaining variables (``jac=None`` differentiates
    those), `popt` (n,) has the fixed values and tied copies filled in, `pcov` (n, n) has zero rows and columns for
    fixed parameters and copied ones for tied parameters, and the degrees of freedom are m - nf.

    estimator : 'lse' (the default: everything above) or 'poisson': the Poisson maximum-likelihood fit of counts
    ``ydata >= 0``, as ``curve_fit_batch`` describes it (deviance residuals in ``fvec``; `sigma` must be None; the
    bounds must keep `f` positive; `absolute_sigma` True gives the Gauss-Newton form of the inverse Fisher information,
    False the quasi-Poisson covariance).  A callable `jac` is still the Jacobian of `f`.

    response, response_origin : a measured kernel (L,) the model is convolved with before it is compared with `ydata`
    (``models.apply_response``: over the sample index, zeros past both ends), as ``curve_fit_batch`` describes it.  `f`
    and a callable `jac` still return the model and ITS Jacobian.  With ``nan_policy='omit'`` the model is evaluated and
    convolved on the whole grid and the points where `ydata` is NaN are dropped afterwards; `xdata` must then be free of
    NaN.
    """
    _models.check_estimator(estimator)
    if response is not None:
        f, jac, xdata, ydata, sigma = _response_single(f, jac, xdata, ydata, sigma, nan_policy, response,
                                                       response_origin)
    pm = None
    if fixed is not None or tied:
        if p0 is None:
            raise ValueError("`p0` is required with `fixed` or `tied`.")
        pm = _param_map(np.atleast_1d(p0).size, fixed, tied)
    if pm is not None:
        return _curve_fit_mapped(pm, f, xdata, ydata, p0, sigma, absolute_sigma, check_finite, bounds, method, jac,
                                 full_output, estimator, kwargs, nan_policy)
    if p0 is None:
        args = getfullargspec(f).args
        if len(args) < 2:
            raise ValueError("Unable to determine number of fit parameters.")
        n = len(args) - 1
    else:
        p0 = np.atleast_1d(p0)
        n = p0.size

    if hasattr(bounds, 'lb') and hasattr(bounds, 'ub'):      # a scipy.optimize.Bounds instance
        bounds = (bounds.lb, bounds.ub)
    lb, ub = prepare_bounds(bounds, np.empty(n))
    if p0 is None:
        p0 = _initialize_feasible(lb, ub)

    if method is None:
        method = 'trf'
    if method == 'lm':
        raise NotImplementedError(
            "method='lm' is a MINPACK bridge in the reference and is outside "
            "the MI355X step path; use 'trf' or 'dogbox'.")

    if check_finite is None:
        check_finite = True if nan_policy is None else False

    # optimisation may produce garbage for float32 inputs: cast to float64
    ydata = np.asarray_chkfinite(ydata, float) if check_finite else np.asarray(ydata, float)
    if isinstance(xdata, (list, tuple, np.ndarray)):
        # `xdata` goes straight to `f`, so anything that is not array_like is left alone
        xdata = np.asarray_chkfinite(xdata, float) if check_finite else np.asarray(xdata, float)
    if ydata.size == 0:
        raise ValueError("`ydata` must not be empty!")

    # nan handling is needed only if check_finite is False: otherwise the data hold none
    if not check_finite and nan_policy is not None:
        if nan_policy == "propagate":
            raise ValueError("`nan_policy='propagate'` is not supported by this function.")
        x_contains_nan = _contains_nan(np.asarray(xdata, float), nan_policy)
        y_contains_nan = _contains_nan(ydata, nan_policy)
        if (x_contains_nan or y_contains_nan) and nan_policy == 'omit':
            has_nan = np.isnan(xdata)
            has_nan = has_nan.any(axis=tuple(range(has_nan.ndim - 1)))
            has_nan |= np.isnan(ydata)
            xdata = xdata[..., ~has_nan]
            ydata = ydata[~has_nan]
            if sigma is not None:                # the corresponding entries of sigma
                sigma = np.asarray(sigma)
                if sigma.ndim == 1:
                    sigma = sigma[~has_nan]
                elif sigma.ndim == 2:
                    sigma = sigma[~has_nan, :]
                    sigma = sigma[:, ~has_nan]

    if _check_poisson(estimator, sigma, ydata):
        # the deviance residual of the counts and its Jacobian c * J (models.poisson_transform)
        def mu_of(params):
            return np.asarray(f(xdata, *params), float)
        func = _memoize_first(lambda params: _models.poisson_transform(mu_of(params), ydata)[0])
        if callable(jac):
            user_jac = jac
            jac = _memoize_first(lambda params: _models.poisson_transform(mu_of(params), ydata)[1][:, np.newaxis]
                                 * np.asarray(user_jac(xdata, *params)))
    else:
        transform = _transform_of(sigma, ydata.size)
        func = _memoize_first(_wrap_func(f, xdata, ydata, transform))
        if callable(jac):
            jac = _memoize_first(_wrap_jac(jac, xdata, transform))
    if jac is None:
        jac = '2-point'

    if 'args' in kwargs:
        # the model function takes xdata and the parameters, nothing else
        raise ValueError("'args' is not a supported keyword argument.")
    if 'max_nfev' not in kwargs:
        kwargs['max_nfev'] = kwargs.pop('maxfev', None)

    # the bound checks of scipy's least_squares, in its words (this package's least_squares keeps the reference's)
    if lb.shape == p0.shape and ub.shape == p0.shape:
        if np.any(lb >= ub):
            raise ValueError("Each lower bound must be strictly less than each upper bound.")
        if not np.all((p0 >= lb) & (p0 <= ub)):
            raise ValueError("Initial guess is outside of provided bounds")

    res = least_squares(func, p0, jac=jac, bounds=bounds, method=method, covariance='pinv', **kwargs)
    if not res.success:
        raise RuntimeError("Optimal parameters not found: " + res.message)

    infodict = dict(nfev=res.nfev, fvec=res.fun)
    if 'leverage' in res:
        infodict['leverage'] = res.leverage
    ier, errmsg = res.status, res.message
    ysize = len(res.fun)
    cost = res.obj_value                     # sum f^2, or the robust-loss objective (scipy: 2 * res.cost)
    popt = res.x
    pcov = res.x_covariance                  # V diag(1 / s^2) V^T over the kept singular values

    warn_cov = False
    if pcov is None or np.isnan(pcov).any():
        pcov = np.full((len(popt), len(popt)), np.inf)
        warn_cov = True
    elif not absolute_sigma:
        if ysize > p0.size:
            pcov = pcov * (cost / (ysize - p0.size))
        else:
            pcov.fill(np.inf)
            warn_cov = True
    if warn_cov:
        warnings.warn(_COV_WARNING, category=OptimizeWarning, stacklevel=2)

    if full_output:
        return popt, pcov, infodict, errmsg, ier
    return popt, pcov


def _curve_fit_mapped(pm, f, xdata, ydata, p0, sigma, absolute_sigma, check_finite, bounds, method, jac, full_output,
                      estimator, kwargs, nan_policy=None):
    """``curve_fit`` over the nf variables of `pm`: the same function on wrapped callables, results expanded."""
    Pfix = np.array(np.atleast_1d(p0), dtype=float)
    if hasattr(bounds, 'lb') and hasattr(bounds, 'ub'):
        bounds = (bounds.lb, bounds.ub)
    lb, ub = prepare_bounds(bounds, np.empty(pm.n))
    if lb.shape != (pm.n,) or ub.shape != (pm.n,):
        raise ValueError("Inconsistent shapes between bounds and `p0`.")
    lbr, ubr = pm.reduce_bounds(lb, ub)

    def fr(x, *xv):
        return f(x, *pm.expand_x(np.asarray(xv, dtype=float), Pfix))
    jr = jac
    if callable(jac):
        def jr(x, *xv):
            return pm.reduce_jac(np.asarray(jac(x, *pm.expand_x(np.asarray(xv, dtype=float), Pfix))))
    out = curve_fit(fr, xdata, ydata, p0=pm.reduce_x(Pfix), sigma=sigma, absolute_sigma=absolute_sigma,
                    check_finite=check_finite, bounds=(lbr, ubr), method=method, jac=jr, full_output=full_output,
                    estimator=estimator, nan_policy=nan_policy, **kwargs)
    return (pm.expand_x(out[0], Pfix), pm.expand_cov(out[1])) + tuple(out[2:])


# What `_fit` needs to know of its caller's data: `lead` (B,) or (G, S), the shape in front of the m points of one data
# set (with m: the shapes a per-problem `sigma` may have); `Y` (problems, rows), one row per problem of the solver;
# `P0` lead + (n,), the start and the template of the map; `make_map` () -> ParamMap, GlobalMap or None;
# `xdata` (xdata, model or None) -> (what a callable receives, what the device receives); and the texts that differ.
_Layout = namedtuple('_Layout', 'lead m Y P0 make_map xdata none_left propagate_hint sigma_2d')


def _fit(lay, f, xdata, sigma, absolute_sigma, bounds, method, jac, driver, ctx, estimator, binned, nan_policy, kwargs,
         response=None, response_origin=0):
    """``curve_fit_batch`` and ``curve_fit_global`` between their shape checks and their results: the checks of the
    keywords in their order, the residual and Jacobian of the solver's variables (on the device: a ``DeviceFit``) and
    the solve.  Returns ``(results, map, no_dof)``: `results` with ``nobs`` / ``omitted`` and ``deviance`` set,
    `no_dof` (problems,) true where the covariance has no variance factor to be scaled by."""
    problems, rows = lay.Y.shape
    Y, P0 = lay.Y, lay.P0
    ydata = Y.reshape(lay.lead + (lay.m,))
    n = P0.shape[-1]
    omitted = nobs = None
    if nan_policy == 'raise':
        if np.isnan(ydata).any():
            raise ValueError("The input contains nan values")
    elif nan_policy == 'omit':
        omitted = np.isnan(ydata)
        kept = np.sum(~omitted, axis=-1)
        if not kept.all():
            raise ValueError(lay.none_left % tuple(int(i) for i in np.argwhere(kept == 0)[0][::-1]))
        nobs = kept.reshape(problems, -1).sum(axis=1).astype(np.int32)
    elif nan_policy is not None:
        raise ValueError("`nan_policy` must be None, 'raise' or 'omit', not %r%s." % (
            nan_policy, lay.propagate_hint if nan_policy == 'propagate' else ""))
    poisson = _check_poisson(estimator, sigma, ydata, omitted)
    mp = lay.make_map()
    model = None
    if response is not None:                     # (curve_fit_batch alone passes one: `lead` is (B,))
        response, response_origin = _models.check_response(response, response_origin, problems)
        _models.check_response_model(
            _models.resolve(f) if isinstance(f, (str, _models.CompositeModel, _models.ExprModel)) else None,
            problems, lay.m, xdata, binned)
    if binned and not isinstance(f, (str, _models.CompositeModel, _models.ExprModel)):
        raise ValueError("`binned=True` needs a built-in model (a name, a spec or a CompositeModel) as `f`: a callable "
                         "integrates itself over its bins.")
    if isinstance(f, _models.ExprModel):         # (before any GPU is touched)
        _models.check_expr_model(f, binned, isinstance(mp, GlobalMap))
    if isinstance(f, (str, _models.CompositeModel, _models.ExprModel)):
        model = _models.resolve(f)
        model.terms(n)
        host_model = _models.binned(model) if binned else model         # whose numpy functions driver='host' calls
        x_host, x_dev = lay.xdata(xdata, host_model)
        if callable(jac):
            raise ValueError("a callable `jac` cannot be combined with the built-in model '%s'." % model.name)
        if jac is not None and jac not in ('2-point', '3-point'):
            raise ValueError("`jac` must be None, '2-point' or '3-point' with a built-in model.")
        if driver not in ('host', 'device'):
            raise ValueError("`driver` must be 'host' or 'device'.")
        if driver == 'host':                     # the numpy functions through the callable path below
            f = host_model.f
            if jac is None:
                jac = host_model.jac
    else:
        x_host, x_dev = lay.xdata(xdata, None)
        if jac is None:
            jac = '2-point'

    transform = None
    if sigma is not None:
        sigma = np.asarray(sigma, float)
        try:
            w, per_problem = _models.sigma_weights(sigma, lay.lead, lay.m, omitted)
        except ValueError:
            if lay.sigma_2d is None or sigma.ndim != 2:
                raise
            raise ValueError(lay.sigma_2d) from None
        # along the rows of a problem; a scalar stays one (numpy multiplies by it in one flat loop)
        transform = w.reshape(problems, rows) if per_problem else np.tile(w, rows // lay.m) if w.ndim else w

    if mp is not None:                           # the solver sees nf (nv) variables; f and jac see all n
        if len(bounds) != 2:
            raise ValueError("`bounds` must contain 2 elements.")
        bounds = mp.reduce_bounds(np.broadcast_to(np.asarray(bounds[0], dtype=float), P0.shape),
                                  np.broadcast_to(np.asarray(bounds[1], dtype=float), P0.shape))
        x_start = mp.reduce_x(P0)
        if callable(f):
            f = mp.wrap_f(f, P0)
        if callable(jac):
            jac = mp.wrap_jac(jac, P0)
    else:
        x_start = P0
    nv = x_start.shape[1]                        # solver variables: n, nf, or nv of a group

    on_device = model is not None and driver == 'device'
    if response is not None and not on_device:   # after the map's column sums, before the data: the device's order
        if callable(jac):
            jac = _models.response_jacobian(jac, response, response_origin)
        f = _models.response_residual(f, response, response_origin)

    if on_device:
        func = _models.DeviceFit(_models.resolvable(model), n, xdata if (binned and response is not None) else x_dev,
                                 ydata, sigma,
                                 Pfix=None if mp is None else P0,
                                 **{'global_map' if isinstance(mp, GlobalMap) else 'param_map': mp},
                                 **({} if response is None
                                    else {'response': response, 'response_origin': response_origin}),
                                 **({'estimator': estimator} if poisson else {}),
                                 **({'binned': True} if binned else {}),
                                 **({'nan_policy': 'omit'} if omitted is not None else {}))
    elif poisson:                                # (after the map: c multiplies the summed columns)
        if callable(jac):
            jac = _models.poisson_jacobian(f, jac, Y)
        f_res = _models.poisson_residual(f, Y)

        def func(X):
            return np.asarray(f_res(x_host, X), float)
    elif transform is None:
        def func(X):
            return np.asarray(f(x_host, X), float) - Y
    else:
        def func(X):
            return transform * (np.asarray(f(x_host, X), float) - Y)

    if callable(jac):
        user_jac = jac
        tj = None if transform is None else np.broadcast_to(transform, (problems, rows))[:, :, np.newaxis]

        def jac(X):                                                        # noqa: F811
            J = np.asarray(user_jac(x_host, X), float)
            return J if tj is None else tj * J

    if omitted is not None and callable(func):   # outermost: after sigma, the Poisson transform and the map
        func = _models.omit_residual(func, Y)
        if callable(jac):
            jac = _models.omit_jacobian(jac, Y)

    if 'args' in kwargs:
        raise ValueError("'args' is not a supported keyword argument.")
    if 'max_nfev' not in kwargs:
        kwargs['max_nfev'] = kwargs.pop('maxfev', None)

    scale_on_gpu = (not absolute_sigma) and rows > nv
    results = least_squares_batch(func, x_start, jac, bounds=bounds, method=method, driver=driver, ctx=ctx,
                                  covariance='pinv', _variance_scale=scale_on_gpu,
                                  **({'_nobs': nobs} if nobs is not None else {}), **kwargs)
    for b, r in enumerate(results):
        if nobs is not None:
            r.nobs, r.omitted = int(nobs[b]), omitted[b].copy()
        if poisson:
            r.deviance = float(np.dot(r.fun, r.fun))
    points = np.full(problems, rows) if nobs is None else nobs
    return results, mp, (points <= nv) & (not absolute_sigma)


def _popt_pcov(results, shape, no_dof, popt_of, pcov_of):
    """`popt` of `shape` and `pcov` from the results of the solve: NaN rows for a problem that did not converge, inf
    under the ``OptimizeWarning`` where the covariance is missing, holds NaN or has no degree of freedom (`no_dof`)."""
    popt = np.full(shape, np.nan)
    pcov = np.full(shape + shape[-1:], np.nan)
    warn_cov = False
    for b, r in enumerate(results):
        if not r.success:
            continue
        C = r.x_covariance
        popt[b] = popt_of(r)
        if C is None or np.isnan(C).any() or no_dof[b]:
            pcov[b] = np.inf
            warn_cov = True
        else:
            pcov[b] = pcov_of(C)
    if warn_cov:
        warnings.warn(_COV_WARNING, category=OptimizeWarning, stacklevel=3)
    return popt, pcov


def curve_fit_batch(f, xdata, ydata, p0, sigma=None, absolute_sigma=False, bounds=(-np.inf, np.inf), method='trf',
                    jac=None, driver='host', ctx=None, fixed=None, tied=None, estimator='lse', binned=False,
                    nan_policy=None, response=None, response_origin=0, separable=False, **kwargs):
    """``curve_fit`` for B data sets of one model, solved together by ``least_squares_batch``.

    f : ``f(xdata, P) -> (B, m)`` for parameters ``P`` of shape (B, n): vectorised over the batch — or the name of a
        built-in model (``bounded_lsq.models``: 'poly', 'exp_sum', 'gauss_sum', 'lorentz_sum', 'gauss2d'; n = p0.shape[1]
        fixes the number of terms) — or a composite: a spec such as 'gauss*2+lorentz+poly*2' (``models.compose``: a sum
        of gauss / lorentz / pvoigt / exp terms and polynomials, whose n the spec fixes) or a ``CompositeModel``,
        treated exactly as a name — or an ``ExprModel``: a formula of the caller's own, ``models.expression('a*exp(-t/tau)+c',
        ('a', 'tau', 'c'))`` (interpreted on the GPU by a kernel of its own, with the exact Jacobian;
        `xdata` (C, m) or (B, C, m) for its C > 1 coordinates; every keyword below but ``binned=True``, which is a
        ValueError with it).  A named model with driver='device' is evaluated on the GPU, residuals and
        Jacobians alike: between the start of the solve and its results only two counters per iteration leave the
        device.  With driver='host' the model's numpy functions are the callbacks.  `xdata` is then (m,) or (B, m)
        — (2, m) or (B, 2, m) for 'gauss2d'.  A wrong name, an n that does not fit the model or a wrong `xdata` shape
        is a ValueError.
    ydata : (B, m);  p0 : (B, n), required
    sigma : None, a scalar, (m,) errors shared by all problems or (B, m) per problem (a shape (B, m) is always read
            this way).  A 2-D covariance is not supported here: ValueError.
    bounds : pair broadcastable to (B, n);  jac : '2-point', '3-point' or ``jac(xdata, P) -> (B, m, n)``; None (the
            default) is '2-point' for a callable `f` and the analytic Jacobian for a named model, whose '2-point' /
            '3-point' are estimated on the device from the kernel's values (a callable `jac` with a name: ValueError)
    driver, ctx, **kwargs : as ``least_squares_batch`` (tolerances, ``max_nfev`` / ``maxfev``, ``loss=``, ...).
    fixed : None, a boolean mask (n,) or a sequence of indices, shared by all problems: parameter j of problem b is
            held at ``p0[b, j]`` (its bounds are ignored).
    tied : None or ``{j: i}``: parameter j is a copy of parameter i (its own `p0` is ignored; the box of the group
            is the intersection of its members' boxes).  See ``bounded_lsq.ParamMap`` for the rules.  A value may be
            ``(i, ratio)`` or ``(i, ratio, offset)``: p_j = ratio * p_i + offset, two floats shared by
            all problems; `popt`, `pcov`, ``active_mask`` and ``x_covariance`` of the member carry them, its box is
            moved through the tie before the intersection, and for a named model on the device driver the model
            kernel applies them (blsq_model_eval_tie_dev).
            The solver then works on the nf <= n remaining variables: `p0` and `bounds` are still given for all n,
            a callable `f` / `jac` still takes (B, n) and returns (B, m) / (B, m, n), finite differences are taken
            over the nf variables, and a named model with driver='device' is evaluated through the map on the GPU
            (blsq_model_eval_map_dev: the Jacobian is computed and stored nf wide).  `popt` (B, n) has the fixed
            values and tied copies filled in; `pcov` (B, n, n) has zero rows and columns for fixed parameters and
            copied ones for tied parameters, and its variance factor is ``obj_value / (m - nf)``.  ``results[b]``
            carries ``x`` (n,), ``x_free`` (nf,), ``param_map`` (n,), ``active_mask`` (n,) and ``x_covariance``
            (n, n) expanded the same way; its ``jac`` (m, nf) is the Jacobian with respect to the SOLVER's variables
            (a tied group's column is the sum of its members').  With both empty nothing changes.
    estimator : 'lse' (the default: least squares, everything above) or 'poisson': the Poisson maximum-likelihood fit
            of counts.  `ydata` must be finite and >= 0 (it need not be integer) and `sigma` must be
            None; any other string is a ValueError.  The residual of point i becomes the deviance residual
            ``sign(mu - y) sqrt(2 [mu - y + y ln(y / mu)])`` of the model value mu, whose sum of squares is the Poisson
            deviance, so the solver, `bounds`, ``loss=``, ``leverage=``, `fixed` / `tied` and every `jac` choice work as
            they do for least squares and the optimum is the maximum-likelihood estimate — without the bias of least
            squares weighted by ``sqrt(y)`` at low counts, and with ``y == 0`` allowed.  A named model with
            driver='device' is transformed inside the model kernel (blsq_model_eval_est_dev); a callable `f` / `jac`
            still returns the model and ITS Jacobian and is wrapped by ``models.poisson_residual`` /
            ``models.poisson_jacobian``, as is the named model with driver='host'.  Nothing guards the model's sign:
            the `bounds` must keep it positive (an amplitude >= 0 over an offset > 0, say), or NaN reaches the solver.
            ``results[b].fun`` holds the deviance residuals, ``obj_value`` the deviance (the robust objective under
            ``loss=``) and ``deviance`` the sum of their squares; ``jac`` is the Jacobian of the deviance residuals.
            `absolute_sigma` keeps its meaning: True returns ``pinv(J^T J)`` of that Jacobian,
            ``J^T J = sum_i c_i^2 dmu_i dmu_i^T``: the Gauss-Newton form of the Fisher information
            ``sum_i dmu_i dmu_i^T / mu_i`` at the optimum, whose inverse is the Cramér-Rao covariance (``c^2`` is ``1 / mu`` where
            mu == y and in expectation close to it; in an empty channel it is ``1 / (2 mu)``, which makes the variance of
            a background of well under one count per channel come out larger, by a third in the worst of the suite's
            problems); False (the default) multiplies it by ``obj_value / (m - nf)``, the quasi-Poisson dispersion.
            For counts that really are Poisson pass True.
    binned : False (the default: the model sampled at the points `xdata`; nothing changes) or True: `ydata` holds the
            contents of bins (histogram channels, detector pixels) and the model is integrated over each bin,
            ``mu_i = integral over [lo_i, hi_i] of model(t; p) dt``, in closed form (DESIGN.md 7n;
            ``bounded_lsq.models.binned``): the model is read as a density, its parameters keep their meaning and order
            (an amplitude is a density, a constant c contributes ``c (hi - lo)``).  Fitting ``width * model(centre)``
            instead widens a peak by ``width^2 / 12`` in variance whenever a bin is not narrow against it.  Valid with a
            name, a spec or a ``CompositeModel`` on both drivers (driver='device': inside the model kernel,
            blsq_model_eval_bin_dev; driver='host': the numpy definition); with a callable `f` it is a ValueError: a
            callable integrates itself.  `xdata` then holds the bin edges: contiguous bins as (m + 1,) or (B, m + 1)
            edges, bins with gaps as rows ``lo, hi`` of shape (2, m) or (B, 2, m), and for 'gauss2d' the pixels as rows
            ``ulo, uhi, vlo, vhi`` of shape (4, m) or (B, 4, m); edges that are not finite or have lo >= hi are a
            ValueError naming the first such bin.  Everything else composes unchanged: ``estimator='poisson'`` (the
            estimator for histogram counts), `fixed` / `tied`, ``loss=``, `bounds`, `sigma`, ``leverage=`` and
            ``jac='2-point'`` / ``'3-point'``.
    nan_policy : None (the default: nothing changes, a NaN passes through), 'raise' (a NaN in `ydata` is a ValueError)
            or 'omit' (DESIGN.md 7o): point i of problem b is left out of the fit iff ``ydata[b, i]`` is NaN — a dead
            channel, a blanked spike, the padding of a shorter scan (``models.pad_ragged``).  Its residual and its
            Jacobian row are exactly 0, so it contributes nothing to the objective, the steps, the covariance or the
            leverages (0 there); its `sigma` entry (shape (B, m)) and, for a callable or a point-sampled model, its
            abscissa may hold anything.  ±inf is not missing data.  A named model with driver='device' omits the points
            inside the model kernel, without evaluating them (blsq_model_eval_nan_dev); driver='host' and a callable
            go through ``models.omit_residual`` / ``models.omit_jacobian``, the definition.  It composes with
            everything above: ``binned=``, ``estimator='poisson'`` (whose checks of `ydata` then look at the kept
            points), `fixed` / `tied`, ``loss=``, `sigma`, ``leverage=`` and every `jac` choice.  ``results[b]`` gains
            ``nobs``, the number of points kept, and ``omitted``, the boolean mask (m,); the variance factor of
            problem b is ``obj_value / (nobs[b] - nf)``, and a problem with ``nobs[b] <= nf`` gets ``pcov[b] = inf``
            under the ``OptimizeWarning`` while its batch mates keep their results.  A problem without a single point
            is a ValueError naming it; 'propagate' or any other string is a ValueError.  NaN in `xdata` of a binned
            model is still rejected, and the rank tolerance of the pseudo-inverse keeps using the allocated m.
    response, response_origin : None (the default: nothing changes, bit for bit) or a measured kernel the model is
            convolved with before it is compared with `ydata`: the instrument response function of a
            detector under a decay, the resolution function of a spectrometer over a line.  `response` has shape (L,),
            shared by all problems, or (B, L), 1 <= L <= 1024, finite and not all zero (L may exceed m);
            ``mu[i] = sum_k response[k] * model[i + response_origin - k]`` with the terms outside [0, m) dropped
            (``models.apply_response``, the definition): ``response_origin=0`` is the causal convolution, whose delay
            lives in the kernel; ``response_origin=L // 2`` with odd L is ``np.convolve(model, response, 'same')``.  The
            convolution is over the SAMPLE INDEX: `xdata` on a uniform grid, and the kernel sampled at its spacing and
            normalised as wanted, are the caller's business.  Past both ends the model counts as zero, so with a
            baseline the outermost L points see an edge that is not in the data: set them to NaN under
            ``nan_policy='omit'`` (the model is still evaluated there, its neighbours need it).  The residual is
            ``w (mu - y)``, under ``estimator='poisson'`` the deviance residual of mu, and the Jacobian the convolved
            columns times w (times c).  A named model with driver='device' is convolved by a kernel of its own behind
            the model kernel (blsq_response_apply_dev); a callable `f` / `jac` still returns the model and ITS
            Jacobian and is wrapped by ``models.response_residual`` / ``models.response_jacobian``, as is the named
            model with driver='host'.  Composite models, `fixed` / `tied`, ``binned=True`` with contiguous edges
            (bin integrals, then a convolution over the bins), `sigma`, ``loss=``, ``leverage=``, `bounds` and every
            `jac` choice compose unchanged, and so do the results and the variance factor.  'gauss2d' (any model of
            two coordinates) and binned edges given as rows ``lo, hi`` are ValueErrors, as are a kernel of another
            shape, one that is not finite or all zero, and an origin outside 0 .. L - 1.
    separable : False (the default: nothing changes, bit for bit) or True: variable projection.  The
            parameters the model is linear in (``models.linear_params``: the amplitudes of gauss / lorentz / pvoigt / exp
            terms, every coefficient of a ``poly*d``, the ``a_k`` and ``c`` of 'exp_sum' / 'gauss_sum' / 'lorentz_sum',
            ``a`` and ``c`` of 'gauss2d') are removed from the solver: for the other parameters alpha they are the
            solution c(alpha) of a small linear least-squares problem, and the solver minimises over alpha alone, with
            Kaufman's Jacobian.  Fewer variables, a better-conditioned problem, and no start values for amplitudes and
            baselines: `p0` and `bounds` keep all n entries, but the linear entries of `p0` are ignored (they may be
            NaN) and the linear entries of `bounds` must be infinite (ValueError naming the parameter: a bounded
            amplitude needs the plain fit).  `f` is a name, a spec or a ``CompositeModel`` on either driver
            (driver='device': three launches per evaluation, blsq_varpro_expand_dev, the model kernel and
            blsq_varpro_reduce_dev; driver='host': ``models.separable_residual`` / ``separable_jacobian``, the
            definition).  `sigma` in all its shapes, `absolute_sigma`, bounds on the non-linear parameters, both
            methods and ``binned=True`` compose.  `popt` (B, n) is alpha* with c(alpha*) filled in.  `pcov` is the
            covariance of the FULL problem at `popt`, a stationary point of it: the pseudo-inverse covariance of the
            plain model's Jacobian evaluated once at `popt` on the GPU, times ``obj_value / (m - n)`` unless
            `absolute_sigma`, inf under the ``OptimizeWarning`` where m <= n.  ``results[b]`` carries ``x`` (n,),
            ``x_nonlinear`` (n - nl,), ``linear_params`` (nl,) indices, ``active_mask`` (n,) with zeros at the linear
            entries, ``fun`` (the reduced residual, which is the full residual at `popt`), ``jac`` (m, n - nl)
            Kaufman's Jacobian, ``x_covariance`` (n, n), and ``status`` / ``nfev`` / ``njev`` / ``optimality`` of the
            reduced solve.  Where the basis functions are linearly dependent at a point the solver visits (two peaks
            on one position and width) the reduced residual there is NaN, which the solver treats as it treats NaN from
            any model: the objective of such a trial point is NaN, the strict accept test fails and the radius update
            compares false, so the point is rejected and proposed again until ``max_nfev`` ends the problem with
            status 0 (no success: NaN rows in `popt` and `pcov`); a start point with NaN residuals ends the same way.
            The batch mates are not affected.  Not yet supported, each a ValueError: a callable or an ``ExprModel`` as `f`,
            ``jac='2-point'`` / ``'3-point'``, ``loss=`` other than 'linear', ``estimator='poisson'``,
            ``nan_policy='omit'``, `fixed` / `tied`, ``response=`` and ``leverage=True``.

    Returns ``(popt (B, n), pcov (B, n, n), results)``, `results` the B ``OptimizeResult`` of the solve.  pcov[b] is
    ``curve_fit``'s for problem b alone: the pseudo-inverse covariance of its final Jacobian, times
    ``obj_value / (m - n)`` unless `absolute_sigma` — multiplied on the GPU; with driver='device' only B n^2 + 4 B
    numbers leave it — and inf under an ``OptimizeWarning`` where m <= n.  ``results[b].x_covariance`` is that
    scaled matrix as well.

    A problem that did not converge (``results[b].success`` false) is NOT an exception here, unlike ``curve_fit``:
    its rows of popt and pcov are NaN and the other problems are returned intact.
    """
    ydata = np.asarray(ydata, float)
    if ydata.ndim != 2:
        raise ValueError("`ydata` must have shape (B, m).")
    if ydata.size == 0:
        raise ValueError("`ydata` must not be empty!")
    B, m = ydata.shape
    P0 = np.asarray(p0, float)
    if P0.ndim != 2 or P0.shape[0] != B:
        raise ValueError("`p0` must have shape (B, n).")
    n = P0.shape[1]
    if not isinstance(separable, (bool, np.bool_)):
        raise ValueError("`separable` must be False or True.")
    if separable:
        return _fit_separable(f, xdata, ydata, P0, sigma, absolute_sigma, bounds, method, jac, driver, ctx, fixed, tied,
                              estimator, binned, nan_policy, response, kwargs)

    def xdata_of(xdata, model):                  # a named model checks its abscissae (or bin edges); one array for both
        if model is not None:
            xdata = model.check_xdata(xdata, B, m)[0]
        elif isinstance(xdata, (list, tuple, np.ndarray)):
            xdata = np.asarray(xdata, float)
        return xdata, xdata
    lay = _Layout((B,), m, ydata, P0, lambda: _param_map(n, fixed, tied), xdata_of,
                  "nan_policy='omit': problem %d has no point left, every entry of its `ydata` is NaN.",
                  " (a NaN passes through with None)", "a 2-D covariance `sigma` is not supported by `curve_fit_batch`.")
    results, pm, no_dof = _fit(lay, f, xdata, sigma, absolute_sigma, bounds, method, jac, driver, ctx, estimator, binned,
                               nan_policy, kwargs, response, response_origin)
    if pm is not None:                           # the full-size fields of the results, expanded for the batch at once
        X_full = pm.expand_x(np.stack([r.x for r in results]), P0)
        masks = pm.expand_mask(np.stack([np.asarray(r.active_mask) for r in results]))
        has_cov = [b for b, r in enumerate(results) if r.x_covariance is not None]
        covs = pm.expand_cov(np.stack([results[b].x_covariance for b in has_cov])) if has_cov else ()
        for b, r in enumerate(results):
            r.x_free, r.param_map = r.x, pm.pmap.copy()
            r.x, r.active_mask = X_full[b], masks[b]
        for b, C in zip(has_cov, covs):
            results[b].x_covariance = C
    return _popt_pcov(results, (B, n), no_dof, lambda r: r.x, lambda C: C) + (results,)


def _full_covariance(ctx, model, n, x, ydata, sigma, binned, popt, scale):
    """The pseudo-inverse covariance of the plain model's Jacobian at `popt` (B, n), computed on the device (the model
    kernel, then blsq_cov_pinv_dev with `scale` (B,) or None): ``(cov (B, n, n), rank, rcond, status)``.  B n^2 + 3 B
    numbers come back."""
    import ctypes as C
    from ._abi import vp
    B, m = ydata.shape
    bufs, h = [], vp()
    try:
        with _models.DeviceModel(ctx, _models.resolvable(model), B, m, n, x, ydata, sigma,
                                 **({'binned': True} if binned else {})) as dm:
            def dev(nbytes):
                bufs.append(ctx.malloc(nbytes))
                return bufs[-1]
            d_P = ctx.to_device(np.ascontiguousarray(popt, dtype=np.float64))
            bufs.append(d_P)
            d_J, d_cov, d_rcond, d_kept = dev(8 * B * m * n), dev(8 * B * n * n), dev(8 * B), dev(8 * B)
            d_rank, d_status = dev(4 * B), dev(4 * B)
            d_scale = None
            if scale is not None:
                d_scale = ctx.to_device(np.ascontiguousarray(scale, dtype=np.float64))
                bufs.append(d_scale)
            dm.jac_dev(d_P, d_J)
            ctx.check(ctx.lib.blsq_cov_plan_create(ctx.h, B, m, n, C.byref(h)), "blsq_cov_plan_create")
            ctx.check(ctx.lib.blsq_cov_pinv_dev(h, d_J, None, d_scale, d_cov, d_rank, d_rcond, d_kept, d_status),
                      "blsq_cov_pinv_dev")
            ctx.sync()
            return (ctx.to_host(d_cov, (B, n, n), np.float64), ctx.to_host(d_rank, (B,), np.int32),
                    ctx.to_host(d_rcond, (B,), np.float64), ctx.to_host(d_status, (B,), np.int32))
    finally:
        if h:
            ctx.lib.blsq_cov_plan_destroy(h)
        for p in bufs:
            ctx.free(p)


def _fit_separable(f, xdata, ydata, P0, sigma, absolute_sigma, bounds, method, jac, driver, ctx, fixed, tied, estimator,
                   binned, nan_policy, response, kwargs):
    """``curve_fit_batch(separable=True)``: the checks, the solve over the non-linear parameters, the
    linear ones filled in and the covariance of the full problem at the result."""
    B, m = ydata.shape
    n = P0.shape[1]
    if isinstance(f, _models.ExprModel):
        raise ValueError("`separable=True` is not yet supported with the expression model '%s': the structure of a "
                         "formula is not known." % f.name)
    if not isinstance(f, (str, _models.CompositeModel)):
        raise ValueError("`separable=True` needs a built-in model (a name, a spec or a CompositeModel) as `f`: the "
                         "linear parameters of a callable are not known.")
    if jac is not None:
        raise ValueError("`jac` must be None with `separable=True`: Kaufman's Jacobian comes from the model's analytic "
                         "one ('2-point' / '3-point' and a callable are not yet supported).")
    if kwargs.get('loss', 'linear') != 'linear':
        raise ValueError("`loss` must be 'linear' with `separable=True`: a robust loss is not yet supported.")
    if _models.check_estimator(estimator) != 'lse':
        raise ValueError("estimator='poisson' is not yet supported with `separable=True`.")
    if nan_policy == 'omit':
        raise ValueError("nan_policy='omit' is not yet supported with `separable=True`.")
    if nan_policy == 'raise':
        if np.isnan(ydata).any():
            raise ValueError("The input contains nan values")
    elif nan_policy is not None:
        raise ValueError("`nan_policy` must be None or 'raise' with `separable=True`, not %r." % (nan_policy,))
    if fixed is not None or tied:
        raise ValueError("`fixed` / `tied` are not yet supported with `separable=True`.")
    if response is not None:
        raise ValueError("`response` is not yet supported with `separable=True`.")
    if kwargs.get('leverage', False):
        raise ValueError("leverage=True is not yet supported with `separable=True`.")
    if driver not in ('host', 'device'):
        raise ValueError("`driver` must be 'host' or 'device'.")
    if 'args' in kwargs:
        raise ValueError("'args' is not a supported keyword argument.")
    kwargs = dict(kwargs)
    if 'max_nfev' not in kwargs:
        kwargs['max_nfev'] = kwargs.pop('maxfev', None)
    model = _models.resolve(f)
    model.terms(n)
    lin, owner = _models.linear_params(model, n)
    if m <= lin.size:
        raise ValueError("`separable=True` needs more points than linear parameters: m = %d, nl = %d." % (m, lin.size))
    host_model = _models.binned(model) if binned else model
    x = host_model.check_xdata(xdata, B, m)[0]
    if len(bounds) != 2:
        raise ValueError("`bounds` must contain 2 elements.")
    try:
        lb = np.broadcast_to(np.asarray(bounds[0], dtype=float), (B, n))
        ub = np.broadcast_to(np.asarray(bounds[1], dtype=float), (B, n))
    except ValueError:
        raise ValueError("`bounds` must be broadcastable to (B, n): they keep all n parameters.") from None
    names = getattr(model, 'param_names', None)
    for k in lin:
        if not (np.all(lb[:, k] == -np.inf) and np.all(ub[:, k] == np.inf)):
            raise ValueError("`separable=True`: parameter %d%s is linear and is projected out, so its bounds must be "
                             "infinite; fit without `separable=True` to bound it."
                             % (k, " ('%s')" % names[k] if names else ""))
    if sigma is not None:
        sigma = np.asarray(sigma, float)
        try:
            _models.sigma_weights(sigma, (B,), m)
        except ValueError:
            if sigma.ndim != 2:
                raise
            raise ValueError("a 2-D covariance `sigma` is not supported by `curve_fit_batch`.") from None
    non = np.nonzero(owner >= 0)[0]
    X0, red = np.ascontiguousarray(P0[:, non]), (lb[:, non], ub[:, non])
    if ctx is None:
        from ._hip_step import default_context
        ctx = default_context()
    spec = _models.resolvable(model)
    on = {'binned': True} if binned else {}
    if driver == 'device':
        func = _models.DeviceFit(spec, n, x, ydata, sigma, separable=True, **on)
        results = least_squares_batch(func, X0, None, bounds=red, method=method, driver=driver, ctx=ctx, **kwargs)
        X = np.stack([r.x for r in results])
        with _models.DeviceModel(ctx, spec, B, m, n, x, ydata, sigma, separable=True, **on) as dm:
            d_X = ctx.to_device(X)
            try:
                c = dm.linear_coefficients(d_X)
            finally:
                ctx.free(d_X)
    else:
        from ._varpro import _HostStage
        stage = _HostStage(model, ydata, sigma, n, binned)
        results = least_squares_batch(lambda X: stage(x, X)[0], X0, lambda X: stage(x, X)[1], bounds=red, method=method,
                                      driver=driver, ctx=ctx, **kwargs)
        X = np.stack([r.x for r in results])
        c = stage(x, X)[2]
    popt = _models.varpro_expand(X, lin, n)
    popt[:, lin] = c
    obj = np.array([r.obj_value for r in results], dtype=float)
    scale = obj / (m - n) if (m > n and not absolute_sigma) else None
    cov, rank, rcond, status = _full_covariance(ctx, model, n, x, ydata, sigma, binned, popt, scale)
    for b, r in enumerate(results):
        mask = np.zeros(n, dtype=np.asarray(r.active_mask).dtype)
        mask[non] = r.active_mask
        r.x_nonlinear, r.linear_params = r.x, lin.copy()
        r.x, r.active_mask = popt[b].copy(), mask
        r.x_covariance = None if int(status[b]) != 0 else cov[b]
        r.x_covariance_rank, r.x_covariance_rcond = int(rank[b]), float(rcond[b])
    no_dof = np.full(B, (m <= n) and not absolute_sigma)
    return _popt_pcov(results, (B, n), no_dof, lambda r: r.x, lambda C: C) + (results,)


GLOBAL_MAX_NV = 256                                      # BLSQ_GLOBAL_MAX_NV


def _fit_separable_global(f, xdata, ydata, p0, shared, sigma, absolute_sigma, bounds, method, jac, driver, ctx, fixed,
                          tied, estimator, nan_policy, kwargs):
    """``curve_fit_global(separable=True)``: the checks, the solve over the non-linear parameters in the
    layout of ``models.separable_global_map``, the linear ones filled in and the blocks of the full covariance."""
    kwargs = dict(kwargs)
    if kwargs.pop('binned', False):
        raise ValueError("`binned=True` is not supported by `curve_fit_global`.")
    if kwargs.pop('response', None) is not None or kwargs.pop('response_origin', 0) != 0:
        raise ValueError("`response` is not supported by `curve_fit_global`: an instrument response is not built for "
                         "global fits.")
    if isinstance(f, _models.ExprModel):
        raise ValueError("`separable=True` is not yet supported with the expression model '%s': the structure of a "
                         "formula is not known." % f.name)
    if not isinstance(f, (str, _models.CompositeModel)):
        raise ValueError("`separable=True` needs a built-in model (a name, a spec or a CompositeModel) as `f`: the "
                         "linear parameters of a callable are not known.")
    if jac is not None:
        raise ValueError("`jac` must be None with `separable=True`: Kaufman's Jacobian comes from the model's analytic "
                         "one ('2-point' / '3-point' and a callable are not yet supported).")
    if kwargs.get('loss', 'linear') != 'linear':
        raise ValueError("`loss` must be 'linear' with `separable=True`: a robust loss is not yet supported.")
    if _models.check_estimator(estimator) != 'lse':
        raise ValueError("estimator='poisson' is not yet supported with `separable=True`.")
    if nan_policy == 'omit':
        raise ValueError("nan_policy='omit' is not yet supported with `separable=True`.")
    if nan_policy not in (None, 'raise'):
        raise ValueError("`nan_policy` must be None or 'raise' with `separable=True`, not %r." % (nan_policy,))
    if fixed is not None or tied:
        raise ValueError("`fixed` / `tied` are not yet supported with `separable=True`.")
    if kwargs.get('leverage', False):
        raise ValueError("leverage=True is not yet supported with `separable=True`.")
    if driver not in ('host', 'device'):
        raise ValueError("`driver` must be 'host' or 'device'.")
    if 'args' in kwargs:
        raise ValueError("'args' is not a supported keyword argument.")
    if 'max_nfev' not in kwargs:
        kwargs['max_nfev'] = kwargs.pop('maxfev', None)
    ydata = np.asarray(ydata, float)
    P0 = np.asarray(p0, float)
    single = ydata.ndim == 2
    if single:
        ydata = ydata[np.newaxis]
        if P0.ndim == 2:
            P0 = P0[np.newaxis]
    if ydata.ndim != 3:
        raise ValueError("`ydata` must have shape (S, m) or (G, S, m).")
    if ydata.size == 0:
        raise ValueError("`ydata` must not be empty!")
    if nan_policy == 'raise' and np.isnan(ydata).any():
        raise ValueError("The input contains nan values")
    G, S, m = ydata.shape
    if P0.ndim != 3 or P0.shape[:2] != (G, S):
        raise ValueError("`p0` must have shape (S, n) or (G, S, n) like `ydata`.")
    n = P0.shape[2]
    model = _models.resolve(f)
    model.terms(n)
    _models.check_global(model)
    gm, lin, owner, non = _models.separable_global_map(model, n, S, shared)
    nl, nv = lin.size, gm.nv
    if nv > GLOBAL_MAX_NV:
        raise ValueError("the group has nv = nsh + S nloc = %d + %d * %d = %d non-linear variables, more than %d."
                         % (gm.ns, S, gm.nl, nv, GLOBAL_MAX_NV))
    if m <= nl:
        raise ValueError("`separable=True` needs more points than linear parameters: m = %d, nl = %d." % (m, nl))
    x_dev, _, sstride = _models.global_xdata(xdata, G, S, m)
    if len(bounds) != 2:
        raise ValueError("`bounds` must contain 2 elements.")
    try:
        lb = np.broadcast_to(np.asarray(bounds[0], dtype=float), (G, S, n))
        ub = np.broadcast_to(np.asarray(bounds[1], dtype=float), (G, S, n))
    except ValueError:
        raise ValueError("`bounds` must be broadcastable to (G, S, n): they keep all n parameters.") from None
    names = getattr(model, 'param_names', None)
    for k in lin:
        if not (np.all(lb[..., k] == -np.inf) and np.all(ub[..., k] == np.inf)):
            raise ValueError("`separable=True`: parameter %d%s is linear and is projected out, so its bounds must be "
                             "infinite; fit without `separable=True` to bound it."
                             % (k, " ('%s')" % names[k] if names else ""))
    if sigma is not None:
        sigma = np.asarray(sigma, float)
        _models.sigma_weights(sigma, (G, S), m)
    red = gm.reduce_bounds(lb[..., non], ub[..., non])
    X0 = np.ascontiguousarray(gm.reduce_x(P0[..., non]))
    if ctx is None:
        from ._hip_step import default_context
        ctx = default_context()
    spec = _models.resolvable(model)
    M, dof = S * m, S * m - nv - S * nl
    want = dict(bounds=red, method=method, driver=driver, ctx=ctx, covariance='pinv', _variance_scale=False, **kwargs)

    def factor(results):
        """(scale (G,) or None, status (G,)): the variance factor of every group, and 1 where its covariance is
        missing."""
        status = np.array([0 if (r.success and r.x_covariance is not None and not np.isnan(r.x_covariance).any())
                           else 1 for r in results], dtype=np.int32)
        if absolute_sigma or dof <= 0:
            return None, status
        return np.array([r.obj_value for r in results], dtype=float) / dof, status

    if driver == 'device':
        func = _models.DeviceFit(spec, n, x_dev, ydata, sigma, separable=True, global_map=gm)
        results = least_squares_batch(func, X0, None, **want)
        X = np.stack([r.x for r in results])
        scale, status = factor(results)
        Cred = np.stack([r.x_covariance if st == 0 else np.full((nv, nv), np.nan) for r, st in zip(results, status)])
        with _models.DeviceModel(ctx, spec, G, m, n, x_dev, ydata, sigma, separable=True, global_map=gm) as dm:
            d_X, d_C = ctx.to_device(X), ctx.to_device(np.ascontiguousarray(Cred))
            try:
                cov, c, info = dm.covariance_blocks(d_X, d_C, scale, status)
            finally:
                ctx.free(d_X)
                ctx.free(d_C)
    else:
        from ._varpro import _HostGlobalStage
        stage = _HostGlobalStage(model, ydata, shared, sigma, n)
        results = least_squares_batch(lambda X: stage(x_dev, X)[0], X0, lambda X: stage(x_dev, X)[1], **want)
        X = np.stack([r.x for r in results])
        scale, status = factor(results)
        Cred = np.stack([r.x_covariance if st == 0 else np.full((nv, nv), np.nan) for r, st in zip(results, status)])
        _, _, c, info, Sinv, TD = stage(x_dev, X)
        cov = _models.separable_global_cov(Cred, Sinv, TD, gm, scale, lin)
    popt = np.full((G, S, n), np.nan)
    pcov = np.full((G, S, n, n), np.nan)
    alpha = gm.split_x(X)                                    # (G, S, na)
    warn_cov = False
    for g, r in enumerate(results):
        r.global_map, r.linear_params = gm, lin.copy()
        r.popt = _models.varpro_expand(alpha[g], lin, n)
        r.popt[:, lin] = c[g]
        r.linear_coefficients = c[g].copy()
        if r.x_covariance is not None and scale is not None:
            r.x_covariance = r.x_covariance * scale[g]
        if not r.success:
            continue
        popt[g] = r.popt
        if status[g] != 0 or (dof <= 0 and not absolute_sigma) or np.isnan(cov[g]).any():
            pcov[g] = np.inf
            warn_cov = True
        else:
            pcov[g] = cov[g]
    if warn_cov:
        warnings.warn(_COV_WARNING, category=OptimizeWarning, stacklevel=3)
    if single:
        return popt[0], pcov[0], results
    return popt, pcov, results


def curve_fit_global(f, xdata, ydata, p0, shared, sigma=None, absolute_sigma=False, bounds=(-np.inf, np.inf),
                     method='trf', jac=None, driver='host', ctx=None, fixed=None, tied=None, estimator='lse',
                     nan_policy=None, separable=False, **kwargs):
    """A global fit: S data sets of one model fitted together, with the parameters in `shared` common to all of them
    (DESIGN.md 7p).  A decay measured at S wavelengths, a line scanned at S temperatures: the rates, the position and
    the width have one value for the group, the amplitudes and baselines one per data set.

    ydata : (S, m) for one global fit, or (G, S, m) for G independent global fits solved as one batch.
    p0 : (..., S, n), required.  A shared parameter starts from data set 0 of its group.
    shared : a boolean mask (n,) or a sequence of indices, the same for every group (``bounded_lsq.GlobalMap`` has the
            rules: a shared index may not be fixed, a tied parameter is shared iff the one it follows is; an empty
            `shared` is a ValueError that points to ``curve_fit_batch``).
    f : a name, a composite spec or a ``CompositeModel`` of one coordinate on either driver (driver='device': residuals
            and Jacobians of the whole group are evaluated on the GPU through blsq_model_eval_global_dev, the
            Jacobian written into the group's column layout) — or a callable ``f(xdata, P) -> (G S, m)`` for the
            parameters ``P`` (G S, n) of all data sets, row g S + s being data set s of group g; it goes through
            ``GlobalMap.wrap_f`` / ``wrap_jac``, as the named model does with driver='host'.  'gauss2d' and
            ``binned=True`` are ValueErrors, and so is ``response=`` (not built for global fits).
    xdata : (m,), (S, m) or (G, S, m); a callable receives (m,) or (G S, m).
    sigma : None, a scalar, (m,), (S, m) or (G, S, m).  bounds : pair broadcastable to (G, S, n); the box of a shared
            parameter is the intersection over the data sets of its group (empty: ValueError).
    jac : None, '2-point', '3-point' (differences over the nv variables) or, with a callable `f`,
            ``jac(xdata, P) -> (G S, m, n)``.
    fixed, tied, estimator, nan_policy, method, driver, ctx, **kwargs (``loss=``, ``f_scale=``, tolerances,
            ``leverage=``) : as ``curve_fit_batch``; `fixed` and `tied` act inside every data set.

    The group is ONE dense problem of M = S m rows and nv = ns + S nl variables (ns shared slots, nl per data set; the
    shared ones first, then the local ones of data set 0, 1, ...; nv <= 256, ValueError beyond).

    Returns ``(popt (..., S, n), pcov (..., S, n, n), results)``.  A shared parameter comes back equal in all S rows.
    ``pcov[g, s]`` is the (n, n) block of data set s of the group's covariance (``GlobalMap.expand_cov``); the variance
    factor of a group is ``obj_value / (M - nv)`` — under 'omit' ``obj_value / (nobs_g - nv)`` with the points the
    group kept — and a group without degrees of freedom gets inf under the ``OptimizeWarning``.  ``results[g]`` is the
    group's ``OptimizeResult``: ``x`` (nv,), ``x_covariance`` (nv, nv) — the full matrix, with the terms between data
    sets —, ``popt`` (S, n), ``global_map``, ``fun`` (M,), ``jac`` (M, nv), ``leverage`` (M,) with ``leverage=True``,
    ``deviance`` under Poisson, ``nobs`` and ``omitted`` (S, m) under 'omit'.  A group that did not converge gives NaN
    rows; with 'omit' a data set without a single point is a ValueError naming group and data set.

    separable : False (the default: nothing changes, bit for bit) or True: the classical algorithm of
            global analysis.  The linear parameters of the model (``models.linear_params``) are projected out per data
            set, so the solver sees the non-linear ones alone: nv = nsh + S nloc variables (nsh shared, nloc local
            non-linear parameters; the layout is ``models.separable_global_map``'s ``GlobalMap`` over the non-linear
            parameters).  nv <= 256 holds for THIS count: with every non-linear parameter shared a group of any S is
            a problem of nsh columns, and the full count nv + S nl has no limit.  Every index in `shared` must be
            non-linear (a shared amplitude would couple the projections: ValueError naming it).  `f` is a name, a spec
            or a ``CompositeModel`` of one coordinate, on either driver (driver='device': blsq_varpro_expand_global_dev,
            the model kernel on the G S data sets and blsq_varpro_reduce_global_dev per evaluation; driver='host':
            ``models.separable_global_residual`` / ``_jacobian``, the definition).  `p0`, `bounds`, `popt` and `pcov`
            keep all n parameters per data set; the linear entries of `p0` are ignored (they may be NaN) and those of
            `bounds` must be infinite; the box of a shared parameter is the intersection over the group.  `sigma` in
            the shapes above, `absolute_sigma`, bounds on the non-linear parameters and both methods compose.  `popt`
            has c(alpha*) filled in.  ``pcov[g, s]`` is the (n, n) block of data set s of the covariance of the FULL
            problem: Kaufman's ``J^T J`` is the Schur complement of the full Gauss-Newton matrix, so the covariance of
            the reduced group is the exact alpha-alpha block and the others follow from (nl, nl) and (nl, n - nl)
            matrices of the projection (``models.separable_global_cov``; on the device blsq_varpro_cov_blocks_dev) —
            nothing of the full size is formed.  Its variance factor is ``obj_value / (S m - nv - S nl)`` unless
            `absolute_sigma`; a group without a degree of freedom, or whose reduced covariance is missing, gets inf
            under the ``OptimizeWarning``.  ``results[g]`` carries ``x`` (nv,), ``x_covariance`` (nv, nv) — the reduced
            matrix, the exact alpha-alpha block of the full covariance, with the same factor —, ``popt`` (S, n),
            ``linear_coefficients`` (S, nl), ``linear_params``, ``global_map``, ``fun`` (S m,) and ``jac`` (S m, nv).
            Each a ValueError of its own: a callable or an ``ExprModel`` as `f`, ``jac=`` other than None, ``loss=``
            other than 'linear', ``estimator='poisson'``, ``nan_policy='omit'``, `fixed` / `tied`, ``leverage=True``,
            m <= nl and a model with nothing non-linear.
    """
    if not isinstance(separable, (bool, np.bool_)):
        raise ValueError("`separable` must be False or True.")
    if separable:
        return _fit_separable_global(f, xdata, ydata, p0, shared, sigma, absolute_sigma, bounds, method, jac, driver,
                                     ctx, fixed, tied, estimator, nan_policy, kwargs)
    if kwargs.pop('binned', False):
        raise ValueError("`binned=True` is not supported by `curve_fit_global`.")
    if kwargs.pop('response', None) is not None or kwargs.pop('response_origin', 0) != 0:
        raise ValueError("`response` is not supported by `curve_fit_global`: an instrument response is not built for "
                         "global fits.")
    ydata = np.asarray(ydata, float)
    P0 = np.asarray(p0, float)
    single = ydata.ndim == 2
    if single:
        ydata = ydata[np.newaxis]
        if P0.ndim == 2:
            P0 = P0[np.newaxis]
    if ydata.ndim != 3:
        raise ValueError("`ydata` must have shape (S, m) or (G, S, m).")
    if ydata.size == 0:
        raise ValueError("`ydata` must not be empty!")
    G, S, m = ydata.shape
    if P0.ndim != 3 or P0.shape[:2] != (G, S):
        raise ValueError("`p0` must have shape (S, n) or (G, S, n) like `ydata`.")
    n = P0.shape[2]
    gm = GlobalMap(n, S, shared, fixed, tied)
    if gm.nv > GLOBAL_MAX_NV:
        raise ValueError("the group has nv = ns + S nl = %d + %d * %d = %d variables, more than %d."
                         % (gm.ns, S, gm.nl, gm.nv, GLOBAL_MAX_NV))

    def xdata_of(xdata, model):                  # a callable gets (m,), or one row per data set of the batch
        if model is not None:
            _models.check_global(model)
        x_dev, _, sstride = _models.global_xdata(xdata, G, S, m)
        return (x_dev if not sstride else np.broadcast_to(x_dev, (G, S, m)).reshape(G * S, m)), x_dev
    lay = _Layout((G, S), m, ydata.reshape(G, S * m), P0, lambda: gm, xdata_of,
                  "nan_policy='omit': data set %d of group %d has no point left, every entry of its `ydata` is NaN.",
                  "", None)
    results, _, no_dof = _fit(lay, f, xdata, sigma, absolute_sigma, bounds, method, jac, driver, ctx, estimator, False,
                              nan_policy, kwargs)
    for g, r in enumerate(results):
        r.global_map = gm
        r.popt = gm.expand_x(r.x, P0[g])
    popt, pcov = _popt_pcov(results, (G, S, n), no_dof, lambda r: r.popt, gm.expand_cov)
    if single:
        return popt[0], pcov[0], results
    return popt, pcov, results
