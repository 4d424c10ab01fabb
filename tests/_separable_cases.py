"""What the tests of the separable fits share: the case grid of the projection, its metrics and their cap,
and the data of the whole fits.  Not collected as a test.

Metrics of a projection against the np.longdouble definition (``models.varpro_reduce``), per problem:
    f:  max |f - f_ref| / |w y|_2
    c:  max |c - c_ref| / max |c_ref|
    J:  per column j, max |J_j - J_ref,j| / (|w G_j|_2 |c_owner(j)|)
Cap: each <= 32 kappa_2(Phi_w) eps.  The float64 definition itself stays below 2.2 kappa eps on the grid (the CPU test
holds it to the cap, which vets the inputs), so the cap leaves a factor of about 15 for another summation order; the
scheme without its correction step misses it by four orders of magnitude on the ill-conditioned case."""
import functools

import numpy as np

from bounded_lsq import models

LD = np.longdouble
EPS = np.finfo(np.float64).eps
CAP = 32.0
B = 3
# (m, nl, na): one row more than nl; 63 / 64 / 65 around the 64-row block of the kernel; 130: three blocks; 16 linear
# columns (the widest Phi), 48 and 61 non-linear ones (four and five tiles of the work layout), 1 (two tiles)
GRID = ((2, 1, 1), (5, 2, 2), (17, 16, 48), (63, 5, 11), (64, 5, 11), (65, 16, 48), (130, 3, 61), (257, 16, 1))
ILL = (130, 5, 11)                                 # one Phi column = another + 1e-5 noise: kappa(Phi_w) about 2e5
WFORMS = ("none", "shared", "per_problem")


class Case:
    def __init__(self, m, nl, na, seed, ill=False):
        rng = np.random.default_rng(seed)
        n = nl + na
        self.m, self.nl, self.na, self.n = m, nl, na, n
        self.lin = np.sort(rng.choice(n, nl, replace=False)).astype(np.int32)
        self.owner = rng.integers(0, nl, n).astype(np.int32)
        self.owner[self.lin] = -1
        self.non = np.flatnonzero(self.owner >= 0)
        self.G = rng.standard_normal((B, m, n))
        if ill:
            self.G[:, :, self.lin[1]] = self.G[:, :, self.lin[0]] + 1e-5 * rng.standard_normal((B, m))
        # y = Phi c0 + noise with 0.5 <= |c0| <= 2: the J metric divides by |c_owner(j)|, so a linear parameter that
        # happens to vanish (y unrelated to Phi) would measure the draw, not the arithmetic
        # The ill-conditioned case keeps its residual r small: every least-squares solver, a QR one included, has an
        # error term kappa^2 eps |r| / (|Phi| |c|) next to kappa eps, which the cap does not model; noise of 1e-6 puts
        # it at a tenth of kappa eps (at 0.1 it would be the larger of the two, and the pair of near-equal columns
        # would take coefficients of 1e3 with opposite signs)
        c0 = rng.uniform(0.5, 2.0, (B, nl)) * rng.choice([-1.0, 1.0], (B, nl))
        noise = 1e-6 if ill else 0.1
        self.y = np.einsum("bip,bp->bi", self.G[:, :, self.lin], c0) + noise * rng.standard_normal((B, m))
        self.ws = {"none": None, "shared": rng.uniform(0.5, 2.0, m), "per_problem": rng.uniform(0.5, 2.0, (B, m))}

    def weights(self, wform):
        w = self.ws[wform]
        return np.ones((B, self.m)) if w is None else np.broadcast_to(w, (B, self.m))

    def kappa(self, wform):
        Pw = self.weights(wform)[:, :, None] * self.G[:, :, self.lin]
        return np.array([np.linalg.cond(Pw[b]) for b in range(B)])


@functools.lru_cache(maxsize=None)
def case(m, nl, na, ill=False):
    return Case(m, nl, na, 1000 * m + 10 * nl + na + (7 if ill else 0), ill)


@functools.lru_cache(maxsize=None)
def reference(m, nl, na, wform, ill=False):
    """(f, J, c, info) of the case in np.longdouble; computed once and shared."""
    cs = case(m, nl, na, ill)
    w = cs.ws[wform]
    out = models.varpro_reduce(cs.G.astype(LD), cs.y.astype(LD), None if w is None else w.astype(LD), cs.lin, cs.owner)
    for a in out:
        a.setflags(write=False)
    return out


def fractions(cs, wform, ref, f=None, J=None, c=None, problems=None):
    """The metrics present, each as a fraction of the cap: dict name -> the worst over the problems looked at."""
    f_ref, J_ref, c_ref, _ = ref
    idx = np.arange(B) if problems is None else np.asarray(problems)
    w = cs.weights(wform)
    cap = CAP * cs.kappa(wform) * EPS
    out = {}
    if f is not None:
        err = np.max(np.abs(f.astype(LD) - f_ref[idx]), axis=1) / np.linalg.norm(w * cs.y, axis=1)[idx]
        out["f"] = float(np.max(err / cap[idx]))
    if c is not None:
        err = np.max(np.abs(c.astype(LD) - c_ref[idx]), axis=1) / np.max(np.abs(c_ref[idx]), axis=1)
        out["c"] = float(np.max(err / cap[idx]))
    if J is not None:
        col = np.linalg.norm(w[:, :, None] * cs.G[:, :, cs.non], axis=1)[idx]                    # (B, na)
        own = np.abs(c_ref[idx][:, cs.owner[cs.non]])
        err = np.max(np.abs(J.astype(LD) - J_ref[idx]), axis=1) / (col * own)
        out["J"] = float(np.max(err / cap[idx][:, None]))
    return out


# ---- whole fits -------------------------------------------------------------------------------------------------------
FIT_B, FIT_M, NOISE = 8, 130, 0.01
TOLS = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12)
FITS = {
    # spec: (truth, xdata)
    "exp*2+poly*1": (np.array([3.0, 0.7, 1.5, 3.1, 0.2]), np.linspace(0.0, 4.0, FIT_M)),
    "gauss*2+lorentz+poly*2": (np.array([2.0, -0.8, 0.3, 1.5, 0.1, 0.35, 1.0, 0.7, 0.3, 0.5, 0.1]),
                               np.linspace(-2.0, 2.0, FIT_M)),
    "gauss2d": (np.array([2.0, 0.3, -0.2, 0.5, 0.1]), None),
    "gauss+poly*1": (np.array([2.0, 0.2, 0.4, 0.3]), np.linspace(-2.0, 2.0, FIT_M + 1)),      # binned: the edges
}


@functools.lru_cache(maxsize=None)
def fit_data(spec, binned=False):
    """(model, n, xdata, truth (B, n), ydata (B, m)) of a whole fit: the truth jittered by 1 % per problem, noise 0.01."""
    truth, x = FITS[spec]
    rng = np.random.default_rng(len(spec) + 17)
    M = models.resolve(spec)
    if x is None:
        x = rng.uniform(-1.5, 1.5, (2, FIT_M))
    P = truth * (1.0 + 0.01 * rng.standard_normal((FIT_B, truth.size)))
    noise = NOISE * (x[1] - x[0] if binned else 1.0)               # (bin contents are densities times the bin width)
    Y = (models.binned(M) if binned else M).f(x, P) + noise * rng.standard_normal((FIT_B, FIT_M))
    for a in (x, P, Y):
        a.setflags(write=False)
    return M, truth.size, x, P, Y


def start(spec, P):
    """p0 of the separable fit: NaN in the linear entries, 1.3 truth + 0.05 in the others."""
    lin, owner = models.linear_params(spec, P.shape[1])
    p0 = 1.3 * P + 0.05
    p0[:, lin] = np.nan
    return p0
