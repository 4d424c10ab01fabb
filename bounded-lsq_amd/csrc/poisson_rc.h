// The Poisson transform of the device, shared by the kernels that apply it: model_kernels.hip (the
// POISSON instances) and response_kernels.hip (the epilogue of the convolution, 7s).
#pragma once
#include <hip/hip_runtime.h>

namespace blsq {

// (r, c) of models.poisson_transform for the model value mu and the count y: r = sign(mu - y) sqrt(D),
// D = 2 [mu - y + y ln(y / mu)] the deviance, c = dr / dmu, in the form that neither cancels nor divides 0 by 0 at
// mu == y.  phi(u) = (u - log1p(u)) / u^2 directly where |u| >= POISSON_U0, by POISSON_TERMS terms of its series
// sum_k (-u)^k / (k + 2) below (Horner; the coefficients are constants folded at compile time, correctly rounded as
// numpy's are).  Nothing is checked: mu <= 0 passes through as IEEE arithmetic gives it.
static constexpr double POISSON_U0 = 0.25;
static constexpr int POISSON_TERMS = 26;
__device__ __forceinline__ void poisson_rc(double mu, double y, double& r, double& c) {
  if (y > 0.0) {
    const double d = mu - y;
    const double u = d / y;
    double phi;
    if (fabs(u) < POISSON_U0) {
      phi = ((POISSON_TERMS - 1) & 1 ? -1.0 : 1.0) / (double)(POISSON_TERMS + 1);
#pragma unroll
      for (int k = POISSON_TERMS - 2; k >= 0; --k) phi = phi * u + (k & 1 ? -1.0 : 1.0) / (double)(k + 2);
    } else {
      phi = (u - log1p(u)) / (u * u);
    }
    const double s = sqrt((2.0 * phi) / y);
    r = d * s;
    c = 1.0 / (mu * s);
  } else {
    r = sqrt(2.0 * mu);
    c = 1.0 / r;
  }
}

}  // namespace blsq
