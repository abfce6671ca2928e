// glm_dev.hpp -- link / variance functions of the GLM (link_functions.rs:5-77), shared by the one-model IRLS pass of moments.hip
// (WM = 3) and the per-group IRLS kernel of grouped_irls.hip: 0 identity / gaussian, 1 log / poisson, 2 logit / binomial,
// 3 inverse / gamma -- evaluated in T, like the reference's `T: RealField + Float`
#pragma once
#include "common.hpp"

namespace pds {

template <typename T>
__device__ __forceinline__ T glm_link(int link, T mu) {
    switch (link) {
        case 1: return (T)log(mu);
        case 2: return (T)log(mu / (T(1) - mu));
        case 3: return T(1) / mu;
        default: return mu;
    }
}
template <typename T>
__device__ __forceinline__ T glm_inv(int link, T eta) {
    switch (link) {
        case 1: return (T)exp(eta);
        case 2: { const T e = (T)exp(eta); return e / (T(1) + e); }
        case 3: return T(1) / eta;
        default: return eta;
    }
}
template <typename T>
__device__ __forceinline__ T glm_deriv(int link, T mu) {
    switch (link) {
        case 1: return T(1) / mu;
        case 2: return T(1) / (mu * (T(1) - mu));
        case 3: { const T r = T(1) / mu; return -(r * r); }
        default: return T(1);
    }
}
template <typename T>
__device__ __forceinline__ T glm_var(int variance, T mu) {
    switch (variance) {
        case 1: return mu;
        case 2: return mu * (T(1) - mu);
        case 3: return mu * mu;
        default: return T(1);
    }
}

// ---- deviances (f64: the report kernels of grouped_glm_report.hip and the final pass of glm_within.hip)
__device__ __forceinline__ double glm_xlogy(double a, double b) { return a > 0.0 ? a * log(b) : 0.0; }  // (0 ln 0 = 0)

// a row's deviance term.  (gr_accumulate of grouped_glm_report.hip spells the same four terms in its own switch, next to the family
// sum's: returned from a helper and added behind the switch they compile to other instructions there.)
__device__ __forceinline__ double glm_unit_deviance(int variance, double y, double mu) {
    const double e = y - mu;
    switch (variance) {
        case 1: return 2.0 * (glm_xlogy(y, y / mu) - e);
        case 2: return 2.0 * (glm_xlogy(y, y / mu) + glm_xlogy(1.0 - y, (1.0 - y) / (1.0 - mu)));
        case 3: return 2.0 * (e / mu - log(y / mu));
        default: return e * e;
    }
}

}  // namespace pds
