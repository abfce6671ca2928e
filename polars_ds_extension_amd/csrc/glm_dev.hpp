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

}  // namespace pds
