// glm_wo_model.hip -- the one-model IRLS iteration with a prior weight pw_i and an offset o_i per row (capi_models.hpp,
// glm_irls_wo_impl: pds_glm_irls_wo_*, and the groups of a weighted / offset grouped call above glm_split_rows).
//   * glm_wo_sums_kernel: the side sums of the first pass -- rows of positive weight, weights that are negative or not finite,
//     sum pw and sum pw y over the rows of positive weight -- by ONE workgroup in a fixed order (no atomics: the same bits every call).
//   * irls_working_wo_kernel: the weighted / offset form of moments.hip's irls_working_wide_kernel, at every width: lane = row,
//     w = pw / (g'(mu)^2 V(mu)), z = (eta - o) + g'(mu) (y - mu) with eta = x . beta + o (first iteration: eta = g(mu0)); a row of
//     weight 0 gets w = 0 and z = 0 whatever its y holds.  The weighted Gram build (moments.hip WM = 1 up to 16 features,
//     moments_wide.hip beyond) then reads w as its weight column and z as its target: the fused WM = 3 pass is left as it is.
#include "common.hpp"
#include "glm_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kSumsThreads = 1024;

template <typename T>
__global__ __launch_bounds__(kSumsThreads) void glm_wo_sums_kernel(const T* __restrict__ y, const T* __restrict__ pw, int64_t n,
                                                                   double* __restrict__ out) {
    __shared__ double sh[4][kSumsThreads];
    double n_pos = 0.0, n_bad = 0.0, spw = 0.0, spwy = 0.0;
    for (int64_t r = threadIdx.x; r < n; r += kSumsThreads) {
        const double w = pw ? (double)as_global(pw)[r] : 1.0;
        if (!(w >= 0.0 && fabs(w) <= 1.79769313486231570e308)) n_bad += 1.0;
        if (w > 0.0) {
            n_pos += 1.0;
            spw += w;
            spwy += w * (double)as_global(y)[r];
        }
    }
    sh[0][threadIdx.x] = n_pos;
    sh[1][threadIdx.x] = n_bad;
    sh[2][threadIdx.x] = spw;
    sh[3][threadIdx.x] = spwy;
    __syncthreads();
    for (int s = kSumsThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 4) out[threadIdx.x] = sh[threadIdx.x][0];
}

template <typename T>
__global__ __launch_bounds__(256) void irls_working_wo_kernel(const T* const* __restrict__ cols, int p, int bias, int64_t n,
                                                              const T* __restrict__ beta, IrlsArgs ia, const T* __restrict__ pw,
                                                              const T* __restrict__ off, T* __restrict__ w_out, T* __restrict__ z_out) {
    const gptr<T> cy = as_global(cols[p]);
    const T b0 = (bias && !ia.init) ? beta[p] : T(0);
    const T ymean = (T)ia.y_mean;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const T yv = cy[r];
        const T pwv = pw ? as_global(pw)[r] : T(1);
        const T ov = off ? as_global(off)[r] : T(0);
        T lin, mu;  // lin: the linear part of z
        if (ia.init) {
            mu = (ia.variance == 2) ? (yv + T(0.5)) * T(0.5) : (yv + ymean) * T(0.5);
            lin = glm_link<T>(ia.link, mu) - ov;
        } else {
            T acc = b0;
            for (int c = 0; c < p; ++c) acc += as_global(cols[c])[r] * beta[c];
            lin = acc;
            mu = glm_inv<T>(ia.link, acc + ov);
        }
        const T d = glm_deriv<T>(ia.link, mu);
        const bool on = pwv > T(0);
        w_out[r] = on ? pwv / (d * d * glm_var<T>(ia.variance, mu)) : T(0);
        z_out[r] = on ? lin + d * (yv - mu) : T(0);
    }
}

}  // namespace

template <typename T>
int launch_glm_wo_sums(pds_ctx* ctx, const T* d_y, const T* d_pw, int64_t n_rows, double* d_out4) {
    KernelTimer timer(ctx, kKindPass2);
    hipLaunchKernelGGL((glm_wo_sums_kernel<T>), dim3(1), dim3(kSumsThreads), 0, ctx->stream, d_y, d_pw, n_rows, d_out4);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_irls_working_wo(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int bias, const T* d_beta, const IrlsArgs& ia,
                           const T* d_pw, const T* d_off, T* d_w, T* d_z) {
    const int nb = (int)std::min<int64_t>(std::max<int64_t>((n_rows + 255) / 256, 1), (int64_t)ctx->num_cus * 8);
    KernelTimer timer(ctx, kKindPass2);
    hipLaunchKernelGGL((irls_working_wo_kernel<T>), dim3(nb), dim3(256), 0, ctx->stream, dc.d_ptrs, n_feat, bias, n_rows, d_beta, ia, d_pw,
                       d_off, d_w, d_z);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_glm_wo_sums<double>(pds_ctx*, const double*, const double*, int64_t, double*);
template int launch_glm_wo_sums<float>(pds_ctx*, const float*, const float*, int64_t, double*);
template int launch_irls_working_wo<double>(pds_ctx*, const DeviceCols<double>&, int, int64_t, int, const double*, const IrlsArgs&,
                                            const double*, const double*, double*, double*);
template int launch_irls_working_wo<float>(pds_ctx*, const DeviceCols<float>&, int, int64_t, int, const float*, const IrlsArgs&, const float*,
                                           const float*, float*, float*);

}  // namespace pds
