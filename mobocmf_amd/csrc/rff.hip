// Random-Fourier-feature function samples evaluated on a grid: the Pareto extraction of a sampled problem
// evaluates every sampled objective / constraint on 1000 d^2 + N points, recursing through the layers
// (mobocmf/layers/mfdgp_hidden_layer.py:326-337, :402-444; mobocmf/util/moop.py:232-272).
//
//   kind 0:  f(x) = sum_j theta[j] s0 cos(W1[j].x + b1[j])
//   kind 1:  f(x) = sum_j  theta[j]      s1 fprev cos(W1[j].x + b1[j])                 (s1 includes sqrt(nu): linear kernel)
//                        + theta[F+j]    s1f cos(W1[j].x + Wf[j] fprev + b1[j])         (RBF on [x, f], shares W1, b1)
//                        + theta[2F+j]   s2 cos(W2[j].x + b2[j])
//
// One thread per grid point (its x row in registers), features streamed through LDS in chunks and read as wave-wide
// broadcasts; the F x n feature matrix the reference materialises (and a library matmul + cos + matvec would, 256 MB per
// block at d = 8) never exists.  The argument W1.x is shared by the first two blocks of kind 1.  FP64 cos-bound.
#include "common.h"
#include "rff_desc.h"

#define RFF_T 256     // threads = grid points per workgroup
#define RFF_FC 64     // features per LDS chunk

template <int KIND, int DB>
__global__ __launch_bounds__(RFF_T) void rff_eval_kernel(int d, int F, int64_t n, const double* __restrict__ x,
                                                         const double* __restrict__ fprev, const double* __restrict__ W1,
                                                         const double* __restrict__ b1, const double* __restrict__ Wf,
                                                         const double* __restrict__ W2, const double* __restrict__ b2,
                                                         const double* __restrict__ theta, double s0, double s1, double s2,
                                                         double* __restrict__ out) {
    __shared__ double w1s[RFF_FC][DB], w2s[KIND ? RFF_FC : 1][DB];
    __shared__ double b1s[RFF_FC], b2s[RFF_FC], wfs[RFF_FC], t0s[RFF_FC], t1s[RFF_FC], t2s[RFF_FC];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * RFF_T + tid;
    const bool live = i < n;
    double xr[DB];
#pragma unroll
    for (int k = 0; k < DB; ++k) xr[k] = (live && k < d) ? x[i * d + k] : 0.0;
    const double fp = (KIND == 1 && live) ? fprev[i] : 0.0;
    double acc = 0.0;
    for (int f0 = 0; f0 < F; f0 += RFF_FC) {
        const int fc = F - f0 < RFF_FC ? F - f0 : RFF_FC;
        __syncthreads();
        for (int e = tid; e < fc * d; e += RFF_T) {
            const int j = e / d, k = e % d;
            w1s[j][k] = W1[(int64_t)(f0 + j) * d + k];
            if (KIND == 1) w2s[j][k] = W2[(int64_t)(f0 + j) * d + k];
        }
        if (tid < fc) {
            b1s[tid] = b1[f0 + tid];
            t0s[tid] = theta[f0 + tid];
            if (KIND == 1) {
                b2s[tid] = b2[f0 + tid];
                wfs[tid] = Wf[f0 + tid];
                t1s[tid] = theta[F + f0 + tid];
                t2s[tid] = theta[2 * F + f0 + tid];
            }
        }
        __syncthreads();
        for (int j = 0; j < fc; ++j) {
            double a1 = b1s[j], a2 = KIND == 1 ? b2s[j] : 0.0;
#pragma unroll
            for (int k = 0; k < DB; ++k) {
                if (k < d) {
                    a1 += w1s[j][k] * xr[k];
                    if (KIND == 1) a2 += w2s[j][k] * xr[k];
                }
            }
            if (KIND == 0) {
                acc += t0s[j] * cos(a1);
            } else {
                acc += t0s[j] * (s0 * fp) * cos(a1) + t1s[j] * s1 * cos(a1 + wfs[j] * fp) + t2s[j] * s2 * cos(a2);
            }
        }
    }
    if (live) out[i] = KIND == 0 ? s0 * acc : acc;
}

extern "C" int mobocmf_rff_eval(int32_t kind, int32_t d, int32_t F, int64_t n, const double* x, const double* fprev,
                                const double* W1, const double* b1, const double* Wf, const double* W2, const double* b2,
                                const double* theta, double s0, double s1, double s2, double* out,
                                mobocmf_stream_t stream) {
    if ((kind != 0 && kind != 1) || d < 1 || d > MOBOCMF_MAX_D || F < 1 || n < 1 || !x || !W1 || !b1 || !theta || !out)
        return MOBOCMF_BAD_ARG;
    if (kind == 1 && (!fprev || !Wf || !W2 || !b2)) return MOBOCMF_BAD_ARG;
    const dim3 grid((unsigned)((n + RFF_T - 1) / RFF_T)), block(RFF_T);
    hipStream_t s = (hipStream_t)stream;
#define RFF_GO(K, D) hipLaunchKernelGGL((rff_eval_kernel<K, D>), grid, block, 0, s, d, F, n, x, fprev, W1, b1, Wf, W2, b2, theta, s0, s1, s2, out)
    if (kind == 0) { if (d <= 2) RFF_GO(0, 2); else if (d <= 8) RFF_GO(0, 8); else RFF_GO(0, 32); }
    else { if (d <= 2) RFF_GO(1, 2); else if (d <= 8) RFF_GO(1, 8); else RFF_GO(1, 32); }
#undef RFF_GO
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

// ------------------------------------------------------------------ all chain samples on the grid in one launch
// The Pareto extraction evaluates every black-box's chain sample (layer 0, then the layers >= 1 recursing on it) at the same
// grid.  Grid (ceil(n / RFF_T), K): workgroup (b, k) takes rows b * RFF_T ... of sample k; a thread keeps its x row and the
// running layer value fprev in registers for all layers, and only the top layer's value is written.  One layer is exactly the
// arithmetic of rff_eval_kernel (same features per LDS chunk, same summation order), so the chained result equals the
// per-layer launches'.  The descriptor of (k, l) is uniform over the workgroup: every branch on it, and every barrier, is too.
template <int KIND, int DB>
__device__ __forceinline__ double rff_chain_layer(const mobocmf_rff_layer_desc& L, const double* __restrict__ P, int d,
                                                  const double (&xr)[DB], double fp, double (*w1s)[DB], double (*w2s)[DB],
                                                  double* b1s, double* b2s, double* wfs, double* t0s, double* t1s,
                                                  double* t2s) {
    const int tid = threadIdx.x, F = L.F;
    const double* W1 = P + L.W1;
    const double* b1 = P + L.b1;
    const double* th = P + L.theta;
    const double* Wf = P + L.Wf;
    const double* W2 = P + L.W2;
    const double* b2 = P + L.b2;
    const double s0 = L.s0, s1 = L.s1, s2 = L.s2;
    double acc = 0.0;
    for (int f0 = 0; f0 < F; f0 += RFF_FC) {
        const int fc = F - f0 < RFF_FC ? F - f0 : RFF_FC;
        __syncthreads();
        for (int e = tid; e < fc * d; e += RFF_T) {
            const int j = e / d, k = e % d;
            w1s[j][k] = W1[(int64_t)(f0 + j) * d + k];
            if (KIND == 1) w2s[j][k] = W2[(int64_t)(f0 + j) * d + k];
        }
        if (tid < fc) {
            b1s[tid] = b1[f0 + tid];
            t0s[tid] = th[f0 + tid];
            if (KIND == 1) {
                b2s[tid] = b2[f0 + tid];
                wfs[tid] = Wf[f0 + tid];
                t1s[tid] = th[F + f0 + tid];
                t2s[tid] = th[2 * F + f0 + tid];
            }
        }
        __syncthreads();
        for (int j = 0; j < fc; ++j) {
            double a1 = b1s[j], a2 = KIND == 1 ? b2s[j] : 0.0;
#pragma unroll
            for (int k = 0; k < DB; ++k) {
                if (k < d) {
                    a1 += w1s[j][k] * xr[k];
                    if (KIND == 1) a2 += w2s[j][k] * xr[k];
                }
            }
            if (KIND == 0) {
                acc += t0s[j] * cos(a1);
            } else {
                acc += t0s[j] * (s0 * fp) * cos(a1) + t1s[j] * s1 * cos(a1 + wfs[j] * fp) + t2s[j] * s2 * cos(a2);
            }
        }
    }
    return KIND == 0 ? s0 * acc : acc;
}

template <int DB>
__global__ __launch_bounds__(RFF_T) void rff_eval_chains_kernel(int d, int64_t n, const double* __restrict__ x,
                                                                const double* __restrict__ P, int64_t plen,
                                                                const mobocmf_rff_layer_desc* __restrict__ desc,
                                                                double* __restrict__ out) {
    __shared__ double w1s[RFF_FC][DB], w2s[RFF_FC][DB];
    __shared__ double b1s[RFF_FC], b2s[RFF_FC], wfs[RFF_FC], t0s[RFF_FC], t1s[RFF_FC], t2s[RFF_FC];
    const int k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * RFF_T + threadIdx.x;
    const bool live = i < n;
    double xr[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c) xr[c] = (live && c < d) ? x[i * d + c] : 0.0;
    double fp = 0.0;
    for (int l = 0; l < MOBOCMF_RFF_MAX_LAYERS; ++l) {
        const mobocmf_rff_layer_desc L = desc[(int64_t)k * MOBOCMF_RFF_MAX_LAYERS + l];
        if (L.kind < 0 && l > 0) break;
        if (!rff_desc_ok(L, l, d, plen)) {
            fp = __builtin_nan("");
            break;
        }
        fp = L.kind == 0 ? rff_chain_layer<0, DB>(L, P, d, xr, fp, w1s, w2s, b1s, b2s, wfs, t0s, t1s, t2s)
                         : rff_chain_layer<1, DB>(L, P, d, xr, fp, w1s, w2s, b1s, b2s, wfs, t0s, t1s, t2s);
    }
    if (live) out[(int64_t)k * n + i] = fp;
}

extern "C" int mobocmf_rff_eval_chains(int32_t K, int32_t d, int64_t n, const double* x, const double* params,
                                       int64_t params_len, const mobocmf_rff_layer_desc* desc, double* out,
                                       mobocmf_stream_t stream) {
    if (K < 1 || K > 65535 || d < 1 || d > MOBOCMF_MAX_D || n < 1 || params_len < 1 || !x || !params || !desc || !out)
        return MOBOCMF_BAD_ARG;
    const dim3 grid((unsigned)((n + RFF_T - 1) / RFF_T), (unsigned)K), block(RFF_T);
    hipStream_t s = (hipStream_t)stream;
#define RFFC_GO(D) hipLaunchKernelGGL((rff_eval_chains_kernel<D>), grid, block, 0, s, d, n, x, params, params_len, desc, out)
    if (d <= 2) RFFC_GO(2); else if (d <= 8) RFFC_GO(8); else RFFC_GO(32);
#undef RFFC_GO
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

__global__ __launch_bounds__(RFF_T) void rff_feasibility_kernel(int K_con, int64_t n, const double* __restrict__ vals,
                                                                int64_t ldv, const double* __restrict__ thr,
                                                                int32_t* __restrict__ ok, double* __restrict__ viol) {
    const int64_t i = (int64_t)blockIdx.x * RFF_T + threadIdx.x;
    if (i >= n) return;
    bool all = true;
    double v = 0.0;
    for (int c = 0; c < K_con; ++c) {
        const double slack = vals[(int64_t)c * ldv + i] - thr[c];
        all = all && slack >= 0.0;
        v += slack < 0.0 ? slack : 0.0;
    }
    ok[i] = all ? 1 : 0;
    viol[i] = v;
}

extern "C" int mobocmf_rff_feasibility(int32_t K_con, int64_t n, const double* vals, int64_t ldv, const double* thr,
                                       int32_t* ok, double* viol, mobocmf_stream_t stream) {
    if (K_con < 1 || n < 1 || ldv < n || !vals || !thr || !ok || !viol) return MOBOCMF_BAD_ARG;
    const dim3 grid((unsigned)((n + RFF_T - 1) / RFF_T)), block(RFF_T);
    hipLaunchKernelGGL(rff_feasibility_kernel, grid, block, 0, (hipStream_t)stream, K_con, n, vals, ldv, thr, ok, viol);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}
