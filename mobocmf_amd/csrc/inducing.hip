// Inducing-point selection by greedy conditional variance: the incomplete pivoted Cholesky of K_nn under the kind-0 kernel
// (Burt, Rasmussen, van der Wilk 2020).  Step j picks the row p with the largest residual d_p = diag(K - L L^T)_p (of
// bitwise-equal residuals the lowest row), forms the new column
//     l = (k(X, x_p) - L[:, :j] L[p, :j]^T) / sqrt(d_p),      l_p = sqrt(d_p),
// and updates d = max(d - l*l, 0), d_p = 0.  It stops before a pick whose residual is <= tol_rel * a (or not positive).
//
// L is kept [max_points][N] (n-contiguous): row i's dot product reads L[t][i] for t = 0..j-1, coalesced over a wavefront, and
// runs in ONE thread in ascending t -- the same instruction sequence in both forms, so they agree bitwise.  The pivot row's
// L[p][0..j-1] (a strided gather of j doubles) and x_p are staged in LDS once per workgroup and step.
//
// Form 1 (is_one_wg_kernel): one workgroup of 1024 threads, one launch, all steps; __syncthreads between steps.
// Form 2 (is_step_kernel):   one launch per pivot.  The launch of step j first reduces the (value, row) partials the workgroups
//   of the previous launch left (every workgroup does so redundantly: at most 1024 pairs), applies the stop rule, computes
//   column j for its rows and leaves its own partial for step j + 1 in the other half of a ping-pong buffer.  No workgroup
//   ever waits on another, and no word is read in the launch that writes it; the pivot never visits the host.  The launch that
//   stops leaves "stopped" partials instead, which every later launch finds, hands on and returns.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)      // the roundings below are part of the result's definition (explicit fma where wanted)

#define IS_T1 1024                  // threads of the one-workgroup form
#define IS_MAXG 1024                // most workgroups (partials) of the per-pivot form
#define IS_STOPPED INT32_MAX        // row of a partial left by a launch at or after the stop (its value is -1)
#define IS_HDR 32768                // workspace header: control words + 2 x IS_MAXG (double, int32) partials
#define IS_ONE_WG_MAX_N 512         // form 0 (automatic): the one-workgroup form up to this many rows (measured)
#define IS_UNROLL 16                // loads of a row's dot product in flight

enum { IS_INFO_X = 1, IS_INFO_HYP = 2 };    // info: non-finite x | non-finite / non-positive hyper-parameter

__device__ __forceinline__ bool is_better(double v, int32_t i, double bv, int32_t bi) {
    return v > bv || (v == bv && i < bi);
}

// (largest value, lowest row) over the workgroup; every thread returns the result.  red_v / red_i: one slot per wavefront.
__device__ __forceinline__ void is_block_best(double& v, int32_t& i, double* red_v, int32_t* red_i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s);
        const int32_t oi = __shfl_xor(i, s);
        if (is_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int nw = (int)(blockDim.x >> 6);
    if (nw == 1) return;
    __syncthreads();                                  // the slots' previous readers are done
    if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = v; red_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = red_v[0]; i = red_i[0];
    for (int w = 1; w < nw; ++w)
        if (is_better(red_v[w], red_i[w], v, i)) { v = red_v[w]; i = red_i[w]; }
}

// sum_t L[t][i] * lp[t], t = 0..j-1 ascending, one fma each; col = L + i, ld = N
__device__ __forceinline__ double is_row_dot(const double* __restrict__ col, int64_t ld, const double* lp, int j) {
    double acc = 0.0;
    int t = 0;
    for (; t + IS_UNROLL <= j; t += IS_UNROLL) {
        double v[IS_UNROLL];
#pragma unroll
        for (int u = 0; u < IS_UNROLL; ++u) v[u] = col[(int64_t)(t + u) * ld];
#pragma unroll
        for (int u = 0; u < IS_UNROLL; ++u) acc = fma(v[u], lp[t + u], acc);
    }
    for (; t < j; ++t) acc = fma(col[(int64_t)t * ld], lp[t], acc);
    return acc;
}

// gram.hip's kind 0: a * exp(-1/2 sum_k ((x_k - z_k) / ls_k)^2), with 1 / ls_k formed once
__device__ __forceinline__ double is_kval(const double* __restrict__ xi, const double* xp, const double* il, int d, double a) {
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const double t = (xi[k] - xp[k]) * il[k];
        s = fma(t, t, s);
    }
    return a * exp(-0.5 * s);
}

// one row of step j: the new column entry and the row's residual after it
__device__ __forceinline__ double is_update_row(int64_t i, int32_t p, double dp, double sq, int64_t N, int d, int j,
                                                const double* __restrict__ x, const double* xp, const double* il, double a,
                                                const double* lp, double* __restrict__ L, double* __restrict__ diag) {
    double l, dn;
    if (i == p) {
        l = sq;
        dn = 0.0;
    } else {
        const double dot = is_row_dot(L + i, N, lp, j);
        l = (is_kval(x + i * d, xp, il, d, a) - dot) / sq;
        dn = diag[i] - l * l;
        dn = dn > 0.0 ? dn : 0.0;                     // clamps NaN too
    }
    L[(int64_t)j * N + i] = l;
    diag[i] = dn;
    return dn;
}

__device__ __forceinline__ int is_hyp_code(const double* hyp, int k) {      // entry k of [a, ls[0..d)]
    const double h = hyp[k];
    const bool ok = isfinite(h) && h > 0.0 && (k == 0 || isfinite(1.0 / h));
    return ok ? 0 : IS_INFO_HYP;
}

// ------------------------------------------------------------------ form 1: one workgroup, one launch
__global__ __launch_bounds__(IS_T1) void is_one_wg_kernel(int64_t N, int d, const double* __restrict__ x,
                                                          const double* __restrict__ hyp, int max_points, double tol_rel,
                                                          double* __restrict__ L, int32_t* __restrict__ idx,
                                                          int32_t* __restrict__ count, double* __restrict__ resid,
                                                          double* __restrict__ diag, int32_t* __restrict__ info) {
    __shared__ double lp[MOBOCMF_INDUCING_MAX_POINTS];
    __shared__ double xp[MAX_D], il[MAX_D];
    __shared__ double red_v[IS_T1 / 64];
    __shared__ int32_t red_i[IS_T1 / 64];
    __shared__ int32_t bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    int code = 0;
    for (int64_t e = tid; e < N * d; e += IS_T1)
        if (!isfinite(x[e])) code = IS_INFO_X;
    if (tid <= d) code |= is_hyp_code(hyp, tid);
    if (code) atomicOr(&bad, code);
    __syncthreads();
    code = bad;
    if (code) {                                       // refused: every output marked
        const double qnan = __builtin_nan("");
        for (int64_t i = tid; i < N; i += IS_T1) diag[i] = qnan;
        for (int t = tid; t < max_points; t += IS_T1) { idx[t] = -1; resid[t] = qnan; }
        if (tid == 0) { *count = 0; *info = (code & IS_INFO_X) ? IS_INFO_X : IS_INFO_HYP; }
        return;
    }
    const double a = hyp[0];
    const double thresh = fmax(tol_rel * a, 0.0);
    if (tid < d) il[tid] = 1.0 / hyp[1 + tid];
    for (int64_t i = tid; i < N; i += IS_T1) diag[i] = a;
    for (int t = tid; t < max_points; t += IS_T1) { idx[t] = -1; resid[t] = 0.0; }
    double v = tid < N ? a : -1.0;
    int32_t bi = tid < N ? tid : INT32_MAX;
    int j = 0;
    for (; j < max_points; ++j) {
        is_block_best(v, bi, red_v, red_i);
        const double dp = v;
        const int32_t p = bi;
        if (!(dp > thresh) || p < 0 || p >= N) break;                 // uniform
        if (tid == 0) { idx[j] = p; resid[j] = dp; }
        for (int t = tid; t < j; t += IS_T1) lp[t] = L[(int64_t)t * N + p];
        if (tid < d) xp[tid] = x[(int64_t)p * d + tid];
        __syncthreads();
        const double sq = sqrt(dp);
        v = -1.0;
        bi = INT32_MAX;
        for (int64_t i = tid; i < N; i += IS_T1) {
            const double dn = is_update_row(i, p, dp, sq, N, d, j, x, xp, il, a, lp, L, diag);
            if (is_better(dn, (int32_t)i, v, bi)) { v = dn; bi = (int32_t)i; }
        }
        // lp / xp are rewritten only after the two barriers of the next is_block_best
    }
    if (tid == 0) { *count = j; *info = 0; }
}

// ------------------------------------------------------------------ form 2: one launch per pivot
// control word (workspace header): ctl[1] = refusal code, zeroed by launch_zero32 before is_init_kernel, which alone writes it.
__global__ __launch_bounds__(256) void is_init_kernel(int64_t N, int d, const double* __restrict__ x,
                                                      const double* __restrict__ hyp, int G, int rows_per_wg,
                                                      int max_points, double* __restrict__ diag,
                                                      double* __restrict__ part_v, int32_t* __restrict__ part_i,
                                                      int32_t* __restrict__ ctl, int32_t* __restrict__ count) {
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    int code = 0;
    for (int64_t e = gt; e < N * d; e += nt)
        if (!isfinite(x[e])) code = IS_INFO_X;
    if (gt <= d) code |= is_hyp_code(hyp, (int)gt);
    if (code) atomicOr(ctl + 1, code);
    const double a = hyp[0];
    if (gt == 0) *count = max_points;                 // until a launch stops earlier
    for (int64_t i = gt; i < N; i += nt) diag[i] = a;
    for (int64_t g = gt; g < G; g += nt) {            // step 0: every residual is a, the lowest row of each workgroup
        part_v[g] = a;
        part_i[g] = (int32_t)(g * rows_per_wg);
    }
}

template <int T>
__global__ __launch_bounds__(T) void is_step_kernel(int64_t N, int d, const double* __restrict__ x,
                                                    const double* __restrict__ hyp, int max_points, double tol_rel, int j,
                                                    int G, double* __restrict__ L, double* __restrict__ diag,
                                                    double* __restrict__ part_v, int32_t* __restrict__ part_i,
                                                    int32_t* __restrict__ ctl, int32_t* __restrict__ idx,
                                                    int32_t* __restrict__ count, double* __restrict__ resid) {
    __shared__ double lp[MOBOCMF_INDUCING_MAX_POINTS];
    __shared__ double xp[MAX_D], il[MAX_D];
    __shared__ double red_v[T / 64];
    __shared__ int32_t red_i[T / 64];
    if (ctl[1] != 0) return;                          // written by is_init_kernel only: the same in every wavefront
    const int tid = threadIdx.x;
    const double* pv = part_v + (j & 1) * IS_MAXG;
    const int32_t* pi = part_i + (j & 1) * IS_MAXG;
    double v = -1.0;
    int32_t bi = INT32_MAX;
    for (int g = tid; g < G; g += T)
        if (is_better(pv[g], pi[g], v, bi)) { v = pv[g]; bi = pi[g]; }
    is_block_best(v, bi, red_v, red_i);
    const double dp = v;
    const int32_t p = bi;
    const double a = hyp[0];
    // The decision comes out of is_block_best, after its barriers: the same in every thread of every workgroup.  A clamped
    // residual is never NaN or negative, so a real row always beats the start value and p == IS_STOPPED means just that.
    if (!(dp > fmax(tol_rel * a, 0.0)) || p < 0 || p >= N) {
        if (tid == 0) {
            if (blockIdx.x == 0 && p != IS_STOPPED) *count = j;       // the launch that stops; later ones only hand on
            part_v[((j + 1) & 1) * IS_MAXG + blockIdx.x] = -1.0;
            part_i[((j + 1) & 1) * IS_MAXG + blockIdx.x] = IS_STOPPED;
        }
        return;
    }
    if (blockIdx.x == 0 && tid == 0) {
        idx[j] = p;
        resid[j] = dp;
    }
    for (int t = tid; t < j; t += T) lp[t] = L[(int64_t)t * N + p];
    if (tid < d) { xp[tid] = x[(int64_t)p * d + tid]; il[tid] = 1.0 / hyp[1 + tid]; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * T + tid;
    v = -1.0;
    bi = INT32_MAX;
    if (i < N) {
        v = is_update_row(i, p, dp, sqrt(dp), N, d, j, x, xp, il, a, lp, L, diag);
        bi = (int32_t)i;
    }
    is_block_best(v, bi, red_v, red_i);
    if (tid == 0) {
        part_v[((j + 1) & 1) * IS_MAXG + blockIdx.x] = v;
        part_i[((j + 1) & 1) * IS_MAXG + blockIdx.x] = bi;
    }
}

// info, and on a refusal every output marked; otherwise the unused tails of idx / resid
__global__ __launch_bounds__(256) void is_finish_kernel(int64_t N, int max_points, const int32_t* __restrict__ ctl,
                                                        int32_t* __restrict__ idx, int32_t* __restrict__ count,
                                                        double* __restrict__ resid, double* __restrict__ diag,
                                                        int32_t* __restrict__ info) {
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    const int code = ctl[1];
    if (code) {
        const double qnan = __builtin_nan("");
        for (int64_t i = gt; i < N; i += nt) diag[i] = qnan;
        for (int64_t t = gt; t < max_points; t += nt) { idx[t] = -1; resid[t] = qnan; }
        if (gt == 0) { *count = 0; *info = (code & IS_INFO_X) ? IS_INFO_X : IS_INFO_HYP; }
        return;
    }
    const int c = *count;
    for (int64_t t = gt; t < max_points; t += nt)
        if (t >= c) { idx[t] = -1; resid[t] = 0.0; }
    if (gt == 0) *info = 0;
}

static bool is_shape_ok(int64_t N, int32_t max_points) {
    return N >= 1 && N <= MOBOCMF_INDUCING_MAX_ROWS && max_points >= 1 && max_points <= MOBOCMF_INDUCING_MAX_POINTS &&
           max_points <= N;
}

extern "C" int mobocmf_select_inducing_workspace_bytes(int64_t N, int32_t max_points, size_t* bytes) {
    if (!bytes || !is_shape_ok(N, max_points)) return MOBOCMF_BAD_ARG;
    *bytes = (size_t)IS_HDR + (size_t)N * (size_t)max_points * sizeof(double);
    return MOBOCMF_OK;
}

extern "C" int mobocmf_select_inducing(int64_t N, int32_t d, const double* x, const double* hyp, int32_t max_points,
                                       double tol_rel, int32_t form, int32_t* idx, int32_t* count, double* resid,
                                       double* diag, int32_t* info, void* workspace, size_t workspace_bytes,
                                       mobocmf_stream_t stream) {
    if (!is_shape_ok(N, max_points) || d < 1 || d > MOBOCMF_MAX_D || form < 0 || form > 2 || !(tol_rel >= 0.0) ||
        !isfinite(tol_rel))
        return MOBOCMF_BAD_ARG;
    if (!x || !hyp || !idx || !count || !resid || !diag || !info || !workspace) return MOBOCMF_BAD_ARG;
    if (workspace_bytes < (size_t)IS_HDR + (size_t)N * (size_t)max_points * sizeof(double)) return MOBOCMF_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* ctl = (int32_t*)ws;
    double* part_v = (double*)(ws + 256);
    int32_t* part_i = (int32_t*)(ws + 256 + 2 * IS_MAXG * sizeof(double));
    double* L = (double*)(ws + IS_HDR);
    if (form == 1 && N > MOBOCMF_INDUCING_ONE_WG_MAX_ROWS) return MOBOCMF_BAD_ARG;     // one CU for minutes: refused
    if (form == 0) form = N <= IS_ONE_WG_MAX_N ? 1 : 2;
    if (form == 1) {
        hipLaunchKernelGGL(is_one_wg_kernel, dim3(1), dim3(IS_T1), 0, s, N, (int)d, x, hyp, (int)max_points, tol_rel, L, idx,
                           count, resid, diag, info);
        HIP_TRY(hipGetLastError());
        return MOBOCMF_OK;
    }
    const int T = N <= 16384 ? 64 : 256;
    const int G = (int)((N + T - 1) / T);             // <= IS_MAXG by MOBOCMF_INDUCING_MAX_ROWS
    int rc = launch_zero32(ctl, 2, s);
    if (rc != MOBOCMF_OK) return rc;
    const int gi = (int)((N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024);
    hipLaunchKernelGGL(is_init_kernel, dim3(gi), dim3(256), 0, s, N, (int)d, x, hyp, G, T, (int)max_points, diag, part_v, part_i,
                       ctl, count);
    for (int j = 0; j < max_points; ++j) {
#define IS_GO(TT)                                                                                                          \
    hipLaunchKernelGGL((is_step_kernel<TT>), dim3(G), dim3(TT), 0, s, N, (int)d, x, hyp, (int)max_points, tol_rel, j, G, L, \
                       diag, part_v, part_i, ctl, idx, count, resid)
        if (T == 64) IS_GO(64);
        else IS_GO(256);
#undef IS_GO
    }
    hipLaunchKernelGGL(is_finish_kernel, dim3(gi), dim3(256), 0, s, N, (int)max_points, ctl, idx, count, resid, diag, info);
    HIP_TRY(hipGetLastError());
    return MOBOCMF_OK;
}
