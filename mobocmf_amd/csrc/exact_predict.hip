// Predictive moments of fitted EXACT-GP surrogates (models/mfgp.py: MFGP, MFGP_lin) against a factorisation formed once, and
// the gradient w.r.t. the test points: mobocmf_exact_predict (include/mobocmf_hip.h), the model evaluation of the MES baseline's
// device acquisition search (MESMOC_MFGP(search="device"), util/exact_predict.py).  The shape is frozen_predict.hip's:
//
//   a WORKGROUP owns (model, a block of 16 test points); nothing is shared between workgroups: no in-launch barrier, no
//   counters, no atomics, no wait, no status word.
//
// Per block, with X the n training inputs, lev their levels and L^-1, a = L^-1 y of mobocmf_exact_gp_factor (read only):
//
//   k_r = S_r + N_r   S_r = sig[level] sig[lev_r] os_s exp(-1/2 |(x - X_r) / ls_s|^2)   N_r = ntab[min(level, lev_r)] os_n exp(-1/2 |(x - X_r) / ls_n|^2)
//   w = L^-1 k   mean = a^T w   var = kss - |w|^2
//   c = g_mean a - 2 g_var w   e = L^-T c   grad_j = -sum_r (x_j - X_rj) (e_r S_r / ls_s,j^2 + e_r N_r / ls_n,j^2)
//
// The two triangular products run on v_mfma_f64_16x16x4_f64 with L^-1 streamed from global memory (row-major as the
// factorisation leaves it: the transposed product reads it k-major, the forward one row by row; both mask the upper triangle
// and everything beyond n, so nothing outside the n x n lower triangle is ever an operand) and the two [n][16] panels in LDS:
// k -> w in turn, then c over w element by element, e over k, and the products e S / e N over both, from which thread
// (coordinate j, column) sums its gradient entry over the training rows in ascending order.  S and N are formed again there
// (two exponentials per element, as the k panel cost) instead of being kept: two panels are what bounds n at 512.
// MOBOCMF_STEP_INPUT_GRADIENTS forms its panels itself.  All LDS is dynamic (2 * 16 + 1 rows of nr doubles and EP_FIXED more).
#include <atomic>

#include "common.h"
#include "tile16.h"

namespace {

constexpr int ET = 512;                      // threads per workgroup: a thread per (coordinate <= 32, column) of the gradient
constexpr int ENW = ET / 64;
constexpr int ECW = 16;                      // columns of a panel and test points of a block
constexpr int EP_FIXED = ECW * MOBOCMF_MAX_D + 2 * MOBOCMF_MAX_D + 2 * MOBOCMF_EXACT_PREDICT_MAX_LEVELS + ENW * ECW * 2 + 2 * ECW;
static_assert(ET == ECW * MOBOCMF_MAX_D, "one thread per gradient entry of a block");
static_assert(MOBOCMF_EXACT_PREDICT_MAX_N % 16 == 0 && EP_FIXED % 2 == 0, "panels of whole tiles, 16-byte carving");

typedef const __attribute__((address_space(1))) double* gcd;
typedef const __attribute__((address_space(1))) int32_t* gci;
#define GC(p) ((gcd)(p))

// One 16 x 16 tile (rows 16 t ..) of L^-1 X (TRANS false: k tiles 0 .. t) or L^-T X (TRANS true: k tiles t .. nt - 1) for a
// panel X [k][16] in LDS; Li is the n x n lower triangle, row-major with leading dimension ld.  An operand outside the
// triangle is 0.0 without being read.
template <bool TRANS>
__device__ __forceinline__ v4d tile_lx(gcd Li, int64_t ld, int n, const double* X, int t, int nt, int lane) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    const int li = lane & 15, lk = lane >> 4, row = t * 16 + li;
    const int kt0 = TRANS ? t : 0, kt1 = TRANS ? nt : t + 1;
    for (int kt = kt0; kt < kt1; ++kt) {
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = kt * 16 + 4 * q + lk;
            const bool in = TRANS ? (k < n && k >= row) : (row < n && k <= row);
            a[q] = in ? (TRANS ? Li[(int64_t)k * ld + row] : Li[(int64_t)row * ld + k]) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = mfma(a[q], X[(kt * 16 + 4 * q + lk) * ECW + li], acc);
    }
    return acc;
}
__device__ __forceinline__ double xor_add(double v, int mask) { return v + __shfl_xor(v, mask); }
// the i-th output tile of wavefront w (frozen_predict.hip tile_of_wave: a lower and an upper triangular operand both give every
// wavefront the same number of k tiles)
__device__ __forceinline__ int tile_of_wave(int i, int w) { return (i & 1) ? i * ENW + ENW - 1 - w : i * ENW + w; }

template <bool INGRAD>
__global__ __launch_bounds__(ET) void exact_predict_kernel(const mobocmf_exact_predict_model* models) {
    extern __shared__ __attribute__((aligned(16))) double ep_lds[];
    const mobocmf_exact_predict_model& md = models[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int n = md.n, d = md.d, T = md.T, nl = md.n_levels, level = md.level;
    const int r0 = blockIdx.x * ECW;
    if (r0 >= T) return;      // (a launch's grid is sized for its largest model)
    const int nb = T - r0 < ECW ? T - r0 : ECW, nt = (n + 15) / 16, nr = nt * 16;
    double* X0 = ep_lds;
    double* X1 = X0 + nr * ECW;
    double* av = X1 + nr * ECW;
    double* xs = av + nr;                                   // [16][MOBOCMF_MAX_D]: the block's test points, zero padded
    double* ils = xs + ECW * MOBOCMF_MAX_D;                 // 1 / ls_s, 1 / ls_n
    double* iln = ils + MOBOCMF_MAX_D;
    double* sg = iln + MOBOCMF_MAX_D;                       // sig, ntab
    double* ntb = sg + MOBOCMF_EXACT_PREDICT_MAX_LEVELS;
    double* red = ntb + MOBOCMF_EXACT_PREDICT_MAX_LEVELS;   // [wavefront][column][2]
    double* gcol = red + ENW * ECW * 2;                     // the columns' seeds: g_mean, g_var
    gcd xtr = GC(md.xtr), Li = GC(md.Linv);
    gci lev = (gci)md.lev;
    const int64_t ld = md.ld;
    const double os_s = GC(md.hyp_s)[0], os_n = GC(md.hyp_n)[0];

    {
        const int c = tid / MOBOCMF_MAX_D, j = tid % MOBOCMF_MAX_D;
        xs[tid] = (c < nb && j < d) ? GC(md.x)[(int64_t)(r0 + c) * d + j] : 0.0;
        if (tid < MOBOCMF_MAX_D) ils[tid] = tid < d ? 1.0 / GC(md.hyp_s)[1 + tid] : 0.0;
        else if (tid < 2 * MOBOCMF_MAX_D) iln[tid - MOBOCMF_MAX_D] = tid - MOBOCMF_MAX_D < d ? 1.0 / GC(md.hyp_n)[1 + tid - MOBOCMF_MAX_D] : 0.0;
        else if (tid < 2 * MOBOCMF_MAX_D + MOBOCMF_EXACT_PREDICT_MAX_LEVELS) {
            const int l = tid - 2 * MOBOCMF_MAX_D;
            sg[l] = l < nl ? GC(md.sig)[l] : 0.0;
            ntb[l] = l < nl ? GC(md.ntab)[l] : 0.0;
        }
        for (int r = tid; r < nr; r += ET) av[r] = r < n ? GC(md.a)[r] : 0.0;
    }
    __syncthreads();

    // the signal and the noise term of k(x_c, X_r); a level outside the tables makes both NaN (and reads nothing)
    auto terms = [&](int r, int c, double& S, double& N) {
        const int lr = lev[r];
        if (lr < 0 || lr >= nl) {
            S = N = __builtin_nan("");
            return;
        }
        double qs = 0.0, qn = 0.0;
        for (int j = 0; j < d; ++j) {
            const double df = xs[c * MOBOCMF_MAX_D + j] - xtr[(int64_t)r * d + j];
            const double us = df * ils[j], un = df * iln[j];
            qs += us * us;
            qn += un * un;
        }
        S = sg[level] * sg[lr] * os_s * exp(-0.5 * qs);
        N = ntb[level < lr ? level : lr] * os_n * exp(-0.5 * qn);
    };

    // k
#pragma unroll 1
    for (int e = tid; e < nr * ECW; e += ET) {
        const int r = e >> 4, c = e & 15;
        double v = 0.0;
        if (r < n && c < nb) {
            double S, N;
            terms(r, c, S, N);
            v = S + N;
        }
        X0[e] = v;
    }
    __syncthreads();
    // w = L^-1 k
    for (int i = 0; i * ENW < nt; ++i) {
        const int t = tile_of_wave(i, wave);
        if (t < nt) {
            const v4d acc = tile_lx<false>(Li, ld, n, X0, t, nt, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) X1[(t * 16 + 4 * r + lk) * ECW + li] = acc[r];
        }
    }
    __syncthreads();
    // moments: a thread keeps one column and every 32nd row; summed through the wavefront, then over the wavefronts in order
    {
        const int cj = tid & 15;
        double q = 0.0, mu = 0.0;
        for (int m = tid >> 4; m < nr; m += ET / ECW) {
            const double w = X1[m * ECW + cj];
            q += w * w;
            mu += av[m] * w;
        }
        q = xor_add(xor_add(q, 16), 32);
        mu = xor_add(xor_add(mu, 16), 32);
        if (lane < ECW) {
            red[(wave * ECW + lane) * 2 + 0] = q;
            red[(wave * ECW + lane) * 2 + 1] = mu;
        }
    }
    __syncthreads();
    if (tid < ECW) {
        double gm = 0.0, gv = 0.0;
        if (tid < nb) {
            double q = 0.0, mu = 0.0;
#pragma unroll
            for (int p = 0; p < ENW; ++p) {
                q += red[(p * ECW + tid) * 2 + 0];
                mu += red[(p * ECW + tid) * 2 + 1];
            }
            md.top_mean[r0 + tid] = mu;
            md.top_var[r0 + tid] = md.kss - q;      // (no clamp, no floor: the host statement has none)
            if (INGRAD) {
                gm = GC(md.seed_gmean)[r0 + tid];
                gv = GC(md.seed_gvar)[r0 + tid];
            }
        }
        gcol[tid] = gm;
        gcol[ECW + tid] = gv;
    }
    if (!INGRAD) return;
    __syncthreads();
    // c = g_mean a - 2 g_var w (over w: an element of c needs the same element of w only)
    for (int e = tid; e < nr * ECW; e += ET) {
        const int r = e >> 4, c = e & 15;
        X1[e] = gcol[c] * av[r] - 2.0 * gcol[ECW + c] * X1[e];
    }
    __syncthreads();
    // e = L^-T c (over k)
    for (int i = 0; i * ENW < nt; ++i) {
        const int t = tile_of_wave(i, wave);
        if (t < nt) {
            const v4d acc = tile_lx<true>(Li, ld, n, X1, t, nt, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) X0[(t * 16 + 4 * r + lk) * ECW + li] = acc[r];
        }
    }
    __syncthreads();
    // e S over e, e N over c
#pragma unroll 1
    for (int e = tid; e < nr * ECW; e += ET) {
        const int r = e >> 4, c = e & 15;
        double ps = 0.0, pn = 0.0;
        if (r < n && c < nb) {
            double S, N;
            terms(r, c, S, N);
            const double ev = X0[e];
            ps = ev * S;
            pn = ev * N;
        }
        X0[e] = ps;
        X1[e] = pn;
    }
    __syncthreads();
    // grad[c][j]: one thread each, the training rows in ascending order
    {
        const int j = tid >> 4, c = tid & 15;
        if (j < d && c < nb) {
            const double xv = xs[c * MOBOCMF_MAX_D + j], is2 = ils[j] * ils[j], in2 = iln[j] * iln[j];
            double g = 0.0;
            for (int r = 0; r < n; ++r) g += (xv - xtr[(int64_t)r * d + j]) * (X0[r * ECW + c] * is2 + X1[r * ECW + c] * in2);
            md.grad[(int64_t)(r0 + c) * d + j] = -g;
        }
    }
}

inline size_t exact_lds_bytes(int n) { return ((size_t)(2 * ECW + 1) * ((n + 15) / 16 * 16) + EP_FIXED) * sizeof(double); }

template <bool INGRAD>
int launch_kernel(const mobocmf_exact_predict_model* dev_models, dim3 grid, size_t shm, hipStream_t s) {
    // the dynamic-LDS attribute is per device: one bit per device ordinal (frozen_predict.hip launch_kernel)
    static std::atomic<uint64_t> configured{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return MOBOCMF_HIP_ERROR;
    if (!(configured.load(std::memory_order_acquire) & (1ull << dev))) {
        if (hipFuncSetAttribute((const void*)exact_predict_kernel<INGRAD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)exact_lds_bytes(MOBOCMF_EXACT_PREDICT_MAX_N)) != hipSuccess)
            return MOBOCMF_HIP_ERROR;
        configured.fetch_or(1ull << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL(exact_predict_kernel<INGRAD>, grid, dim3(ET), shm, s, dev_models);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

bool mode_ok(int32_t mode) { return mode == MOBOCMF_STEP_FORWARD || mode == MOBOCMF_STEP_INPUT_GRADIENTS; }

bool sizes_ok(const mobocmf_exact_predict_model* m) {
    return m && m->n >= 1 && m->n <= MOBOCMF_EXACT_PREDICT_MAX_N && m->d >= 1 && m->d <= MOBOCMF_MAX_D && m->T >= 1 &&
           m->T <= MOBOCMF_TOPK_MAX_N && m->n_levels >= 1 && m->n_levels <= MOBOCMF_EXACT_PREDICT_MAX_LEVELS && m->level >= 0 &&
           m->level < m->n_levels && m->ld >= m->n;
}

}  // namespace

extern "C" {

int mobocmf_exact_predict_work_bytes(const mobocmf_exact_predict_model* model, int32_t mode, size_t* bytes) {
    if (!bytes || !sizes_ok(model) || !mode_ok(mode)) return MOBOCMF_BAD_ARG;
    *bytes = 0;      // both modes keep their panels in LDS
    return MOBOCMF_OK;
}

int mobocmf_exact_predict(const mobocmf_exact_predict_model* host_models, const mobocmf_exact_predict_model* dev_models,
                          int32_t n_models, int32_t mode, mobocmf_stream_t stream) {
    if (!host_models || !dev_models || n_models < 1 || n_models > 2 * MOBOCMF_ACQ_MAX_PAIRS || !mode_ok(mode)) return MOBOCMF_BAD_ARG;
    int nmax = 0, tmax = 0;
    for (int i = 0; i < n_models; ++i) {
        const mobocmf_exact_predict_model& m = host_models[i];
        if (!sizes_ok(&m) || !m.xtr || !m.lev || !m.sig || !m.ntab || !m.hyp_s || !m.hyp_n || !m.Linv || !m.a || !m.x ||
            !m.top_mean || !m.top_var)
            return MOBOCMF_BAD_ARG;
        if (mode == MOBOCMF_STEP_INPUT_GRADIENTS && (!m.seed_gmean || !m.seed_gvar || !m.grad)) return MOBOCMF_BAD_ARG;
        if (m.n > nmax) nmax = m.n;
        if (m.T > tmax) tmax = m.T;
    }
    const dim3 grid((unsigned)((tmax + ECW - 1) / ECW), (unsigned)n_models);
    const size_t shm = exact_lds_bytes(nmax);
    return mode == MOBOCMF_STEP_INPUT_GRADIENTS ? launch_kernel<true>(dev_models, grid, shm, (hipStream_t)stream)
                                                : launch_kernel<false>(dev_models, grid, shm, (hipStream_t)stream);
}

}  // extern "C"
