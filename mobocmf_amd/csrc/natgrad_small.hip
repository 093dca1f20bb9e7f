// Natural-gradient step of q(u) = N(m, L_S L_S^T) for SMALL layers (M <= 128), the whole update of one layer by ONE workgroup and
// every layer of a step object in ONE launch ("Natural gradients in the one-launch steps").  Same algebra as
// natgrad.hip:
//   P     = tril(L_S^T tril(g_LS))           B = I + gamma_t scale (tril(P) + tril(P, -1)^T)   (= I + 2 gamma_t scale Psi)
//   J B J = C C^T  (J reverses the M indices),  T = J C^-T J  lower, T T^T = B^-1
//   L_new = L_S T                            m_new = m - gamma_t scale L_new (L_new^T g_m)
// Two families, chosen per workgroup from the layer's M:
//   M <= 32:  full 32 x 32 matrices in LDS (row stride 33), plain FP64 FMA;
//   M <= 128: lower triangles packed as swizzled 16 x 16 tiles (tile16.h), two of them in LDS (X: L_S, later L_new; Y: g_LS,
//             then J B J -> C -> C^-1 in place), the products on v_mfma_f64_16x16x4_f64, the pivot blocks by chol_inv_tile16;
//             the inverses of the pivot blocks wait in `work` between the factorisation and the inversion.
// Workgroup barriers only; nothing waits for another workgroup.  No atomics, fixed summation orders, nothing read on the host.
#include <math.h>

#include "common.h"
#include "natgrad_schedule.h"
#include "tile16.h"

#define NGS_THREADS 512
#define NGS_WAVES (NGS_THREADS / 64)
#define NGS_SMALL_M 32
#define NGS_LD 33                                  // row stride of the small family's matrices
#define NGS_MAX_M MOBOCMF_NATGRAD_SMALL_MAX_M
#define NGS_TILE_SLOTS 5                           // ceil(36 tiles of M = 128 / NGS_WAVES)
// LDS, in doubles: [0] gamma_t scale, [1] two ints (guard, failed pivot), [2] the step count; then g_m, v and the 4 partial
// sums of the matrix-vector products; then the pivot block's inverse; then the matrices
#define NGS_VEC 8
#define NGS_PART (NGS_VEC + 2 * NGS_MAX_M)
#define NGS_D0 (NGS_PART + 4 * NGS_MAX_M)
#define NGS_MAT (NGS_D0 + 256)

typedef mobocmf_natgrad_small_layer NgsLayer;

static_assert(NGS_TILE_SLOTS * NGS_WAVES >= (NGS_MAX_M / 16) * (NGS_MAX_M / 16 + 1) / 2, "every tile needs a wavefront slot");
static_assert(NGS_MAX_M / 16 <= NGS_WAVES, "one wavefront per tile of a panel");

namespace {

size_t ngs_lds_bytes(int M) {
    const int nt = (M + 15) / 16;
    const size_t mat = M <= NGS_SMALL_M ? (size_t)5 * NGS_SMALL_M * NGS_LD : (size_t)2 * (nt * (nt + 1) / 2) * 256;
    return (NGS_MAT + mat) * sizeof(double);
}

// tile (ti, tj <= ti) of the packed index t = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void ngs_tile_of(int t, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

// v = N^T g, w = N v (N lower triangular, read through `at`), m -= gs w, L_S <- N on the lower triangle.  Four row / column
// classes per sum, added in a fixed order.
template <class At>
__device__ __forceinline__ void ngs_write_back(const NgsLayer& ly, double gs, double* lds, At at) {
    const int M = ly.M, tid = threadIdx.x;
    const double* gv = lds + NGS_VEC;
    double* vv = lds + NGS_VEC + NGS_MAX_M;
    double* part = lds + NGS_PART;
    const int c = tid & (NGS_MAX_M - 1), p = tid >> 7;
    {
        double acc = 0.0;
        if (c < M)
            for (int i = c + p; i < M; i += 4) acc += at(i, c) * gv[i];
        part[p * NGS_MAX_M + c] = acc;
    }
    __syncthreads();
    if (tid < M) vv[tid] = (part[tid] + part[NGS_MAX_M + tid]) + (part[2 * NGS_MAX_M + tid] + part[3 * NGS_MAX_M + tid]);
    __syncthreads();
    {
        double acc = 0.0;
        if (c < M)
            for (int j = p; j <= c; j += 4) acc += at(c, j) * vv[j];
        part[p * NGS_MAX_M + c] = acc;
    }
    __syncthreads();
    if (tid < M)
        ly.m[tid] -= gs * ((part[tid] + part[NGS_MAX_M + tid]) + (part[2 * NGS_MAX_M + tid] + part[3 * NGS_MAX_M + tid]));
    for (int e = tid; e < M * M; e += NGS_THREADS) {
        const int i = e / M, j = e - i * M;
        if (j <= i) ly.L_S[e] = at(i, j);
    }
}

// ---- M <= 32.  Returns the failed pivot of J B J (1-based) or 0, the same value in every thread.
__device__ int ngs_small(const NgsLayer& ly, double gs, double* lds) {
    const int M = ly.M, tid = threadIdx.x;
    double* gv = lds + NGS_VEC;
    double* sL = lds + NGS_MAT;                    // tril(L_S)
    double* sG = sL + NGS_SMALL_M * NGS_LD;        // tril(g_LS), later L_new
    double* sB = sG + NGS_SMALL_M * NGS_LD;        // J B J, consumed by the factorisation
    double* sC = sB + NGS_SMALL_M * NGS_LD;        // C (lower)
    double* sI = sC + NGS_SMALL_M * NGS_LD;        // C^-1 (lower)
    for (int e = tid; e < M * M; e += NGS_THREADS) {
        const int i = e / M, j = e - i * M;
        double l = 0.0, g = 0.0;
        if (j <= i) {
            l = ly.L_S[e];
            g = ly.g_LS[e];
        }
        sL[i * NGS_LD + j] = l;
        sG[i * NGS_LD + j] = g;
    }
    if (tid < M) gv[tid] = ly.g_m[tid];
    __syncthreads();
    for (int e = tid; e < M * M; e += NGS_THREADS) {
        const int i = e / M, j = e - i * M;
        if (j <= i) {
            double p = 0.0;
            for (int k = i; k < M; ++k) p += sL[k * NGS_LD + i] * sG[k * NGS_LD + j];
            sB[(M - 1 - j) * NGS_LD + (M - 1 - i)] = (i == j ? 1.0 : 0.0) + gs * p;
        }
    }
    __syncthreads();
    // right-looking Cholesky, one barrier per column: the scaled column goes to sC, the trailing update reads the unscaled one
    for (int j = 0; j < M; ++j) {
        const double d = sB[j * NGS_LD + j];
        if (!(d > 0.0) || !(d < INFINITY)) return j + 1;      // (every thread reads the same word)
        const double r = 1.0 / sqrt(d);
        const int n = M - 1 - j;
        for (int e = tid; e < n * n; e += NGS_THREADS) {
            const int a = e / n, i = j + 1 + a, k = j + 1 + (e - a * n);
            if (k <= i) sB[i * NGS_LD + k] -= (sB[i * NGS_LD + j] * r) * (sB[k * NGS_LD + j] * r);
        }
        for (int i = j + tid; i < M; i += NGS_THREADS) sC[i * NGS_LD + j] = sB[i * NGS_LD + j] * r;
        __syncthreads();
    }
    // C^-1 by forward substitution, one thread per column
    if (tid < M) {
        const int c = tid;
        for (int i = c; i < M; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= sC[i * NGS_LD + k] * sI[k * NGS_LD + c];
            sI[i * NGS_LD + c] = s / sC[i * NGS_LD + i];
        }
    }
    __syncthreads();
    // L_new = L_S T, T[k][j] = C^-1[M-1-j][M-1-k]
    for (int e = tid; e < M * M; e += NGS_THREADS) {
        const int i = e / M, j = e - i * M;
        if (j <= i) {
            double s = 0.0;
            for (int k = j; k <= i; ++k) s += sL[i * NGS_LD + k] * sI[(M - 1 - j) * NGS_LD + (M - 1 - k)];
            sG[i * NGS_LD + j] = s;
        }
    }
    __syncthreads();
    ngs_write_back(ly, gs, lds, [sG](int i, int j) { return sG[i * NGS_LD + j]; });
    return 0;
}

// ---- 32 < M <= 128.  Returns the failed pivot of J B J (1-based) or 0, the same value in every thread.
__device__ int ngs_tiled(const NgsLayer& ly, double gs, double* lds) {
    const int M = ly.M, tid = threadIdx.x;
    const int nt = (M + 15) >> 4, ntri = nt * (nt + 1) / 2;
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    double* gv = lds + NGS_VEC;
    int* flags = (int*)(lds + 1);
    double* D0 = lds + NGS_D0;
    double* X = lds + NGS_MAT;
    double* Y = X + ntri * 256;
    for (int e = tid; e < ntri * 256; e += NGS_THREADS) {
        int ti, tj;
        ngs_tile_of(e >> 8, ti, tj);
        const int r = (e >> 4) & 15, c = e & 15, i = 16 * ti + r, j = 16 * tj + c;
        double l = 0.0, g = 0.0;
        if (i < M && j <= i) {
            l = ly.L_S[(int64_t)i * M + j];
            g = ly.g_LS[(int64_t)i * M + j];
        }
        X[(e & ~255) + tel(r, c)] = l;
        Y[(e & ~255) + tel(r, c)] = g;
    }
    if (tid < M) gv[tid] = ly.g_m[tid];
    __syncthreads();
    // P = tril(L^T G): tile (ti, tj) = sum_{tk >= ti} L(tk, ti)^T G(tk, tj), held in registers until G may be overwritten
    v4d acc[NGS_TILE_SLOTS];
#pragma unroll
    for (int q = 0; q < NGS_TILE_SLOTS; ++q) {
        acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
        const int t = wave + NGS_WAVES * q;
        if (t < ntri) {
            int ti, tj;
            ngs_tile_of(t, ti, tj);
            for (int tk = ti; tk < nt; ++tk) {
                const double* A = X + tix(tk, ti);
                const double* B = Y + tix(tk, tj);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[q] = mfma(A[tel(4 * k + lk, li)], B[tel(4 * k + lk, li)], acc[q]);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < ntri * 256; e += NGS_THREADS) {
        int ti, tj;
        ngs_tile_of(e >> 8, ti, tj);
        const int r = (e >> 4) & 15, c = e & 15;
        Y[(e & ~255) + tel(r, c)] = (ti == tj && r == c) ? 1.0 : 0.0;      // identity: the padding of J B J
    }
    __syncthreads();
    // J B J [M-1-b][M-1-a] = delta + gs P[a][b], a >= b
#pragma unroll
    for (int q = 0; q < NGS_TILE_SLOTS; ++q) {
        const int t = wave + NGS_WAVES * q;
        if (t < ntri) {
            int ti, tj;
            ngs_tile_of(t, ti, tj);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = 16 * ti + 4 * r + lk, b = 16 * tj + li;
                if (a < M && b <= a) {
                    const int i = M - 1 - b, j = M - 1 - a;
                    Y[tix(i >> 4, j >> 4) + tel(i & 15, j & 15)] = (a == b ? 1.0 : 0.0) + gs * acc[q][r];
                }
            }
        }
    }
    __syncthreads();
    // J B J = C C^T in place, right-looking by 16-wide block columns
    for (int s = 0; s < nt; ++s) {
        if (wave == 0) {
            double* Dss = Y + tix(s, s);
            int f = chol_inv_tile16(Dss, D0, lane);
            // lanes 0-15 wrote the factor: the other lanes of the wavefront read its diagonal only behind a fence
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const double dg = Dss[tel(li, li)];
            if (!f) f = __ffsll((unsigned long long)__ballot(!(dg > 0.0) || !(dg < INFINITY)));      // an infinite pivot
            if (f && lane == 0) flags[1] = 16 * s + f;
        }
        __syncthreads();
        if (flags[1]) return flags[1];
        if (tid < 256) ly.work[s * 256 + tid] = D0[tid];      // C_ss^-1 waits in `work` for the inversion
        for (int ti = s + 1 + wave; ti < nt; ti += NGS_WAVES) {      // C(ti, s) = A(ti, s) C_ss^-T
            double* A = Y + tix(ti, s);
            v4d d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) d = mfma(A[tel(li, 4 * k + lk)], D0[tel(li, 4 * k + lk)], d);
#pragma unroll
            for (int r = 0; r < 4; ++r) A[tel(4 * r + lk, li)] = d[r];
        }
        __syncthreads();
        const int n = nt - 1 - s;
        for (int e = wave; e < n * (n + 1) / 2; e += NGS_WAVES) {      // A(ti, tj) -= C(ti, s) C(tj, s)^T
            int a, b;
            ngs_tile_of(e, a, b);
            double* D = Y + tix(s + 1 + a, s + 1 + b);
            const double* P = Y + tix(s + 1 + a, s);
            const double* Q = Y + tix(s + 1 + b, s);
            v4d d;
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = D[tel(4 * r + lk, li)];
#pragma unroll
            for (int k = 0; k < 4; ++k) d = mfma(-P[tel(li, 4 * k + lk)], Q[tel(li, 4 * k + lk)], d);
#pragma unroll
            for (int r = 0; r < 4; ++r) D[tel(4 * r + lk, li)] = d[r];
        }
        __syncthreads();
    }
    // C^-1 in place, block row by block row: Inv(i, s) = -C_ii^-1 sum_{t = s}^{i-1} C(i, t) Inv(t, s), one wavefront per s < i
    for (int i = 0; i < nt; ++i) {
        if (tid < 256) D0[tid] = ly.work[i * 256 + tid];
        __syncthreads();
        const int s = wave;
        v4d d2 = {0.0, 0.0, 0.0, 0.0};
        if (s < i) {
            v4d d = {0.0, 0.0, 0.0, 0.0};
            for (int t = s; t < i; ++t) {
                const double* A = Y + tix(i, t);
                const double* B = Y + tix(t, s);
#pragma unroll
                for (int k = 0; k < 4; ++k) d = mfma(A[tel(li, 4 * k + lk)], B[tel(4 * k + lk, li)], d);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) d2 = mfma(D0[tel(li, 4 * k + lk)], d[k], d2);      // the accumulator is the B fragment
        }
        __syncthreads();
        if (s < i) {
            double* R = Y + tix(i, s);
#pragma unroll
            for (int r = 0; r < 4; ++r) R[tel(4 * r + lk, li)] = -d2[r];
        }
        if (tid < 256) Y[tix(i, i) + tid] = D0[tid];
        __syncthreads();
    }
    // L_new = L T, T[k][j] = C^-1[M-1-j][M-1-k] (k >= j, both < M): tile (ti, tj) = sum_{tk = tj}^{ti} L(ti, tk) T(tk, tj)
#pragma unroll
    for (int q = 0; q < NGS_TILE_SLOTS; ++q) {
        acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
        const int t = wave + NGS_WAVES * q;
        if (t < ntri) {
            int ti, tj;
            ngs_tile_of(t, ti, tj);
            const int j = 16 * tj + li;
            for (int tk = tj; tk <= ti; ++tk) {
                const double* A = X + tix(ti, tk);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int kk = 16 * tk + 4 * k + lk;
                    double b = 0.0;
                    if (kk < M && j <= kk) {
                        const int ri = M - 1 - j, ci = M - 1 - kk;
                        b = Y[tix(ri >> 4, ci >> 4) + tel(ri & 15, ci & 15)];
                    }
                    acc[q] = mfma(A[tel(li, 4 * k + lk)], b, acc[q]);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NGS_TILE_SLOTS; ++q) {
        const int t = wave + NGS_WAVES * q;
        if (t < ntri) {
#pragma unroll
            for (int r = 0; r < 4; ++r) X[t * 256 + tel(4 * r + lk, li)] = acc[q][r];
        }
    }
    __syncthreads();
    ngs_write_back(ly, gs, lds, [X](int i, int j) { return X[tix(i >> 4, j >> 4) + tel(i & 15, j & 15)]; });
    return 0;
}

__global__ __launch_bounds__(NGS_THREADS) void natgrad_small_kernel(const NgsLayer* layers, double gamma, double gamma_init,
                                                                    double log_ratio, int warmup) {
    extern __shared__ __attribute__((aligned(16))) double ngs_lds[];
    const NgsLayer ly = layers[blockIdx.x];
    int* flags = (int*)(ngs_lds + 1);
    int64_t* tword = (int64_t*)(ngs_lds + 2);
    if (threadIdx.x == 0) {
        // the guard: the producing step reported a failed Cholesky, an abandoned wait or a non-finite loss -> nothing of this
        // layer is written, the counter included
        int bad = 0;
        for (int k = 0; k < ly.n_guard_info; ++k) bad |= ly.guard_info[k] != 0;
        // (32 bits, as the ABI declares the status words: the launches only ever OR bits 0 and 1 into them, and on this
        // little-endian target the low half of InLaunchSync's int64 word is the word they write)
        if (ly.guard_status) bad |= ly.guard_status[0] != 0;
        if (ly.guard_loss) bad |= !isfinite(ly.guard_loss[0]);
        flags[0] = bad;
        flags[1] = 0;
        const int64_t t = ly.step_count[0];
        tword[0] = t;
        ngs_lds[0] = gamma_at(t, gamma, gamma_init, log_ratio, warmup) * ly.scale;
    }
    __syncthreads();
    if (flags[0]) return;
    const double gs = ngs_lds[0];
    const int fail = ly.M <= NGS_SMALL_M ? ngs_small(ly, gs, ngs_lds) : ngs_tiled(ly, gs, ngs_lds);
    if (threadIdx.x == 0) {
        ly.info[0] = fail;
        if (fail) ly.skipped[0] += 1;
        ly.step_count[0] = tword[0] + 1;
    }
}

bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }

}  // namespace

extern "C" {

int mobocmf_natgrad_small_work_bytes(int32_t M, size_t* bytes) {
    if (!bytes || M < 1 || M > NGS_MAX_M) return MOBOCMF_BAD_ARG;
    *bytes = M <= NGS_SMALL_M ? 0 : (size_t)((M + 15) / 16) * 256 * sizeof(double);
    return MOBOCMF_OK;
}

int mobocmf_natgrad_small_step(const mobocmf_natgrad_small_layer* host_layers, const mobocmf_natgrad_small_layer* dev_layers,
                               int32_t n_layers, double gamma, double gamma_init, int32_t warmup_steps,
                               mobocmf_stream_t stream) {
    if (!host_layers || !dev_layers || n_layers < 1) return MOBOCMF_BAD_ARG;
    if (!pos_finite(gamma) || !pos_finite(gamma_init) || !(gamma_init <= gamma) || warmup_steps < 0) return MOBOCMF_BAD_ARG;
    size_t lds = 0;
    for (int z = 0; z < n_layers; ++z) {
        const mobocmf_natgrad_small_layer& ly = host_layers[z];
        if (ly.M < 1 || ly.M > NGS_MAX_M || !ly.m || !ly.L_S || !ly.g_m || !ly.g_LS || !ly.step_count || !ly.skipped || !ly.info ||
            !pos_finite(ly.scale) || ly.n_guard_info < 0 || (ly.n_guard_info > 0 && !ly.guard_info) ||
            (ly.M > NGS_SMALL_M && !ly.work))
            return MOBOCMF_BAD_ARG;
        const size_t need = ngs_lds_bytes(ly.M);
        if (need > lds) lds = need;
    }
    if (lds > 64 * 1024)      // (a property of the loaded kernel, not of a call: setting it again is harmless)
        HIP_TRY(hipFuncSetAttribute((const void*)natgrad_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)ngs_lds_bytes(NGS_MAX_M)));
    hipLaunchKernelGGL(natgrad_small_kernel, dim3((unsigned)n_layers), dim3(NGS_THREADS), lds, (hipStream_t)stream, dev_layers,
                       gamma, gamma_init, log(gamma / gamma_init), (int)warmup_steps);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

}  // extern "C"
