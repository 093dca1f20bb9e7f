// Fitting the EXACT-GP baselines (models/mfgp.py: MFGP, MFGP_lin) on the device: the launches of one Adam step on the marginal
// likelihood that are not the factorisation's (include/mobocmf_hip.h, mobocmf_exact_fit_*; util/exact_fit.py drives them).
//
//   covariance  K = sig sig^T os_s E^s + ntab[min] os_n E^n + tau I from the CURRENT raw parameters, padded for
//               mobocmf_exact_gp_factor (zeros, identity on the padded diagonal)
//   prepare     L^-T (the operand of the triangular product that forms K^-1) and alpha = L^-T a
//   gradient    the <= 83 sums  sum_ij G_ij dK_ij / dtheta,  G = (alpha alpha^T - K^-1) / 2 formed on the fly; a workgroup owns
//               (model, strip of 16 rows) and STORES its partial sums into its row of the slab
//   update      sums the slab in strip order, then fit()'s loop body: stop on a non-finite loss, best iterate, chain rule to
//               the raw parameters, torch-default Adam through the pointer table; a second mode finishes (restore)
//
// Workgroups of different models share nothing, a strip's sums are reduced in a fixed order (wavefront shuffles, then LDS,
// then the slab): no atomics, no in-launch wait, two runs are bitwise equal.  The constrained values and the level tables are
// formed again by every workgroup that needs them (fit_values: a few dozen transcendental calls) -- rho moves every step.
#include "common.h"

namespace {

constexpr int FT = 256;                         // threads per workgroup, all kernels of this file
constexpr int FNW = FT / 64;
constexpr int FD = MOBOCMF_MAX_D;
constexpr int FL = MOBOCMF_EXACT_FIT_MAX_LEVELS;
constexpr int FS = MOBOCMF_EXACT_FIT_SUMS;      // 2 (d_max + 1) + 1 + 2 levels
constexpr int FRS = MOBOCMF_EXACT_FIT_STRIP;    // rows of a strip
constexpr int FCC = 64;                         // columns of a chunk of a strip
constexpr int FXS = FD + 1;                     // LDS stride of a row of inputs (odd: no bank conflicts across rows)
// positions in the slab / the sums (include/mobocmf_hip.h)
constexpr int S_OS_S = 0, S_LS_S = 1, S_OS_N = 1 + FD, S_LS_N = 2 + FD, S_TAU = 2 + 2 * FD, S_SIG = 3 + 2 * FD, S_NTAB = 3 + 2 * FD + FL;
static_assert(S_NTAB + FL == FS, "the slab's layout");
static_assert(FT == FRS * 16 && FCC == 64 && FT == 8 * FD, "thread maps of the gradient kernel");
static_assert(MOBOCMF_EXACT_FIT_MAX_N % FRS == 0 && MOBOCMF_EXACT_FIT_MAX_N % TILE == 0, "whole strips, whole tiles");

typedef mobocmf_exact_fit_model Model;
typedef mobocmf_exact_fit_param Param;

// ---- the work area of a model (doubles): K | LiT | Kinv (npad x npad each) | alpha (npad) | slab (strips x FS) | sums (FS)
struct Work { double *K, *LiT, *Kinv, *alpha, *slab, *sums; };
__host__ __device__ inline int npad_of(int n) { return (n + TILE - 1) / TILE * TILE; }
__host__ __device__ inline int strips_of(int n) { return (n + FRS - 1) / FRS; }
__host__ __device__ inline size_t work_doubles(int n) {
    const size_t np = (size_t)npad_of(n);
    return 3 * np * np + np + (size_t)strips_of(n) * FS + FS + 1;      // (one double to spare behind the sums)
}
__host__ __device__ inline Work carve(void* work, int n) {
    const size_t np = (size_t)npad_of(n);
    Work w;
    w.K = (double*)work;
    w.LiT = w.K + np * np;
    w.Kinv = w.LiT + np * np;
    w.alpha = w.Kinv + np * np;
    w.slab = w.alpha + np;
    w.sums = w.slab + (size_t)strips_of(n) * FS;
    return w;
}

// ---- constraints (gp.py): kind 0 the value itself, 1 lo + softplus(raw) (Positive, GreaterThan), 2 lo + (hi - lo) sigmoid(raw)
__device__ inline double fit_value(int kind, double raw, double lo, double hi) {
    if (kind == MOBOCMF_EXACT_FIT_SOFTPLUS) return lo + (raw > 20.0 ? raw : log1p(exp(raw)));      // torch's threshold
    if (kind == MOBOCMF_EXACT_FIT_SIGMOID) return lo + (hi - lo) * (1.0 / (1.0 + exp(-raw)));
    return raw;
}
__device__ inline double fit_slope(int kind, double raw, double lo, double hi) {
    if (kind == MOBOCMF_EXACT_FIT_SOFTPLUS) {
        if (raw > 20.0) return 1.0;
        const double z = exp(raw);
        return z / (z + 1.0);
    }
    if (kind == MOBOCMF_EXACT_FIT_SIGMOID) {
        const double s = 1.0 / (1.0 + exp(-raw));
        return (hi - lo) * s * (1.0 - s);
    }
    return 1.0;
}

struct Vals {
    double tau, os_s, os_n;
    double ls_s[FD], ls_n[FD];
    double sig[FL], ntab[FL], rho[FL];
};

// The constrained values and the level tables of a model from its raw parameters, into LDS (threads 0 .. 67 work; the caller
// synchronises).  sig[l] = prod_{q < l} rho_q, ntab[t] = [t >= 1] + sum_{k = 3}^{nf - 2} [t + 1 >= k] rho_{k-2}^2.
__device__ inline void fit_values(const Model& md, Vals* V, int tid) {
    const Param* P = md.params;
    if (tid < FD) {
        const Param& p = P[MOBOCMF_EXACT_FIT_P_LS_S];
        V->ls_s[tid] = tid < md.d ? fit_value(p.kind, p.raw[tid], p.lo, p.hi) : 1.0;
    } else if (tid < 2 * FD) {
        const int c = tid - FD;
        const Param& p = P[MOBOCMF_EXACT_FIT_P_LS_N];
        V->ls_n[c] = c < md.d ? fit_value(p.kind, p.raw[c], p.lo, p.hi) : 1.0;
    } else if (tid == 2 * FD) {
        const Param& p = P[MOBOCMF_EXACT_FIT_P_NOISE];
        V->tau = fit_value(p.kind, p.raw[0], p.lo, p.hi);
    } else if (tid == 2 * FD + 1) {
        const Param& p = P[MOBOCMF_EXACT_FIT_P_OS_S];
        V->os_s = fit_value(p.kind, p.raw[0], p.lo, p.hi);
    } else if (tid == 2 * FD + 2) {
        const Param& p = P[MOBOCMF_EXACT_FIT_P_OS_N];
        V->os_n = fit_value(p.kind, p.raw[0], p.lo, p.hi);
    } else if (tid == 2 * FD + 3) {
        const int nl = md.n_levels;
        if (md.kernel == MOBOCMF_EXACT_FIT_KERNEL_LIN) {
            const Param& p = P[MOBOCMF_EXACT_FIT_P_RHO];
            double run = 1.0;
            for (int l = 0; l < FL; ++l) {
                V->sig[l] = l < nl ? run : 0.0;
                const double r = l < nl - 1 ? fit_value(p.kind, p.raw[l], p.lo, p.hi) : 0.0;
                V->rho[l] = r;
                run *= r;
            }
            for (int t = 0; t < FL; ++t) {
                double v = t >= 1 ? 1.0 : 0.0;
                for (int k = 3; k <= nl - 2; ++k)
                    if (t + 1 >= k) v += V->rho[k - 2] * V->rho[k - 2];
                V->ntab[t] = t < nl ? v : 0.0;
            }
        } else {
            for (int l = 0; l < FL; ++l) {
                V->sig[l] = l < nl ? 1.0 : 0.0;
                V->ntab[l] = l < nl ? (double)l : 0.0;
                V->rho[l] = 0.0;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ covariance
// A workgroup owns a 16 x 16 tile of the npad x npad matrix of one model.
__global__ __launch_bounds__(FT) void exact_fit_cov_kernel(const Model* models) {
    __shared__ Vals V;
    __shared__ double xi[16 * FXS], xj[16 * FXS];
    __shared__ int li[16], lj[16];
    const Model& md = models[blockIdx.y];
    const int tid = threadIdx.x, n = md.n, d = md.d, nl = md.n_levels, np = npad_of(n), tiles = np / 16;
    if ((int)blockIdx.x >= tiles * tiles) return;      // (the grid is sized for the largest model)
    const int ti = blockIdx.x / tiles, tj = blockIdx.x % tiles;
    fit_values(md, &V, tid);
    for (int e = tid; e < 2 * 16 * FD; e += FT) {
        const int side = e / (16 * FD), r = (e / FD) % 16, c = e % FD;
        const int row = (side ? tj : ti) * 16 + r;
        (side ? xj : xi)[r * FXS + c] = (row < n && c < d) ? md.x[(int64_t)row * d + c] : 0.0;
    }
    if (tid < 32) {
        const int row = (tid < 16 ? ti : tj) * 16 + (tid & 15);
        (tid < 16 ? li : lj)[tid & 15] = row < n ? md.lev[row] : 0;
    }
    __syncthreads();
    const int r = tid >> 4, c = tid & 15, i = ti * 16 + r, j = tj * 16 + c;
    double v = i == j ? 1.0 : 0.0;      // the padding: identity on the diagonal
    if (i < n && j < n) {
        const int a = li[r], b = lj[c];
        if (a < 0 || a >= nl || b < 0 || b >= nl) {
            v = __builtin_nan("");      // a level outside the tables is never an index
        } else {
            double qs = 0.0, qn = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = xi[r * FXS + k] - xj[c * FXS + k];
                const double us = df / V.ls_s[k], un = df / V.ls_n[k];
                qs += us * us;
                qn += un * un;
            }
            v = V.sig[a] * V.sig[b] * V.os_s * exp(-0.5 * qs) + V.ntab[a < b ? a : b] * V.os_n * exp(-0.5 * qn);
            if (i == j) v += V.tau;
        }
    }
    carve(md.work, n).K[(int64_t)i * np + j] = v;
}

// --------------------------------------------------------------------------------------------------------------- prepare
// Blocks [0, tt): a 32 x 32 tile of LiT = (L^-1)^T over the whole padded matrix; blocks [tt_grid, ...): four rows of
// alpha = L^-T a, a wavefront each, summed over k = i .. n - 1 with the lanes strided and a shuffle tree.
__global__ __launch_bounds__(FT) void exact_fit_prepare_kernel(const Model* models, int tt_grid) {
    __shared__ double tile[32][33];
    const Model& md = models[blockIdx.y];
    const int tid = threadIdx.x, n = md.n, np = npad_of(n), tiles = np / 32;
    const Work w = carve(md.work, n);
    if ((int)blockIdx.x < tt_grid) {
        if ((int)blockIdx.x >= tiles * tiles) return;
        const int ti = blockIdx.x / tiles, tj = blockIdx.x % tiles, c = tid & 31, r0 = tid >> 5;
        for (int r = r0; r < 32; r += 8) tile[r][c] = md.Linv[(int64_t)(ti * 32 + r) * np + tj * 32 + c];
        __syncthreads();
        for (int r = r0; r < 32; r += 8) w.LiT[(int64_t)(tj * 32 + r) * np + ti * 32 + c] = tile[c][r];
        return;
    }
    const int i = ((int)blockIdx.x - tt_grid) * FNW + (tid >> 6), lane = tid & 63;
    if (i >= np) return;
    double s = 0.0;
    if (i < n)
        for (int k = i + lane; k < n; k += 64) s += md.Linv[(int64_t)k * np + i] * md.a[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) w.alpha[i] = s;
}

// -------------------------------------------------------------------------------------------------------------- gradient
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// A workgroup owns (model, strip of FRS rows) and walks the columns in chunks of FCC.  Per chunk, phase A: thread (row, column
// lane) forms its four elements' weights  Ws = G sig_i sig_j E^s,  Wn = G ntab[min] E^n  into LDS and keeps the scalar sums;
// phase B: thread (coordinate c, eighth of the chunk) sums Ws (x_ic - x_jc)^2 and Wn (x_ic - x_jc)^2 over its elements.
__global__ __launch_bounds__(FT) void exact_fit_grad_kernel(const Model* models) {
    __shared__ Vals V;
    __shared__ double xs[FRS * FXS], xc[FCC * FXS];
    __shared__ double Ws[FRS * FCC], Wn[FRS * FCC];
    __shared__ double red[FNW][3 + FL], rowsum[FRS], lsred[8][2][FD];
    __shared__ int levs[FRS], levc[FCC];
    const Model& md = models[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = md.n, d = md.d, nl = md.n_levels, np = npad_of(n);
    const int r0 = blockIdx.x * FRS;
    if (r0 >= n) return;      // (the grid is sized for the largest model)
    const Work w = carve(md.work, n);
    fit_values(md, &V, tid);
    for (int e = tid; e < FRS * FD; e += FT) {
        const int r = e / FD, c = e % FD;
        xs[r * FXS + c] = (r0 + r < n && c < d) ? md.x[(int64_t)(r0 + r) * d + c] : 0.0;
    }
    if (tid < FRS) levs[tid] = r0 + tid < n ? md.lev[r0 + tid] : 0;
    __syncthreads();

    const int row = tid >> 4, cl = tid & 15, i = r0 + row;      // phase A
    const int pc = tid & (FD - 1), part = tid / FD;             // phase B
    const int li = levs[row];
    const bool row_ok = i < n, li_ok = li >= 0 && li < nl;
    const double ai = row_ok ? w.alpha[i] : 0.0;
    const double sgi = li_ok ? V.sig[li] : 0.0;
    double a_os_s = 0.0, a_os_n = 0.0, a_tau = 0.0, a_row = 0.0, a_nt[FL], a_ls_s = 0.0, a_ls_n = 0.0;
#pragma unroll
    for (int t = 0; t < FL; ++t) a_nt[t] = 0.0;

#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += FCC) {
        for (int e = tid; e < FCC * FD; e += FT) {
            const int r = e / FD, c = e % FD;
            xc[r * FXS + c] = (c0 + r < n && c < d) ? md.x[(int64_t)(c0 + r) * d + c] : 0.0;
        }
        if (tid < FCC) levc[tid] = c0 + tid < n ? md.lev[c0 + tid] : 0;
        __syncthreads();
#pragma unroll 1
        for (int q = 0; q < FCC / 16; ++q) {
            const int jl = cl + 16 * q, j = c0 + jl;
            double ws = 0.0, wn = 0.0;
            if (row_ok && j < n) {
                const int lj = levc[jl];
                if (!li_ok || lj < 0 || lj >= nl) {
                    ws = wn = __builtin_nan("");
                    a_os_s += ws;      // (every sum of the strip becomes NaN, as the covariance did)
                    a_tau += ws;
                } else {
                    double qs = 0.0, qn = 0.0;
                    for (int k = 0; k < d; ++k) {
                        const double df = xs[row * FXS + k] - xc[jl * FXS + k];
                        const double us = df / V.ls_s[k], un = df / V.ls_n[k];
                        qs += us * us;
                        qn += un * un;
                    }
                    const double G = 0.5 * (ai * w.alpha[j] - w.Kinv[(int64_t)i * np + j]);
                    const double Es = exp(-0.5 * qs), En = exp(-0.5 * qn);
                    const int m = li < lj ? li : lj;
                    const double gr = G * V.sig[lj] * Es;      // row i's share of d / dsig[l_i] (x 2 os_s at the end)
                    ws = gr * sgi;
                    const double ge = G * En;
                    wn = ge * V.ntab[m];
                    a_os_s += ws;
                    a_os_n += wn;
                    a_row += gr;
                    if (i == j) a_tau += G;
#pragma unroll
                    for (int t = 0; t < FL; ++t) a_nt[t] += t == m ? ge : 0.0;
                }
            }
            Ws[row * FCC + jl] = ws;
            Wn[row * FCC + jl] = wn;
        }
        __syncthreads();
        if (pc < d) {
            constexpr int per = FRS * FCC / 8;
#pragma unroll 4
            for (int e = part * per; e < (part + 1) * per; ++e) {
                const double df = xs[(e / FCC) * FXS + pc] - xc[(e % FCC) * FXS + pc];
                const double df2 = df * df;
                a_ls_s += Ws[e] * df2;
                a_ls_n += Wn[e] * df2;
            }
        }
        __syncthreads();
    }

    // the strip's sums: shuffles within a wavefront, then LDS in wavefront order
    {
        const double r_os_s = wave_sum(a_os_s), r_os_n = wave_sum(a_os_n), r_tau = wave_sum(a_tau);
        if (lane == 0) {
            red[wave][0] = r_os_s;
            red[wave][1] = r_os_n;
            red[wave][2] = r_tau;
        }
#pragma unroll
        for (int t = 0; t < FL; ++t) {
            const double r = wave_sum(a_nt[t]);
            if (lane == 0) red[wave][3 + t] = r;
        }
        double rr = a_row;      // the 16 lanes of a row
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) rr += __shfl_xor(rr, m);
        if (cl == 0) rowsum[row] = rr;
        lsred[part][0][pc] = a_ls_s;
        lsred[part][1][pc] = a_ls_n;
    }
    __syncthreads();
    double* out = w.slab + (size_t)blockIdx.x * FS;
    if (tid < FS) {
        double v = 0.0;
        if (tid == S_OS_S || tid == S_OS_N || tid == S_TAU) {
            const int k = tid == S_OS_S ? 0 : tid == S_OS_N ? 1 : 2;
            for (int p = 0; p < FNW; ++p) v += red[p][k];
        } else if (tid >= S_NTAB) {
            const int t = tid - S_NTAB;
            for (int p = 0; p < FNW; ++p) v += red[p][3 + t];
            v *= V.os_n;
        } else if (tid >= S_SIG) {
            const int l = tid - S_SIG;
            for (int r = 0; r < FRS; ++r)
                if (r0 + r < n && levs[r] == l) v += rowsum[r];
            v *= 2.0 * V.os_s;
        } else {
            const bool noise = tid >= S_LS_N;
            const int c = tid - (noise ? S_LS_N : S_LS_S);
            if (c < d) {
                for (int p = 0; p < 8; ++p) v += lsred[p][noise ? 1 : 0][c];
                const double ls = noise ? V.ls_n[c] : V.ls_s[c];
                v = v * (noise ? V.os_n : V.os_s) / (ls * ls * ls);
            }
        }
        out[tid] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- update
// One workgroup per model.  Thread 0 takes fit()'s decisions; the others follow them through LDS.
__global__ __launch_bounds__(FT) void exact_fit_update_kernel(const Model* models, int mode, double lr, double b1, double b2, double eps) {
    __shared__ Vals V;
    __shared__ double D[FS], drho[FL];
    __shared__ int act[3];      // 0: go on (1) or leave (0); 1: new best; 2: the iteration
    const Model& md = models[blockIdx.x];
    const int tid = threadIdx.x, n = md.n, d = md.d, nl = md.n_levels;
    const Work w = carve(md.work, n);
    const Param* P = md.params;
    int32_t* words = md.words;

    if (mode == MOBOCMF_EXACT_FIT_FINISH) {
        if (tid == 0) {
            const double loss = -md.mll[0];
            const int info = md.info[0];
            md.stats[1] = loss;
            words[MOBOCMF_EXACT_FIT_W_FINAL_INFO] = info;
            if (info < 0) words[MOBOCMF_EXACT_FIT_W_ABANDONED] = 1;
            const bool back = words[MOBOCMF_EXACT_FIT_W_BEST_IT] >= 0 && (!isfinite(loss) || info != 0 || loss > md.stats[0]);
            if (back) words[MOBOCMF_EXACT_FIT_W_RESTORED] = 1;
            act[0] = back ? 1 : 0;
        }
        __syncthreads();
        if (!act[0]) return;
        for (int k = 0; k < MOBOCMF_EXACT_FIT_PARAMS; ++k)
            for (int e = tid; e < P[k].numel; e += FT) P[k].raw[e] = P[k].best[e];
        return;
    }

    // 1. the slab, strip by strip
    if (tid < FS) {
        double v = 0.0;
        const int ns = strips_of(n);
        for (int s = 0; s < ns; ++s) v += w.slab[(size_t)s * FS + tid];
        D[tid] = v;
        w.sums[tid] = v;
    }
    // 2. - 6. (thread 0)
    if (tid == 0) {
        const int it = words[MOBOCMF_EXACT_FIT_W_IT];
        int go = 0, best = 0;
        if (words[MOBOCMF_EXACT_FIT_W_STOPPED_AT] < 0) {
            const double loss = -md.mll[0];
            const int info = md.info[0];
            if (!isfinite(loss) || info != 0) {
                words[MOBOCMF_EXACT_FIT_W_STOPPED_AT] = it;
                if (it < md.cap) md.losses[it] = __builtin_nan("");
                if (info < 0) words[MOBOCMF_EXACT_FIT_W_ABANDONED] = 1;
            } else {
                go = 1;
                if (it < md.cap) md.losses[it] = loss;
                if (words[MOBOCMF_EXACT_FIT_W_BEST_IT] < 0 || loss < md.stats[0]) {
                    best = 1;
                    md.stats[0] = loss;
                    words[MOBOCMF_EXACT_FIT_W_BEST_IT] = it;
                }
            }
        }
        act[0] = go;
        act[1] = best;
        act[2] = it;
    }
    fit_values(md, &V, tid);
    __syncthreads();
    if (!act[0]) return;
    if (act[1])
        for (int k = 0; k < MOBOCMF_EXACT_FIT_PARAMS; ++k)
            for (int e = tid; e < P[k].numel; e += FT) P[k].best[e] = P[k].raw[e];
    // 7. the chain rule: d mll / d rho through sig (prefix and running products, no division) and ntab
    if (tid < FL) {
        double g = 0.0;
        const int q = tid;
        if (md.kernel == MOBOCMF_EXACT_FIT_KERNEL_LIN && q < nl - 1) {
            double run = 1.0;
            for (int p = 0; p < q; ++p) run *= V.rho[p];      // prod_{p < q} rho_p: d sig[q + 1] / d rho_q
            for (int l = q + 1; l < nl; ++l) {
                g += D[S_SIG + l] * run;
                run *= V.rho[l];
            }
            const int k = q + 2;                               // ntab holds rho_{k-2}^2 for k = 3 .. nf - 2
            if (k >= 3 && k <= nl - 2)
                for (int t = k - 1; t < nl; ++t) g += D[S_NTAB + t] * 2.0 * V.rho[q];
        }
        drho[q] = g;
    }
    __syncthreads();
    {
        // thread -> (parameter, element): five scalars and vectors of at most FD elements
        int k = -1, e = 0;
        double dv = 0.0;
        if (tid < FD) { k = MOBOCMF_EXACT_FIT_P_LS_S; e = tid; dv = D[S_LS_S + (e < FD ? e : 0)]; }
        else if (tid < 2 * FD) { k = MOBOCMF_EXACT_FIT_P_LS_N; e = tid - FD; dv = D[S_LS_N + e]; }
        else if (tid == 2 * FD) { k = MOBOCMF_EXACT_FIT_P_NOISE; dv = D[S_TAU]; }
        else if (tid == 2 * FD + 1) { k = MOBOCMF_EXACT_FIT_P_OS_S; dv = D[S_OS_S]; }
        else if (tid == 2 * FD + 2) { k = MOBOCMF_EXACT_FIT_P_OS_N; dv = D[S_OS_N]; }
        else if (tid < 2 * FD + 3 + FL) { k = MOBOCMF_EXACT_FIT_P_RHO; e = tid - (2 * FD + 3); dv = drho[e]; }
        if (k >= 0 && e < P[k].numel) {
            const Param& p = P[k];
            const double raw = p.raw[e];
            const double gi = -dv * fit_slope(p.kind, raw, p.lo, p.hi);      // the loss is -mll
            p.grad[e] = gi;
            // torch.optim.Adam (mobocmf_adam_multi's expressions)
            const double step = (double)(act[2] + 1);
            const double bc1 = 1.0 - pow(b1, step), bc2s = sqrt(1.0 - pow(b2, step));
            const double mi = b1 * p.exp_avg[e] + (1.0 - b1) * gi;
            const double vi = b2 * p.exp_avg_sq[e] + (1.0 - b2) * gi * gi;
            p.exp_avg[e] = mi;
            p.exp_avg_sq[e] = vi;
            p.raw[e] = raw - (lr / bc1) * mi / (sqrt(vi) / bc2s + eps);
        }
    }
    // 8.
    if (tid == 0) words[MOBOCMF_EXACT_FIT_W_IT] = act[2] + 1;
}

bool sizes_ok(const Model* m) {
    return m && m->n >= 1 && m->n <= MOBOCMF_EXACT_FIT_MAX_N && m->d >= 1 && m->d <= MOBOCMF_MAX_D && m->n_levels >= 1 &&
           m->n_levels <= MOBOCMF_EXACT_FIT_MAX_LEVELS &&
           (m->kernel == MOBOCMF_EXACT_FIT_KERNEL_MIN || m->kernel == MOBOCMF_EXACT_FIT_KERNEL_LIN);
}

// every pointer a launch may read or write, and the lengths of the parameter tensors
bool model_ok(const Model& m) {
    if (!sizes_ok(&m) || !m.x || !m.lev || !m.y || !m.Linv || !m.a || !m.mll || !m.info || !m.work || !m.losses || !m.stats ||
        !m.words || m.cap < 1)
        return false;
    for (int k = 0; k < MOBOCMF_EXACT_FIT_PARAMS; ++k) {
        const Param& p = m.params[k];
        int want = 1;
        if (k == MOBOCMF_EXACT_FIT_P_LS_S || k == MOBOCMF_EXACT_FIT_P_LS_N) want = m.d;
        if (k == MOBOCMF_EXACT_FIT_P_RHO) want = m.kernel == MOBOCMF_EXACT_FIT_KERNEL_LIN ? m.n_levels - 1 : 0;
        if (p.numel != want) return false;
        if (want == 0) continue;
        if (!p.raw || !p.best || !p.exp_avg || !p.exp_avg_sq || !p.grad) return false;
        if (p.kind != MOBOCMF_EXACT_FIT_IDENTITY && p.kind != MOBOCMF_EXACT_FIT_SOFTPLUS && p.kind != MOBOCMF_EXACT_FIT_SIGMOID)
            return false;
    }
    return true;
}

int check_table(const Model* host_models, const Model* dev_models, int32_t n_models, int* nmax) {
    if (!host_models || !dev_models || n_models < 1 || n_models > MOBOCMF_EXACT_FIT_MAX_MODELS) return MOBOCMF_BAD_ARG;
    *nmax = 0;
    for (int i = 0; i < n_models; ++i) {
        if (!model_ok(host_models[i])) return MOBOCMF_BAD_ARG;
        if (host_models[i].n > *nmax) *nmax = host_models[i].n;
    }
    return MOBOCMF_OK;
}

inline int launched() { return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR; }

}  // namespace

extern "C" {

int mobocmf_exact_fit_work_bytes(const mobocmf_exact_fit_model* model, int32_t n_models, size_t* bytes) {
    if (!bytes || !sizes_ok(model) || n_models < 1 || n_models > MOBOCMF_EXACT_FIT_MAX_MODELS) return MOBOCMF_BAD_ARG;
    *bytes = work_doubles(model->n) * sizeof(double);
    return MOBOCMF_OK;
}

int mobocmf_exact_fit_covariance(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                                 int32_t n_models, mobocmf_stream_t stream) {
    int nmax = 0;
    const int rc = check_table(host_models, dev_models, n_models, &nmax);
    if (rc != MOBOCMF_OK) return rc;
    const int tiles = npad_of(nmax) / 16;
    hipLaunchKernelGGL(exact_fit_cov_kernel, dim3((unsigned)(tiles * tiles), (unsigned)n_models), dim3(FT), 0, (hipStream_t)stream,
                       dev_models);
    return launched();
}

int mobocmf_exact_fit_prepare(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                              int32_t n_models, mobocmf_stream_t stream) {
    int nmax = 0;
    const int rc = check_table(host_models, dev_models, n_models, &nmax);
    if (rc != MOBOCMF_OK) return rc;
    const int np = npad_of(nmax), tt = (np / 32) * (np / 32);
    hipLaunchKernelGGL(exact_fit_prepare_kernel, dim3((unsigned)(tt + np / FNW), (unsigned)n_models), dim3(FT), 0,
                       (hipStream_t)stream, dev_models, tt);
    return launched();
}

int mobocmf_exact_fit_gradient(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                               int32_t n_models, mobocmf_stream_t stream) {
    int nmax = 0;
    const int rc = check_table(host_models, dev_models, n_models, &nmax);
    if (rc != MOBOCMF_OK) return rc;
    hipLaunchKernelGGL(exact_fit_grad_kernel, dim3((unsigned)strips_of(nmax), (unsigned)n_models), dim3(FT), 0, (hipStream_t)stream,
                       dev_models);
    return launched();
}

int mobocmf_exact_fit_update(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                             int32_t n_models, int32_t mode, double lr, double beta1, double beta2, double eps,
                             mobocmf_stream_t stream) {
    int nmax = 0;
    const int rc = check_table(host_models, dev_models, n_models, &nmax);
    if (rc != MOBOCMF_OK) return rc;
    if (mode != MOBOCMF_EXACT_FIT_STEP && mode != MOBOCMF_EXACT_FIT_FINISH) return MOBOCMF_BAD_ARG;
    hipLaunchKernelGGL(exact_fit_update_kernel, dim3((unsigned)n_models), dim3(FT), 0, (hipStream_t)stream, dev_models, (int)mode, lr,
                       beta1, beta2, eps);
    return launched();
}

}  // extern "C"
