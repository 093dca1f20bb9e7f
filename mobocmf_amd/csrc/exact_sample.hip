// Posterior FUNCTION samples of the exact-GP baselines (models/mfgp.py: MFGP, MFGP_lin) by Matheron's rule in the n-dimensional
// function space, for several (model, sample) problems of different n at once (include/mobocmf_hip.h, mobocmf_exact_sample_*;
// util/exact_sample.py drives them).  With C_sig = cos(W_sig x + b_sig), C_noi = cos(W_noi x + b_noi) (F x n each):
//
//   gram     G = s_i s_j c_sig^2 (C_sig^T C_sig)_ij + ntab[min(l_i, l_j)] c_noi^2 (C_noi^T C_noi)_ij + noise [i == j], padded for
//            mobocmf_exact_gp_factor (zeros, identity on the padded diagonal), and r = y - Phi^T theta0 - e.  A workgroup owns a
//            64 x 64 tile on or below the diagonal and mirrors it; the cosines of a chunk of 16 features are formed in LDS and
//            both n x n x F products run on v_mfma_f64_16x16x4_f64 from there: Phi never reaches memory
//   solve    w = L^-T a from the factorisation's state (a wavefront per row), and the factorisation's info word
//   weights  theta = theta0 + Phi w, and per requested output level the folded one-layer sample (W1 = [W_sig; W_noi], b1,
//            theta' = [s(f) c_sig theta_sig ; c_noi sum_{l <= f} sqrt(delta_l) theta_noi,l]) into a packed RFFChainSample
//
// The kernels draw nothing: every random number is an operand.  Sums run in a fixed order (the matrix instruction's, wavefront
// shuffles, LDS in part order): no atomics, no in-launch wait, two runs are bitwise equal.
#include "common.h"
#include "tile16.h"

namespace {

constexpr int ST = 256;                               // threads per workgroup, all kernels of this file
constexpr int SFC = MOBOCMF_EXACT_SAMPLE_CHUNK;       // features of a chunk
constexpr int SB = 64;                                // rows / columns of a tile of G
constexpr int SCS = 80;                               // LDS stride of a feature's 64 cosines
constexpr int SL = MOBOCMF_EXACT_SAMPLE_MAX_LEVELS;
constexpr int SD = MOBOCMF_MAX_D;
constexpr int SWS = SD + 1;                           // LDS stride of a feature's frequencies
constexpr int SHEAD = 13;                             // packed one-layer chain sample: 5 + 1 header, 7 layer scalars
static_assert(SFC == 16 && ST == 4 * SB && TILE % SB == 0, "thread maps of the gram kernel");
static_assert(4 * SB * (1 + SL) <= 2 * SFC * SCS, "the r partial sums reuse the first two cosine panels");

typedef mobocmf_exact_sample_problem Problem;

__host__ __device__ inline int npad_of(int n) { return (n + TILE - 1) / TILE * TILE; }
__host__ __device__ inline int64_t packed_len(int d, int F) { return SHEAD + (int64_t)2 * F * (d + 2); }

// ------------------------------------------------------------------------------------------------------------------ gram
__global__ __launch_bounds__(ST) void exact_sample_gram_kernel(const Problem* probs) {
    __shared__ double C[4 * SFC * SCS];               // panels: 0 rows / signal, 1 columns / signal, 2 rows / noise, 3 columns / noise
    __shared__ double Wl[2][SFC * SWS], bl[2][SFC];
    __shared__ double th[(1 + SL) * SFC];
    __shared__ double tab[3][SL];                     // sig, ntab, sqrt(delta)
    __shared__ int levs[2][SB];
    const Problem& pb = probs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int n = pb.n, d = pb.d, nl = pb.n_levels, F = pb.F, np = npad_of(n), tiles = np / SB;
    if ((int)blockIdx.x >= tiles * (tiles + 1) / 2) return;      // (the grid is sized for the largest problem)
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const bool want_r = tj == 0;

    if (tid < 2 * SB) {
        const int side = tid >> 6, row = (side ? tj : ti) * SB + (tid & 63);
        levs[side][tid & 63] = row < n ? pb.lev[row] : 0;
    }
    if (tid < 3 * SL) {
        const int which = tid / SL, l = tid % SL;
        const double* src = which == 0 ? pb.sig : which == 1 ? pb.ntab : pb.sqd;
        tab[which][l] = l < nl ? src[l] : 0.0;
    }
    const double csq_s = 2.0 * pb.scal[0] / (double)F, csq_n = 2.0 * pb.scal[1] / (double)F, noise = pb.scal[2];

    // feature phase: thread -> (side, row of the tile, half of the chunk); r phase: thread -> (row, quarter of the chunk)
    const int fside = (tid & 127) >> 6, frow = tid & 63, fh = tid >> 7;
    const int grow = (fside ? tj : ti) * SB + frow;
    const bool grow_ok = grow < n;
    const double* xrow = pb.x + (int64_t)(grow_ok ? grow : 0) * d;
    const int rrow = tid & 63, rpart = tid >> 6;
    v4d acc_s[4], acc_n[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc_s[cb] = acc_n[cb] = v4d{0.0, 0.0, 0.0, 0.0};
    double rs = 0.0, rn[SL];
#pragma unroll
    for (int l = 0; l < SL; ++l) rn[l] = 0.0;

#pragma unroll 1
    for (int f0 = 0; f0 < F; f0 += SFC) {
        for (int e = tid; e < 2 * SFC * d; e += ST) {
            const int kind = e / (SFC * d), fl = (e / d) % SFC, k = e % d, f = f0 + fl;
            Wl[kind][fl * SWS + k] = f < F ? (kind ? pb.W_noi : pb.W_sig)[(int64_t)f * d + k] : 0.0;
        }
        if (tid < 2 * SFC) {
            const int kind = tid / SFC, f = f0 + tid % SFC;
            bl[kind][tid % SFC] = f < F ? (kind ? pb.b_noi : pb.b_sig)[f] : 0.0;
        }
        if (want_r)
            for (int e = tid; e < (1 + SL) * SFC; e += ST) {
                const int blk = e / SFC, f = f0 + e % SFC;
                th[e] = (blk <= nl && f < F) ? pb.theta0[(int64_t)blk * F + f] : 0.0;
            }
        __syncthreads();
        {
            double as[8], an[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                as[q] = bl[0][fh * 8 + q];
                an[q] = bl[1][fh * 8 + q];
            }
            for (int k = 0; k < d; ++k) {
                const double xv = xrow[k];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    as[q] = __builtin_fma(Wl[0][(fh * 8 + q) * SWS + k], xv, as[q]);
                    an[q] = __builtin_fma(Wl[1][(fh * 8 + q) * SWS + k], xv, an[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int fl = fh * 8 + q;
                const bool on = grow_ok && f0 + fl < F;
                C[(fside)*SFC * SCS + fl * SCS + frow] = on ? cos(as[q]) : 0.0;
                C[(2 + fside) * SFC * SCS + fl * SCS + frow] = on ? cos(an[q]) : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < SFC / 4; ++ks) {
            const int kf = (4 * ks + lk) * SCS;
            const double a_s = C[kf + 16 * wave + li], a_n = C[2 * SFC * SCS + kf + 16 * wave + li];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                acc_s[cb] = mfma(a_s, C[SFC * SCS + kf + 16 * cb + li], acc_s[cb]);
                acc_n[cb] = mfma(a_n, C[3 * SFC * SCS + kf + 16 * cb + li], acc_n[cb]);
            }
        }
        if (want_r) {
#pragma unroll
            for (int q = 0; q < SFC / 4; ++q) {
                const int fl = rpart + 4 * q;
                const double cs = C[fl * SCS + rrow], cn = C[2 * SFC * SCS + fl * SCS + rrow];
                rs = __builtin_fma(cs, th[fl], rs);
#pragma unroll
                for (int l = 0; l < SL; ++l) rn[l] = __builtin_fma(cn, th[(1 + l) * SFC + fl], rn[l]);
            }
        }
        __syncthreads();
    }

    // the tile: the level and scale combination, the noise, the padding; mirrored above the diagonal
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 16 * wave + lk + 4 * q, col = 16 * cb + li;
            const int i = ti * SB + row, j = tj * SB + col;
            double v = i == j ? 1.0 : 0.0;      // the padding: identity on the diagonal
            if (i < n && j < n) {
                const int a = levs[0][row], b = levs[1][col];
                if (a < 0 || a >= nl || b < 0 || b >= nl) {
                    v = __builtin_nan("");      // a level outside the tables is never an index
                } else {
                    v = tab[0][a] * tab[0][b] * csq_s * acc_s[cb][q] + tab[1][a < b ? a : b] * csq_n * acc_n[cb][q];
                    if (i == j) v += noise;
                }
            }
            pb.G[(int64_t)i * np + j] = v;
            if (ti != tj) pb.G[(int64_t)j * np + i] = v;
        }
    }

    if (!want_r) return;
    double* red = C;      // [part][row][1 + SL]; the loop's last barrier is behind every read of the panels
    red[(rpart * SB + rrow) * (1 + SL)] = rs;
#pragma unroll
    for (int l = 0; l < SL; ++l) red[(rpart * SB + rrow) * (1 + SL) + 1 + l] = rn[l];
    __syncthreads();
    if (tid < SB) {
        const int i = ti * SB + tid;
        if (i < n) {
            const int a = levs[0][tid];
            double v = __builtin_nan("");
            if (a >= 0 && a < nl) {
                double ps = 0.0;
                for (int p = 0; p < 4; ++p) ps += red[(p * SB + tid) * (1 + SL)];
                double pn = 0.0;
                for (int l = 0; l < SL; ++l) {
                    if (l > a) break;
                    double t = 0.0;
                    for (int p = 0; p < 4; ++p) t += red[(p * SB + tid) * (1 + SL) + 1 + l];
                    pn += tab[2][l] * t;
                }
                v = pb.y[i] - (tab[0][a] * sqrt(csq_s) * ps + sqrt(csq_n) * pn) - pb.e[i];
            }
            pb.r[i] = v;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- solve
// Four rows of w = L^-T a per workgroup, a wavefront each, summed over k = i .. n - 1 with the lanes strided and a shuffle tree.
__global__ __launch_bounds__(ST) void exact_sample_solve_kernel(const Problem* probs) {
    const Problem& pb = probs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, n = pb.n, np = npad_of(n);
    if (blockIdx.x == 0 && tid == 0) pb.info_out[0] = pb.info[0];
    const int i = (int)blockIdx.x * (ST / 64) + (tid >> 6);
    if (i >= n) return;
    double s = 0.0;
    for (int k = i + lane; k < n; k += 64) s += pb.Linv[(int64_t)k * np + i] * pb.a[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) pb.w[i] = s;
}

// --------------------------------------------------------------------------------------------------------------- weights
// A workgroup owns (problem, 16 features): thread (feature, row lane) sums its rows i = lane, lane + 16, ..., the 16 lanes of a
// feature are reduced by shuffles.
__global__ __launch_bounds__(ST) void exact_sample_weights_kernel(const Problem* probs) {
    __shared__ double tab[2][SL];                     // sig, sqrt(delta)
    const Problem& pb = probs[blockIdx.y];
    const int tid = threadIdx.x, fl = tid >> 4, rl = tid & 15;
    const int n = pb.n, d = pb.d, nl = pb.n_levels, F = pb.F, n_out = pb.n_out;
    const int fbase = (int)blockIdx.x * SFC;
    if (fbase >= F) return;                           // (the grid is sized for the largest problem)
    if (tid < 2 * SL) {
        const int which = tid / SL, l = tid % SL;
        tab[which][l] = l < nl ? (which ? pb.sqd : pb.sig)[l] : 0.0;
    }
    __syncthreads();
    const int f = fbase + fl;
    const bool valid = f < F;
    const double c_s = sqrt(2.0 * pb.scal[0] / (double)F), c_n = sqrt(2.0 * pb.scal[1] / (double)F);
    const int64_t plen = packed_len(d, F), o_w = SHEAD, o_b = SHEAD + (int64_t)2 * F * d, o_t = o_b + 2 * F;

    double acc_s = 0.0, acc_n[SL];
#pragma unroll
    for (int l = 0; l < SL; ++l) acc_n[l] = 0.0;
    if (valid) {
        const double* ws = pb.W_sig + (int64_t)f * d;
        const double* wn = pb.W_noi + (int64_t)f * d;
        const double bs = pb.b_sig[f], bn = pb.b_noi[f];
        for (int i = rl; i < n; i += 16) {
            const double* xr = pb.x + (int64_t)i * d;
            double as = bs, an = bn;
            for (int k = 0; k < d; ++k) {
                const double xv = xr[k];
                as = __builtin_fma(ws[k], xv, as);
                an = __builtin_fma(wn[k], xv, an);
            }
            const int a = pb.lev[i];
            const double wi = pb.w[i];
            if (a < 0 || a >= nl) {
                acc_s = __builtin_nan("");
            } else {
                const double ps = wi * cos(as), pn = wi * cos(an);
                acc_s = __builtin_fma(tab[0][a], ps, acc_s);
#pragma unroll
                for (int l = 0; l < SL; ++l) acc_n[l] += l <= a ? pn : 0.0;
            }
        }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        acc_s += __shfl_xor(acc_s, m);
#pragma unroll
        for (int l = 0; l < SL; ++l) acc_n[l] += __shfl_xor(acc_n[l], m);
    }
    if (valid && rl == 0) {
        const double ths = pb.theta0[f] + c_s * acc_s;
        pb.theta[f] = ths;
        double tn[SL];
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            tn[l] = 0.0;
            if (l < nl) {
                tn[l] = pb.theta0[(int64_t)(1 + l) * F + f] + tab[1][l] * c_n * acc_n[l];
                pb.theta[(int64_t)(1 + l) * F + f] = tn[l];
            }
        }
        const double bs = pb.b_sig[f], bn = pb.b_noi[f];
        for (int o = 0; o < n_out; ++o) {
            const int lv = pb.out_level[o];
            double* base = pb.chain + o * plen;
            double fold = 0.0;
#pragma unroll
            for (int l = 0; l < SL; ++l) fold += (l <= lv && l < nl) ? tab[1][l] * tn[l] : 0.0;
            base[o_b + f] = bs;
            base[o_b + F + f] = bn;
            base[o_t + f] = tab[0][lv] * c_s * ths;
            base[o_t + F + f] = c_n * fold;
        }
    }
    for (int e = tid; e < SFC * d; e += ST) {
        const int f2 = fbase + e / d, k = e % d;
        if (f2 >= F) break;
        const double vs = pb.W_sig[(int64_t)f2 * d + k], vn = pb.W_noi[(int64_t)f2 * d + k];
        for (int o = 0; o < n_out; ++o) {
            double* base = pb.chain + o * plen;
            base[o_w + (int64_t)f2 * d + k] = vs;
            base[o_w + (int64_t)(F + f2) * d + k] = vn;
        }
    }
    if (blockIdx.x == 0 && tid < n_out) {
        // the header of layers/rff.py: version 1, one layer, d, 2F features, the length, kind 0; alpha = F, s0 = 1
        double* base = pb.chain + tid * plen;
        const double head[SHEAD] = {1.0, 1.0, (double)d, 2.0 * F, (double)plen, 0.0, (double)F, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < SHEAD; ++q) base[q] = head[q];
    }
}

bool problem_ok(const Problem& p, bool weights) {
    if (p.n < 1 || p.n > MOBOCMF_EXACT_SAMPLE_MAX_N || p.d < 1 || p.d > MOBOCMF_MAX_D || p.n_levels < 1 ||
        p.n_levels > MOBOCMF_EXACT_SAMPLE_MAX_LEVELS || p.F < 1 || p.F > MOBOCMF_EXACT_SAMPLE_MAX_F)
        return false;
    if (!p.x || !p.lev || !p.sig || !p.sqd || !p.scal || !p.W_sig || !p.b_sig || !p.W_noi || !p.b_noi || !p.theta0) return false;
    if (!weights) return p.y && p.ntab && p.e && p.G && p.r;
    if (!p.Linv || !p.a || !p.info || !p.w || !p.theta || !p.info_out || p.n_out < 0 || p.n_out > MOBOCMF_EXACT_SAMPLE_MAX_LEVELS)
        return false;
    if (p.n_out > 0 && !p.chain) return false;
    for (int o = 0; o < p.n_out; ++o)
        if (p.out_level[o] < 0 || p.out_level[o] >= p.n_levels) return false;
    return true;
}

int check_table(const Problem* host, const Problem* dev, int32_t n_problems, bool weights, int* nmax, int* fmax) {
    if (!host || !dev || n_problems < 1 || n_problems > MOBOCMF_EXACT_SAMPLE_MAX_PROBLEMS) return MOBOCMF_BAD_ARG;
    *nmax = *fmax = 0;
    for (int i = 0; i < n_problems; ++i) {
        if (!problem_ok(host[i], weights)) return MOBOCMF_BAD_ARG;
        if (host[i].n > *nmax) *nmax = host[i].n;
        if (host[i].F > *fmax) *fmax = host[i].F;
    }
    return MOBOCMF_OK;
}

inline int launched() { return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR; }

}  // namespace

extern "C" {

int mobocmf_exact_sample_gram(const mobocmf_exact_sample_problem* host_problems, const mobocmf_exact_sample_problem* dev_problems,
                              int32_t n_problems, mobocmf_stream_t stream) {
    int nmax = 0, fmax = 0;
    const int rc = check_table(host_problems, dev_problems, n_problems, false, &nmax, &fmax);
    if (rc != MOBOCMF_OK) return rc;
    const int tiles = npad_of(nmax) / SB;
    hipLaunchKernelGGL(exact_sample_gram_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2), (unsigned)n_problems), dim3(ST), 0,
                       (hipStream_t)stream, dev_problems);
    return launched();
}

int mobocmf_exact_sample_weights(const mobocmf_exact_sample_problem* host_problems, const mobocmf_exact_sample_problem* dev_problems,
                                 int32_t n_problems, mobocmf_stream_t stream) {
    int nmax = 0, fmax = 0;
    const int rc = check_table(host_problems, dev_problems, n_problems, true, &nmax, &fmax);
    if (rc != MOBOCMF_OK) return rc;
    hipLaunchKernelGGL(exact_sample_solve_kernel, dim3((unsigned)((nmax + 3) / 4), (unsigned)n_problems), dim3(ST), 0,
                       (hipStream_t)stream, dev_problems);
    if (launched() != MOBOCMF_OK) return MOBOCMF_HIP_ERROR;
    hipLaunchKernelGGL(exact_sample_weights_kernel, dim3((unsigned)((fmax + SFC - 1) / SFC), (unsigned)n_problems), dim3(ST), 0,
                       (hipStream_t)stream, dev_problems);
    return launched();
}

}  // extern "C"
