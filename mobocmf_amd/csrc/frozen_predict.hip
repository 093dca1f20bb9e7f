// Predictive moments of fitted surrogates with 128 < M <= 1024 inducing points against their FROZEN chains, and the gradient
// w.r.t. the test points: mobocmf_frozen_predict (M <= 512) and mobocmf_frozen_predict_split (M <= 1024) (include/mobocmf_hip.h),
// the model evaluation of an acquisition search (JESMOC_MFDGP(search="device"), util/panel_predict.py) where the one-launch
// steps (tiny_step.hip, coop_step.hip) stop.
//
// A search evaluates n models at the same T test points, T S columns per model -- 125 at the search's own sizes: one tile of
// the layer path's grid-filling products -- against parameters that stay constant, so L^-1, L^-T, U, U^T and a of every layer
// exist already (the layer's CHAIN state, state_bytes of mobocmf_chain_block_bytes).  Every column of every layer depends on
// its own base row only:
//
//   a WORKGROUP owns (model, a block of base rows), runs ALL layers for those rows and their S replicas, 16 columns at a time,
//   and sums its rows' d/dx in a fixed order.
//
// Nothing is shared between workgroups: no in-launch barrier, no counters, no atomics, no wait -- hence nothing to abandon and no
// status word.  Per block of 16 columns the layer's eval branch runs column by column,
//
//   K = k(Z~, [x, f])   A = L^-1 K   C = U^T A   mean = a^T A   var = max(k_nn - |A|^2 + |C|^2, 1e-10)
//   dA = 2 U (C gv) + a g_mean - 2 A gv   dK = L^-T dA   then the Gram backward w.r.t. x and f,
//
// the four triangular products on v_mfma_f64_16x16x4_f64 with the M x M operand streamed from global memory (L2: every workgroup
// of a model reads the same 2 MB at M = 512) and the [M][16] panels in LDS -- two of them, 64 KB each at M = 512, which is what
// bounds M: K -> A -> C reuse them in turn (C over K), and so do dA (over A, element by element) and dK (over C).
// MOBOCMF_STEP_INPUT_GRADIENTS forms the panels again instead of reading saved ones: the top layer's blocks run forward and
// backward back to back on the panels they have in LDS, the layers below are re-formed (their S-fold fewer columns at layer 0),
// and no M x T S storage exists in either mode.
//
// mobocmf_frozen_predict_split is the same kernel on panels of CW = 8 columns ([M][8]: two of them and a are 136 KB at M = 1024)
// with the S replicas of a base row SPLIT over workgroups:
//
//   L >= 2: a workgroup owns (model, base row t, part p) -- the replicas s in [8 p, 8 p + 8) -- and runs the whole chain for
//           them: layer 0's single column of row t (every part forms it again), then its <= 8 columns of every layer above
//           (column (t, s) of layer l >= 2 reads column (t, s) of layer l - 1 only);   L = 1: a workgroup owns 8 base rows.
//
// The backward below the top layer is linear in what the layer above sends back and the floor gate depends on the forward alone,
// so every part back-propagates its own sum g_f, sum g_f eps through layer 0 and writes a partial d/dx of its row to `work`
// ([part][T][d]); frozen_split_reduce_kernel, the second launch of the call, sums the parts in ascending order.  Of an MFMA's 16
// output columns the upper eight duplicate the lower eight and are never stored.
#include <atomic>

#include "small_step_common.h"
#include "tile16.h"

namespace {

constexpr int FT = 512;                      // threads per workgroup: two wavefronts per SIMD (the products wait for L2)
constexpr int FNW = FT / 64;
// (a panel row is CW doubles: the four k rows a B fragment reads are 256 (CW = 8) or 512 (CW = 16) contiguous bytes)
constexpr int FCOLS = MOBOCMF_MAX_XDIV;      // columns of a layer a workgroup holds, at most (S > 16: one base row)
constexpr int FXFW = DBT + 2;                // a staged column: x (zero padded), f, valid flag
constexpr int FRED = DBT + 1;
constexpr int SCW = 8;                       // columns of a panel, and replicas of a part, of the split form

typedef const __attribute__((address_space(1))) double* gcd;
#define GC(p) ((gcd)(p))

// base rows per workgroup: one 16-column block per layer where S allows it
__host__ __device__ inline int frozen_rows_per_wg(int L, int S) { return L == 1 ? 16 : (S >= 16 ? 1 : 16 / S); }

// base rows (L = 1) or replicas of a base row (L >= 2) of a workgroup of the split form, and the parts of a base row
__host__ __device__ inline int frozen_split_parts(int L, int S) { return L == 1 ? 1 : (S + SCW - 1) / SCW; }
__host__ __device__ inline int frozen_split_grid(int L, int S, int T) { return L == 1 ? (T + SCW - 1) / SCW : T * frozen_split_parts(L, S); }

// One 16 x 16 tile of T X for a panel X [k][CW] in LDS and T given k-major in global memory (Tk[k * ld + row] = T[row][k]),
// k tiles kt0 .. kt1-1; the fragments of four k tiles are requested together (coop_step.hip tile_tx).  CW = 8: the lanes of
// output columns 8 .. 15 read columns 0 .. 7 again (the same LDS words: a broadcast), and the caller drops what they hold.
template <int CW>
__device__ __forceinline__ v4d tile_tx(const double* Tk_, int ld, const double* X, int t, int kt0, int kt1, int lane) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    const int li = lane & 15, lk = lane >> 4;
    gcd tp = GC(Tk_) + (int64_t)lk * ld + t * 16 + li;
    const double* xp = X + lk * CW + (li & (CW - 1));
    for (int kb = kt0; kb < kt1; kb += 4) {
        double a[4][4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int kt = kb + kk < kt1 ? kb + kk : kt1 - 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) a[kk][q] = tp[(int64_t)(kt * 16 + 4 * q) * ld];
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kb + kk < kt1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = mfma(a[kk][q], xp[((kb + kk) * 16 + 4 * q) * CW], acc);
            }
        }
    }
    return acc;
}
__device__ __forceinline__ double xor_add(double v, int mask) { return v + __shfl_xor(v, mask); }
// the sum over the lanes of a wavefront that keep the same column (lane % CW)
template <int CW>
__device__ __forceinline__ double column_sum(double v) {
    v = xor_add(xor_add(v, 16), 32);
    if constexpr (CW == 8) v = xor_add(v, 8);
    return v;
}
// the i-th output tile of wavefront w: w, 2 FNW - 1 - w, 2 FNW + w, ... -- a lower and an upper triangular operand (k tiles
// 0..t and t..nt-1) both give every wavefront the same number of k tiles
__device__ __forceinline__ int tile_of_wave(int i, int w) { return (i & 1) ? i * FNW + FNW - 1 - w : i * FNW + w; }

// CW: the columns of a panel and of a block.  SPLIT: the ownership rule -- false: (model, a block of base rows), CW = 16; true:
// (model, base row, part of its replicas), CW = 8 (the header of this file).  A column c of a workgroup's layer l is, SPLIT:
// replica s0 + c of the one base row (layer 0: base row c, a single one where L >= 2); else replica c % S of base row c / S.
template <bool INGRAD, int CW, bool SPLIT>
__global__ __launch_bounds__(FT) void frozen_predict_kernel(const mobocmf_frozen_predict_model* models) {
    static_assert(CW == (SPLIT ? SCW : 16), "a block of base rows on 16-column panels, or split replicas on 8-column ones");
    constexpr int LOGCW = CW == 16 ? 4 : 3;
    constexpr int NCOL = SPLIT ? CW : FCOLS;      // columns of a layer a workgroup holds, at most
    extern __shared__ __attribute__((aligned(16))) double fp_lds[];
    __shared__ double hy[TLM * HS], il[TLM * 2 * DBT], epsv[TLM * NCOL];
    __shared__ double xr[CW * DBT], gxacc[CW * DBT], xf[CW * FXFW], gcol[2 * CW], dxblk[CW * FRED];
    __shared__ double vmean[TLM * NCOL], vvar[TLM * NCOL];        // per column of every layer: the moments ...
    __shared__ double vgm[TLM * NCOL], vge[TLM * NCOL];           // ... and what the layer above sent back: sum g_f, sum g_f eps
    __shared__ double red[FNW * CW * FRED];

    const mobocmf_frozen_predict_model& md = models[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int L = md.L, M = md.M, d = md.d, S = L > 1 ? md.S : 1, T = md.T;
    const int Mp = (M + TILE - 1) / TILE * TILE, nt = (M + 15) / 16, Mr = nt * 16;
    const int parts = SPLIT ? frozen_split_parts(L, S) : 1, part = SPLIT ? blockIdx.x % parts : 0;
    const int RB = SPLIT ? (L == 1 ? CW : 1) : frozen_rows_per_wg(L, S);
    const int r0 = SPLIT ? blockIdx.x / parts * RB : blockIdx.x * RB;
    if (r0 >= T) return;      // (a launch's grid is sized for its largest model)
    const int nb = T - r0 < RB ? T - r0 : RB;
    const int s0 = part * CW, ns = S - s0 < CW ? S - s0 : CW;      // (SPLIT) the part's replicas
    double* X0 = fp_lds;
    double* X1 = X0 + Mr * CW;
    double* av = X1 + Mr * CW;

    // ---- constants of the launch: packed hyper-parameters, inverse lengthscales, the layers' fixed samples, the base rows
    for (int e = tid; e < TLM * HS; e += FT) {
        const int l = e / HS, t = e % HS;
        hy[e] = (l < L && t < (l ? 5 + 2 * d : 1 + d)) ? GC(md.hyp[l])[t] : 0.0;
    }
    for (int e = tid; e < TLM * NCOL; e += FT) {
        const int l = e / NCOL, s = e % NCOL;
        epsv[e] = (l >= 1 && l < L && s < (SPLIT ? ns : S)) ? GC(md.samples[l])[SPLIT ? s0 + s : s] : 0.0;
        vgm[e] = 0.0;
        vge[e] = 0.0;
    }
    for (int e = tid; e < CW * DBT; e += FT) {
        const int r = e / DBT, k = e % DBT;
        xr[e] = (r < nb && k < d) ? GC(md.x)[(int64_t)(r0 + r) * d + k] : 0.0;
        gxacc[e] = 0.0;
    }
    __syncthreads();
    for (int e = tid; e < TLM * 2 * DBT; e += FT) {
        const int l = e / (2 * DBT), kk = e % (2 * DBT), k2 = kk % DBT;
        double v = 0.0;
        if (l < L && k2 < d) {
            if (l == 0) v = kk < DBT ? 1.0 / hy[l * HS + 1 + k2] : 0.0;
            else v = 1.0 / hy[l * HS + 5 + (kk < DBT ? 0 : d) + k2];
        }
        il[e] = v;
    }
    __syncthreads();

    // ---- one block of CW columns of layer l: forward, and (bwd) backward on the panels it has just formed
    auto block = [&](int l, int cb, bool bwd) {
        const int kind = l > 0, div = l ? S : 1, nc = SPLIT ? (l ? ns : nb) : nb * div, c0 = cb * CW;
        const double* hyl = hy + l * HS;
        const double* ill = il + l * 2 * DBT;
        const int64_t mm = (int64_t)Mp * Mp;
        const double* cs = (const double*)md.chain[l];      // [L | L^-1 | L^-T | U | U^T | L_S | a | m], Mp x Mp each, then Mp
        const double *Linv = cs + FCS_LINV * mm, *LinvT = cs + FCS_LINVT * mm, *U = cs + FCS_U * mm, *UT = cs + FCS_UT * mm;
        gcd ag = GC(cs + FCS_A * mm), zx = GC(md.Zx[l]), zf = GC(md.zf[l]);
        // the block's columns: base row, f = mean + sqrt(var) eps of the layer below (layer 0's column serves the S replicas)
        if (tid < CW) {
            const int c = c0 + tid, valid = c < nc, b = valid ? (SPLIT ? (l ? 0 : c) : c / div) : 0;
            double f = 0.0;
            if (valid && l > 0) {
                const int pc = (l - 1) * NCOL + (l == 1 ? b : c);
                f = vmean[pc] + sqrt(vvar[pc]) * epsv[l * NCOL + (SPLIT ? c : c % S)];
            }
#pragma unroll
            for (int k = 0; k < DBT; ++k) xf[tid * FXFW + k] = valid ? xr[b * DBT + k] : 0.0;
            xf[tid * FXFW + DBT] = f;
            xf[tid * FXFW + DBT + 1] = valid ? 1.0 : 0.0;
        }
        for (int e = tid; e < Mr; e += FT) av[e] = e < M ? ag[e] : 0.0;
        __syncthreads();
        // K
#pragma unroll 1
        for (int e = tid; e < Mr * CW; e += FT) {
            const int m = e >> LOGCW, j = e & (CW - 1);
            double v = 0.0;
            if (m < M && xf[j * FXFW + DBT + 1] != 0.0) {
                double zb[ZW];
#pragma unroll
                for (int k = 0; k < DBT; ++k) zb[k] = k < d ? zx[(int64_t)m * d + k] : 0.0;
                zb[DBT] = kind ? zf[m] : 0.0;
                KV o;
                kern_eval(kind, d, xf + j * FXFW, xf[j * FXFW + DBT], zb, hyl, ill, o);
                v = o.k;
            }
            X0[m * CW + j] = v;
        }
        __syncthreads();
        // A = L^-1 K
        for (int i = 0; i * FNW < nt; ++i) {
            const int t = tile_of_wave(i, wave);
            if (t < nt) {
                const v4d acc = tile_tx<CW>(LinvT, Mp, X0, t, 0, t + 1, lane);
                if (CW == 16 || li < CW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) X1[(t * 16 + 4 * r + lk) * CW + li] = acc[r];
                }
            }
        }
        __syncthreads();
        // C = U^T A (over K)
        for (int i = 0; i * FNW < nt; ++i) {
            const int t = tile_of_wave(i, wave);
            if (t < nt) {
                const v4d acc = tile_tx<CW>(U, Mp, X1, t, t, nt, lane);
                if (CW == 16 || li < CW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) X0[(t * 16 + 4 * r + lk) * CW + li] = acc[r];
                }
            }
        }
        __syncthreads();
        // moments: a thread keeps one column (FT is a multiple of CW) and every (FT / CW)-th row; summed through the wavefront,
        // then over the wavefronts in order
        const int cj = tid & (CW - 1);
        {
            double q = 0.0, mu = 0.0, r = 0.0;
            for (int m = tid >> LOGCW; m < Mr; m += FT / CW) {
                const double a = X1[m * CW + cj], c = X0[m * CW + cj];
                q += a * a;
                mu += av[m] * a;
                r += c * c;
            }
            q = column_sum<CW>(q);
            mu = column_sum<CW>(mu);
            r = column_sum<CW>(r);
            if (lane < CW) {
                red[(wave * CW + lane) * 3 + 0] = q;
                red[(wave * CW + lane) * 3 + 1] = mu;
                red[(wave * CW + lane) * 3 + 2] = r;
            }
        }
        __syncthreads();
        if (tid < CW) {
            const int c = c0 + tid;
            double gm = 0.0, gvc = 0.0;
            if (c < nc) {
                double q = 0.0, mu = 0.0, r = 0.0;
#pragma unroll
                for (int p = 0; p < FNW; ++p) {
                    q += red[(p * CW + tid) * 3 + 0];
                    mu += red[(p * CW + tid) * 3 + 1];
                    r += red[(p * CW + tid) * 3 + 2];
                }
                const double fn = xf[tid * FXFW + DBT];
                const double knn = kind ? hyl[0] * (hyl[2] * fn * fn + hyl[1]) + hyl[3] : hyl[0];
                const double vr = (knn - q) + r, var = vr < MINV ? MINV : vr;
                vmean[l * NCOL + c] = mu;
                vvar[l * NCOL + c] = var;
                const int64_t gc = SPLIT ? (l ? (int64_t)r0 * S + s0 + c : (int64_t)r0 + c) : (int64_t)r0 * div + c;
                if (l == L - 1) { md.top_mean[gc] = mu; md.top_var[gc] = var; }
                if (INGRAD && bwd) {
                    double gv;
                    if (l == L - 1) { gm = GC(md.seed_gmean)[gc]; gv = GC(md.seed_gvar)[gc]; }
                    else { gm = vgm[l * NCOL + c]; gv = vge[l * NCOL + c] * 0.5 / sqrt(var); }
                    gvc = vr > MINV ? gv : 0.0;      // clamp_min passes gradient only above the floor
                }
            }
            gcol[tid] = gm;
            gcol[CW + tid] = gvc;
        }
        __syncthreads();
        if (!INGRAD || !bwd) return;
        // dA = 2 U (C gv) + a g_mean - 2 A gv (over A: an element of dA needs the same element of A only)
        for (int i = 0; i * FNW < nt; ++i) {
            const int t = tile_of_wave(i, wave);
            if (t < nt) {
                const v4d acc = tile_tx<CW>(UT, Mp, X0, t, 0, t + 1, lane);
                if (CW == 16 || li < CW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = t * 16 + 4 * r + lk;
                        X1[row * CW + li] = 2.0 * gcol[CW + li] * acc[r] + av[row] * gcol[li] - 2.0 * X1[row * CW + li] * gcol[CW + li];
                    }
                }
            }
        }
        __syncthreads();
        // dK = L^-T dA (over C)
        for (int i = 0; i * FNW < nt; ++i) {
            const int t = tile_of_wave(i, wave);
            if (t < nt) {
                const v4d acc = tile_tx<CW>(Linv, Mp, X1, t, t, nt, lane);
                if (CW == 16 || li < CW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) X0[(t * 16 + 4 * r + lk) * CW + li] = acc[r];
                }
            }
        }
        __syncthreads();
        // Gram backward w.r.t. the columns' inputs: a thread keeps one column (FT is a multiple of CW) and sums over its inducing rows
        {
            double dxa[DBT], dfs = 0.0;
#pragma unroll
            for (int t = 0; t < DBT; ++t) dxa[t] = 0.0;
#pragma unroll 1
            for (int e = tid; e < Mr * CW; e += FT) {
                const int m = e >> LOGCW;
                if (m < M && xf[cj * FXFW + DBT + 1] != 0.0) {
                    double zb[ZW];
#pragma unroll
                    for (int k = 0; k < DBT; ++k) zb[k] = k < d ? zx[(int64_t)m * d + k] : 0.0;
                    zb[DBT] = kind ? zf[m] : 0.0;
                    kern_back_in(kind, d, xf + cj * FXFW, xf[cj * FXFW + DBT], zb, hyl, ill, X0[m * CW + cj], dxa, dfs);
                }
            }
#pragma unroll
            for (int t = 0; t <= DBT; ++t) {
                const double v = column_sum<CW>(t < DBT ? dxa[t < DBT ? t : 0] : dfs);
                if (lane < CW) red[(wave * CW + lane) * FRED + t] = v;
            }
        }
        __syncthreads();
        if (tid < CW * FRED) {
            const int j = tid / FRED, t = tid % FRED, c = c0 + j;
            double sum = 0.0;
#pragma unroll
            for (int p = 0; p < FNW; ++p) sum += red[(p * CW + j) * FRED + t];
            if (t == DBT && kind) sum += gcol[CW + j] * hyl[0] * 2.0 * hyl[2] * xf[j * FXFW + DBT];      // d k_nn / d f
            dxblk[tid] = c < nc ? sum : 0.0;
        }
        __syncthreads();
        // the block's share of its base rows' d/dx, and of the gradients of the layer below, column by column in order
        if (tid < CW * DBT) {
            const int r = tid / DBT, t = tid % DBT;
            if (r < nb) {
                double sum = gxacc[tid];
                for (int j = 0; j < CW; ++j)
                    if (c0 + j < nc && (SPLIT ? (l ? 0 : c0 + j) : (c0 + j) / div) == r) sum += dxblk[j * FRED + t];
                gxacc[tid] = sum;
            }
        } else if (l > 0 && tid >= 256 && tid < 256 + NCOL) {
            const int pc = tid - 256, npc = l == 1 ? nb : nc;
            if (pc < npc) {
                double gm = vgm[(l - 1) * NCOL + pc], ge = vge[(l - 1) * NCOL + pc];
                for (int j = 0; j < CW; ++j) {
                    const int c = c0 + j;
                    if (c < nc && (l == 1 ? (SPLIT ? 0 : c / S) : c) == pc) {
                        const double g = dxblk[j * FRED + DBT];
                        gm += g;
                        ge += g * epsv[l * NCOL + (SPLIT ? c : c % S)];
                    }
                }
                vgm[(l - 1) * NCOL + pc] = gm;
                vge[(l - 1) * NCOL + pc] = ge;
            }
        }
        __syncthreads();
    };

    auto blocks_of = [&](int l) { return SPLIT ? 1 : (nb * (l ? S : 1) + 15) / 16; };
    for (int l = 0; l < L; ++l)
        for (int cb = 0; cb < blocks_of(l); ++cb) block(l, cb, l == L - 1);
    if constexpr (INGRAD) {
        for (int l = L - 2; l >= 0; --l)
            for (int cb = 0; cb < blocks_of(l); ++cb) block(l, cb, true);
        if (SPLIT && L > 1) {      // the part's share of its base row: `work` [part][T][d], summed by frozen_split_reduce_kernel
            if (tid < d) ((double*)md.work)[((int64_t)part * T + r0) * d + tid] = gxacc[tid];
        } else if (tid < nb * d) md.grad[(int64_t)r0 * d + tid] = gxacc[(tid / d) * DBT + tid % d];
    }
}

// grad of the split form's models with L >= 2: the parts' partial d/dx in ascending part order (every slot read here was written
// by the launch before, in the same call)
__global__ __launch_bounds__(256) void frozen_split_reduce_kernel(const mobocmf_frozen_predict_model* models) {
    const mobocmf_frozen_predict_model& md = models[blockIdx.y];
    if (md.L < 2) return;
    const int n = md.T * md.d, parts = frozen_split_parts(md.L, md.S);
    gcd w = GC((const double*)md.work);
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        double sum = 0.0;
        for (int p = 0; p < parts; ++p) sum += w[(int64_t)p * n + e];
        md.grad[e] = sum;
    }
}

template <int CW>
inline size_t frozen_lds_bytes(int M) { return (size_t)(2 * CW + 1) * ((M + 15) / 16 * 16) * sizeof(double); }

template <bool INGRAD, int CW, bool SPLIT>
int launch_kernel(const mobocmf_frozen_predict_model* dev_models, dim3 grid, size_t shm, hipStream_t s) {
    // the dynamic-LDS attribute is per device: one bit per device ordinal (gemm_f64.hip launch_small_panel)
    static std::atomic<uint64_t> configured{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return MOBOCMF_HIP_ERROR;
    if (!(configured.load(std::memory_order_acquire) & (1ull << dev))) {
        if (hipFuncSetAttribute((const void*)frozen_predict_kernel<INGRAD, CW, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)frozen_lds_bytes<CW>(SPLIT ? MOBOCMF_FROZEN_SPLIT_MAX_M : MOBOCMF_FROZEN_MAX_M)) != hipSuccess)
            return MOBOCMF_HIP_ERROR;
        configured.fetch_or(1ull << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL((frozen_predict_kernel<INGRAD, CW, SPLIT>), grid, dim3(FT), shm, s, dev_models);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

}  // namespace

// Descriptors validated by the caller (api.hip, which also vouches for the chain-state layout the kernel indexes).
int launch_frozen_predict(const mobocmf_frozen_predict_model* host_models, const mobocmf_frozen_predict_model* dev_models,
                          int n_models, bool input_gradients, hipStream_t s) {
    int mmax = 0, gx = 1;
    for (int i = 0; i < n_models; ++i) {
        const mobocmf_frozen_predict_model& m = host_models[i];
        const int rb = frozen_rows_per_wg(m.L, m.L > 1 ? m.S : 1);
        if (m.M > mmax) mmax = m.M;
        if ((m.T + rb - 1) / rb > gx) gx = (m.T + rb - 1) / rb;
    }
    const dim3 grid((unsigned)gx, (unsigned)n_models);
    const size_t shm = frozen_lds_bytes<16>(mmax);
    return input_gradients ? launch_kernel<true, 16, false>(dev_models, grid, shm, s)
                           : launch_kernel<false, 16, false>(dev_models, grid, shm, s);
}

// The split form (descriptors validated by api.hip, `work` included): one launch, and for the input gradient of models with
// L >= 2 the reduction of the parts' partials after it on the same stream.
int launch_frozen_predict_split(const mobocmf_frozen_predict_model* host_models, const mobocmf_frozen_predict_model* dev_models,
                                int n_models, bool input_gradients, hipStream_t s) {
    int mmax = 0, gx = 1, nred = 0;
    for (int i = 0; i < n_models; ++i) {
        const mobocmf_frozen_predict_model& m = host_models[i];
        const int g = frozen_split_grid(m.L, m.L > 1 ? m.S : 1, m.T);
        if (m.M > mmax) mmax = m.M;
        if (g > gx) gx = g;
        if (m.L > 1 && m.T * m.d > nred) nred = m.T * m.d;
    }
    const dim3 grid((unsigned)gx, (unsigned)n_models);
    const size_t shm = frozen_lds_bytes<SCW>(mmax);
    if (!input_gradients) return launch_kernel<false, SCW, true>(dev_models, grid, shm, s);
    const int rc = launch_kernel<true, SCW, true>(dev_models, grid, shm, s);
    if (rc != MOBOCMF_OK || nred == 0) return rc;
    hipLaunchKernelGGL(frozen_split_reduce_kernel, dim3((unsigned)((nred + 255) / 256), (unsigned)n_models), dim3(256), 0, s, dev_models);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}
