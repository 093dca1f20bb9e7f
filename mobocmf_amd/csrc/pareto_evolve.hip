// NSGA-II over chain samples: the population logic of MOOP(search="evolve") (include/mobocmf_hip.h states the algorithm; the
// objective values and violations come from mobocmf_rff_eval_chains / mobocmf_rff_feasibility).
//
// (a) mobocmf_nsga_survive: ONE workgroup, thread i = input row i.  The constraint-domination relation is a bit matrix in LDS
//     (word w of row i = which of the rows 32 w .. 32 w + 31 dominate row i, stored [w][i] so that a wave reads consecutive
//     words); ranks by peeling it against the word mask of the rows still alive, two workgroup barriers per rank; crowding
//     neighbours and order positions by counting over the rows.  The objective values sit in LDS beside the bit matrix when
//     they fit (k n 8 bytes), else every pass reads them from global memory at a wave-uniform address.  Survivors are gathered
//     through registers, every read before any write, so the outputs may be the inputs.
// (b) mobocmf_nsga_vary: one thread per (pair, variable): tournament, simulated binary crossover, polynomial mutation, every
//     uniform addressed by (seed, generation word, pair, slot).
#include <math.h>

#include "common.h"

#define NS_MAXN MOBOCMF_NSGA_MAX_ROWS
#define NS_LDS_MAX (160 * 1024 - 512)      // LDS of a CDNA4 workgroup, less the kernel's static part (the barrier count's words)

struct NsLayout {
    int W;                           // 32-bit words per row of the bit matrix
    size_t dom, val, rank, alive, fs, total;   // byte offsets; `val` holds the violations, later the crowding distances
    int f_lds;                       // the objective values fit beside the bit matrix
};

static NsLayout ns_layout(int n, int k) {
    NsLayout L;
    L.W = (n + 31) / 32;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 15) / 16 * 16; return at; };
    L.dom = take((size_t)L.W * n * 4);     // (the survivors' source rows reuse it after the peeling: n words fit in W n)
    L.val = take((size_t)n * 8);
    L.rank = take((size_t)n * 4);
    L.alive = take((size_t)L.W * 4);
    L.f_lds = o + (size_t)k * n * 8 <= NS_LDS_MAX;
    L.fs = take(L.f_lds ? (size_t)k * n * 8 : 0);
    L.total = o;
    return L;
}

struct NsArgs {
    int n, n_keep, d, k, W, f_lds;
    unsigned o_val, o_rank, o_alive, o_fs;
    const double *X, *F, *viol;
    int64_t ldf, ldf_out;
    double *X_out, *F_out, *viol_out, *crowd_out;
    int32_t *rank_out, *src_out;
    int64_t* generation;
};

// (no __restrict__ on the rows: the outputs may be the inputs)
template <int KB>
__global__ __launch_bounds__(NS_MAXN) void nsga_survive_kernel(const NsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char ns_lds[];
    uint32_t* dom = (uint32_t*)ns_lds;
    double* sval = (double*)(ns_lds + a.o_val);
    int32_t* srank = (int32_t*)(ns_lds + a.o_rank);
    uint32_t* salive = (uint32_t*)(ns_lds + a.o_alive);
    double* Fs = (double*)(ns_lds + a.o_fs);
    int32_t* ssrc = (int32_t*)ns_lds;
    const int n = a.n, k = a.k, W = a.W, i = threadIdx.x;
    const bool live = i < n;
    const bool f_lds = a.f_lds != 0;
    const double inf = __builtin_inf();

    // ---- the row: objective values, violation (NaN anywhere: infeasible, +inf)
    double mine[KB];
    bool nan = false;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        mine[c] = (live && c < k) ? a.F[(int64_t)c * a.ldf + i] : 0.0;
        nan = nan || mine[c] != mine[c];
    }
    double vi = (live && a.viol) ? a.viol[i] : 0.0;
    if (nan || vi != vi) vi = inf;
    const bool feas = vi == 0.0;
    if (live) {
        sval[i] = vi;
        srank[i] = -1;
        if (f_lds)
            for (int c = 0; c < k; ++c) Fs[c * n + i] = a.F[(int64_t)c * a.ldf + i];
    }
    if (i < W) {
        const int left = n - 32 * i;
        salive[i] = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
    }
    __syncthreads();

    // ---- who dominates row i
    if (live) {
        for (int w = 0; w < W; ++w) {
            uint32_t bits = 0;
            const int cnt = n - 32 * w < 32 ? n - 32 * w : 32;
            for (int b = 0; b < cnt; ++b) {
                const int j = 32 * w + b;
                const double vj = sval[j];
                bool dm;
                if (vj == 0.0) {                       // (uniform: every thread looks at the same j)
                    dm = true;
                    if (feas) {
                        bool le = true, lt = false;
#pragma unroll
                        for (int c = 0; c < KB; ++c) {
                            if (c < k) {
                                const double q = f_lds ? Fs[c * n + j] : a.F[(int64_t)c * a.ldf + j];
                                le = le && q <= mine[c];
                                lt = lt || q < mine[c];
                            }
                        }
                        dm = le && lt;
                    }
                } else {
                    dm = !feas && vj < vi;
                }
                bits |= (dm ? 1u : 0u) << b;
            }
            dom[w * n + i] = bits;
        }
    }
    __syncthreads();

    // ---- ranks: peel the rows no living row dominates (at most n ranks: a strict partial order has a minimal element)
    int rank = -1;
    bool alive = live;
    for (int r = 0; r < n; ++r) {
        bool held = false;
        if (alive)
            for (int w = 0; w < W && !held; ++w) held = (dom[w * n + i] & salive[w]) != 0u;
        const int left = __syncthreads_count(alive && held);      // every read of salive precedes the updates below
        if (alive && !held) {
            rank = r;
            alive = false;
            atomicAnd(&salive[i >> 5], ~(1u << (i & 31)));
        }
        __syncthreads();
        if (left == 0) break;                                      // uniform
    }
    if (live) srank[i] = rank;
    __syncthreads();

    // ---- crowding within the rank, one term per objective in order
    double crowd = 0.0;
    if (live) {
        for (int c = 0; c < k; ++c) {
            double me = f_lds ? Fs[c * n + i] : a.F[(int64_t)c * a.ldf + i];
            if (me != me) me = inf;
            double mn = me, mx = me, pv = 0.0, nv = 0.0;
            bool hasp = false, hasn = false;
            for (int m = 0; m < n; ++m) {
                if (srank[m] != rank || m == i) continue;
                double q = f_lds ? Fs[c * n + m] : a.F[(int64_t)c * a.ldf + m];
                if (q != q) q = inf;
                mn = q < mn ? q : mn;
                mx = q > mx ? q : mx;
                if (q < me || (q == me && m < i)) {
                    if (!hasp || q > pv) pv = q;
                    hasp = true;
                } else {
                    if (!hasn || q < nv) nv = q;
                    hasn = true;
                }
            }
            double term;
            if (!hasp || !hasn) term = inf;
            else if (mx == mn) term = 0.0;
            else {
                term = (nv - pv) / (mx - mn);
                if (term != term) term = 0.0;
            }
            crowd = crowd + term;
        }
        sval[i] = crowd;                       // (the violations were last read before the peeling)
    }
    __syncthreads();

    // ---- position under (rank ascending, crowding descending, row ascending)
    int pos = n;
    if (live) {
        pos = 0;
        for (int m = 0; m < n; ++m) {
            const int rm = srank[m];
            const double cm = sval[m];
            pos += (rm < rank || (rm == rank && (cm > crowd || (cm == crowd && m < i)))) ? 1 : 0;
        }
    }
    // the viol input of row i was read at the top; every thread is past several barriers since
    if (pos < a.n_keep) {
        ssrc[pos] = i;                         // (the bit matrix is dead)
        a.src_out[pos] = i;
        a.rank_out[pos] = rank;
        a.crowd_out[pos] = crowd;
        if (a.viol_out) a.viol_out[pos] = vi;
    }
    __syncthreads();

    // ---- gather the survivors: all reads, a barrier, all writes
    const bool out = i < a.n_keep;
    const int s = out ? ssrc[i] : 0;
    {
        double xr[MOBOCMF_MAX_D];
#pragma unroll
        for (int c = 0; c < MOBOCMF_MAX_D; ++c) xr[c] = (out && c < a.d) ? a.X[(int64_t)s * a.d + c] : 0.0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < MOBOCMF_MAX_D; ++c)
            if (out && c < a.d) a.X_out[(int64_t)i * a.d + c] = xr[c];
    }
    {
        double fr[KB];
#pragma unroll
        for (int c = 0; c < KB; ++c) fr[c] = (out && c < k) ? a.F[(int64_t)c * a.ldf + s] : 0.0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (out && c < k) a.F_out[(int64_t)c * a.ldf_out + i] = fr[c];
    }
    if (i == 0 && a.generation) a.generation[0] = a.generation[0] + 1;
}

extern "C" int mobocmf_nsga_survive(int32_t n_in, int32_t n_keep, int32_t d, int32_t k, const double* X, const double* F,
                                    int64_t ldf, const double* viol, double* X_out, double* F_out, int64_t ldf_out,
                                    double* viol_out, int32_t* rank_out, double* crowd_out, int32_t* src_out,
                                    int64_t* generation, mobocmf_stream_t stream) {
    if (k < 1 || k > MOBOCMF_PARETO_MAX_K || d < 1 || d > MOBOCMF_MAX_D || n_keep < 2 || n_keep > n_in || n_in > NS_MAXN)
        return MOBOCMF_BAD_ARG;
    if (!X || !F || !X_out || !F_out || !rank_out || !crowd_out || !src_out || ldf < n_in || ldf_out < n_keep ||
        (viol && !viol_out))
        return MOBOCMF_BAD_ARG;
    const NsLayout L = ns_layout(n_in, k);
    NsArgs a;
    a.n = n_in; a.n_keep = n_keep; a.d = d; a.k = k; a.W = L.W; a.f_lds = L.f_lds;
    a.o_val = (unsigned)L.val; a.o_rank = (unsigned)L.rank; a.o_alive = (unsigned)L.alive; a.o_fs = (unsigned)L.fs;
    a.X = X; a.F = F; a.viol = viol; a.ldf = ldf; a.ldf_out = ldf_out;
    a.X_out = X_out; a.F_out = F_out; a.viol_out = viol_out; a.crowd_out = crowd_out;
    a.rank_out = rank_out; a.src_out = src_out; a.generation = generation;
    const dim3 block((unsigned)round_up(n_in, 64));
#define NS_GO(KB)                                                                                                          \
    do {                                                                                                                   \
        if (L.total > 64 * 1024)   /* (a property of the loaded kernel, not of a call: setting it again is harmless) */    \
            HIP_TRY(hipFuncSetAttribute((const void*)nsga_survive_kernel<KB>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                        NS_LDS_MAX));                                                                      \
        hipLaunchKernelGGL((nsga_survive_kernel<KB>), dim3(1), block, L.total, (hipStream_t)stream, a);                    \
    } while (0)
    if (k <= 2) NS_GO(2);
    else if (k <= 4) NS_GO(4);
    else NS_GO(16);
#undef NS_GO
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

// ------------------------------------------------------------------ (b) variation
static const mobocmf_nsga_options kDefaultNsga = {sizeof(mobocmf_nsga_options), 0u, 15.0, 0.9, 20.0, 0.0};

extern "C" int mobocmf_nsga_options_init(mobocmf_nsga_options* opt) {
    if (!opt) return MOBOCMF_BAD_ARG;
    *opt = kDefaultNsga;
    return MOBOCMF_OK;
}

static bool nsga_options_ok(const mobocmf_nsga_options& o) {
    return o.struct_size == sizeof(mobocmf_nsga_options) && o.eta_c >= 0.0 && o.eta_c <= 1000.0 && o.p_c >= 0.0 &&
           o.p_c <= 1.0 && o.eta_m >= 0.0 && o.eta_m <= 1000.0 && o.p_m >= 0.0 && o.p_m <= 1.0;     // (NaN fails every one)
}

#define NV_T 64

// x^e (x > 0) of the header: IEEE operations only, nothing fused, so that the host restatement gives the same bits
#define NV_LN2 0.6931471805599453
__device__ __forceinline__ double nv_lg(double x) {
#pragma clang fp contract(off)
    int n;
    double m = frexp(x, &n);
    if (m < 0.7071067811865476) {
        m = 2.0 * m;
        n = n - 1;
    }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double P = 1.0 / 23.0;
#pragma unroll
    for (int j = 21; j >= 1; j -= 2) P = P * z + 1.0 / (double)j;
    return (double)n * NV_LN2 + (2.0 * s) * P;
}
__device__ __forceinline__ double nv_ex(double y) {
#pragma clang fp contract(off)
    const double n = rint(y * 1.4426950408889634);
    const double r = y - n * NV_LN2;
    double T = 1.0;
#pragma unroll
    for (int j = 14; j >= 1; --j) T = 1.0 + (r * T) / (double)j;
    return ldexp(T, (int)n);
}
__device__ __forceinline__ double nv_pw(double x, double e) {
#pragma clang fp contract(off)
    return nv_ex(e * nv_lg(x));
}

__global__ __launch_bounds__(NV_T) void nsga_vary_kernel(int Np, int d, const double* __restrict__ X,
                                                         const int32_t* __restrict__ rank, const double* __restrict__ crowd,
                                                         uint64_t seed, const int64_t* __restrict__ generation, double eta_c,
                                                         double p_c, double eta_m, double p_m, double* __restrict__ children,
                                                         int32_t* __restrict__ parents) {
#pragma clang fp contract(off)      // the header's formulas in IEEE operations as written: the host restatement's bits
    const int t = blockIdx.x * NV_T + threadIdx.x;
    if (t >= (Np / 2) * d) return;
    const int q = t / d, v = t - q * d;
    const uint64_t gen = (uint64_t)generation[0], base = (uint64_t)q << 32;
    int par[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        int r[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int x = (int)(philox_uniform(seed, gen, base + (uint64_t)(2 * e + h)) * (double)Np);
            r[h] = x < Np - 1 ? x : Np - 1;
        }
        const int ra = rank[r[0]], rb = rank[r[1]];
        const double ca = crowd[r[0]], cb = crowd[r[1]];
        const bool a_wins = ra < rb || (ra == rb && (ca > cb || (!(cb > ca) && r[0] <= r[1])));
        par[e] = a_wins ? r[0] : r[1];
        if (parents && v == 0) parents[2 * q + e] = par[e];
    }
    const double p0 = X[(int64_t)par[0] * d + v], p1 = X[(int64_t)par[1] * d + v];
    double c[2] = {p0, p1};
    const uint64_t sv = base + 8u + 8u * (uint64_t)v;
    if (philox_uniform(seed, gen, base + 4u) < p_c && philox_uniform(seed, gen, sv) < 0.5) {
        const double w = philox_uniform(seed, gen, sv + 1u);
        const double ex = 1.0 / (eta_c + 1.0);
        const double beta = w <= 0.5 ? nv_pw(2.0 * w, ex) : nv_pw(1.0 / (2.0 * (1.0 - w)), ex);
        c[0] = 0.5 * ((1.0 + beta) * p0 + (1.0 - beta) * p1);
        c[1] = 0.5 * ((1.0 - beta) * p0 + (1.0 + beta) * p1);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        double x = c[e];
        if (philox_uniform(seed, gen, sv + 2u + 2u * (uint64_t)e) < p_m) {
            const double w = philox_uniform(seed, gen, sv + 3u + 2u * (uint64_t)e);
            const double ex = 1.0 / (eta_m + 1.0);
            x += w < 0.5 ? nv_pw(2.0 * w, ex) - 1.0 : 1.0 - nv_pw(2.0 * (1.0 - w), ex);
        }
        children[(int64_t)(2 * q + e) * d + v] = fmin(fmax(x, 0.0), 1.0);
    }
}

extern "C" int mobocmf_nsga_vary(int32_t Np, int32_t d, const double* X, const int32_t* rank, const double* crowd,
                                 uint64_t seed, const int64_t* generation, const mobocmf_nsga_options* opt, double* children,
                                 int32_t* parents, mobocmf_stream_t stream) {
    if (Np < 2 || Np > NS_MAXN || (Np & 1) || d < 1 || d > MOBOCMF_MAX_D || !X || !rank || !crowd || !generation || !children)
        return MOBOCMF_BAD_ARG;
    const mobocmf_nsga_options& o = opt ? *opt : kDefaultNsga;
    if (!nsga_options_ok(o)) return MOBOCMF_BAD_ARG;
    const double p_m = o.p_m == 0.0 ? 1.0 / (double)d : o.p_m;
    const int threads = (Np / 2) * d;
    hipLaunchKernelGGL(nsga_vary_kernel, dim3((unsigned)((threads + NV_T - 1) / NV_T)), dim3(NV_T), 0, (hipStream_t)stream,
                       (int)Np, (int)d, X, rank, crowd, seed, generation, o.eta_c, o.p_c, o.eta_m, p_m, children, parents);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}
