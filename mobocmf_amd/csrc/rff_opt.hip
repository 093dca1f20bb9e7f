// Chain samples with their input gradients, and the constrained multi-start refinement of sampled Pareto optima (the stage of
// MOOP after the grid evaluation: each objective's constrained optimum).  Feature formulas: the header comment of rff.hip.
//
// Both kernels spread ONE evaluation of a chain over many lanes: a refinement is a long serial chain of evaluations of a small
// function (F L cosines), so latency binds, and the features are split over the lanes of NW wavefronts (thread t takes features
// t, t + 64 NW, ...): NW = 1 for the value-and-gradient kernel (a wavefront per point), 8 or 4 for the refinement (a
// workgroup per start; measured at d = 8, F = 500, 16 starts, two constraints: 36 ms with one wavefront per start).  Forward
// mode through the layers:
//
//   df_l/dx = (partial f_l / partial x) + D_l df_{l-1}/dx,     D_l = partial f_l / partial f_{l-1}
//
// Only two scalars per layer cross the lanes (the value and D_l; a butterfly within each wavefront, then the wavefronts'
// partial sums through LDS, added in the order 0, 1, ... by every thread: a fixed order, the same bits everywhere): the gradient
// stays split over the lanes, pg_l = px_l + D_l pg_{l-1} per lane, because the recursion is linear in it, and so does any
// linear combination of several chains' gradients (the merit function of the refinement) -- one d-vector is summed per
// evaluation.
#include "common.h"
#include "rff_desc.h"

#define RO_WAVE 64
#define RO_VG_WAVES 4          // points per workgroup of the value-and-gradient kernel

// sum over the wave, the same bits in every lane (xor butterfly: both partners of a pair add the same two numbers)
__device__ __forceinline__ double ro_wave_sum(double v) {
#pragma unroll
    for (int off = RO_WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, RO_WAVE);
    return v;
}

// v[0, nv) summed over the NW wavefronts that share an evaluation, the same bits in every thread.  red: NW * NV doubles of LDS
// (unused for NW = 1).  Every thread of the workgroup must arrive (two barriers).
template <int NW, int NV>
__device__ __forceinline__ void ro_sum(double (&v)[NV], int nv, double* red, int lane, int wave) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (k < nv) v[k] = ro_wave_sum(v[k]);
    if (NW == 1) return;
    __syncthreads();                                       // the readers of the previous sum are done with red
    if (lane < nv) {
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) mine = lane == k ? v[k] : mine;
        red[wave * NV + lane] = mine;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (k < nv) {
            double t = red[k];
#pragma unroll
            for (int w = 1; w < NW; ++w) t += red[w * NV + k];
            v[k] = t;
        }
}

// Chain `chain` (MOBOCMF_RFF_MAX_LAYERS descriptors) at the point xr (the same in every lane): returns its value (wave-uniform)
// and leaves this thread's share of the input gradient in pg (the gradient = the sum of pg over the NW * 64 threads).  An invalid
// descriptor: NaN, and nothing is read through it.
template <int DB, int NW>
__device__ __forceinline__ double ro_chain(const mobocmf_rff_layer_desc* __restrict__ chain, const double* __restrict__ P,
                                           int64_t plen, int d, const double (&xr)[DB], double (&pg)[DB], double* red,
                                           int lane, int wave) {
    const int t0f = wave * RO_WAVE + lane;                 // this thread's first feature
    double fp = 0.0;
#pragma unroll
    for (int k = 0; k < DB; ++k) pg[k] = 0.0;
    for (int l = 0; l < MOBOCMF_RFF_MAX_LAYERS; ++l) {
        const mobocmf_rff_layer_desc L = chain[l];
        if (L.kind < 0 && l > 0) break;
        if (!rff_desc_ok(L, l, d, plen)) {
            fp = __builtin_nan("");
#pragma unroll
            for (int k = 0; k < DB; ++k) pg[k] = fp;
            break;
        }
        const int F = L.F;
        const double* W1 = P + L.W1;
        const double* b1 = P + L.b1;
        const double* th = P + L.theta;
        double px[DB];
#pragma unroll
        for (int k = 0; k < DB; ++k) px[k] = 0.0;
        double pv[2] = {0.0, 0.0};                         // the value and D_l
        if (L.kind == 0) {
            for (int j = t0f; j < F; j += NW * RO_WAVE) {
                const double* w = W1 + (int64_t)j * d;
                double a1 = b1[j];
#pragma unroll
                for (int k = 0; k < DB; ++k)
                    if (k < d) a1 += w[k] * xr[k];
                double s, c;
                sincos(a1, &s, &c);
                const double t = th[j];
                pv[0] += t * c;
                const double cx = -(t * s);
#pragma unroll
                for (int k = 0; k < DB; ++k)
                    if (k < d) px[k] += cx * w[k];
            }
            ro_sum<NW, 2>(pv, 1, red, lane, wave);
            fp = L.s0 * pv[0];
#pragma unroll
            for (int k = 0; k < DB; ++k) pg[k] = L.s0 * px[k];
        } else {
            const double* Wf = P + L.Wf;
            const double* W2 = P + L.W2;
            const double* b2 = P + L.b2;
            const double s0fp = L.s0 * fp;
            for (int j = t0f; j < F; j += NW * RO_WAVE) {
                const double* w = W1 + (int64_t)j * d;
                const double* v = W2 + (int64_t)j * d;
                double a1 = b1[j], a2 = b2[j];
#pragma unroll
                for (int k = 0; k < DB; ++k)
                    if (k < d) {
                        a1 += w[k] * xr[k];
                        a2 += v[k] * xr[k];
                    }
                const double wf = Wf[j], t0 = th[j], t1 = th[F + j] * L.s1, t2 = th[2 * F + j] * L.s2;
                double s1, c1, sf, cf, s2, c2;
                sincos(a1, &s1, &c1);
                sincos(a1 + wf * fp, &sf, &cf);
                sincos(a2, &s2, &c2);
                pv[0] += t0 * s0fp * c1 + t1 * cf + t2 * c2;
                pv[1] += t0 * L.s0 * c1 - t1 * wf * sf;
                const double cx1 = -(t0 * s0fp * s1 + t1 * sf), cx2 = -(t2 * s2);
#pragma unroll
                for (int k = 0; k < DB; ++k)
                    if (k < d) px[k] += cx1 * w[k] + cx2 * v[k];
            }
            ro_sum<NW, 2>(pv, 2, red, lane, wave);
            fp = pv[0];
            const double D = pv[1];
#pragma unroll
            for (int k = 0; k < DB; ++k) pg[k] = px[k] + D * pg[k];
        }
    }
    return fp;
}

// component `lane` of a vector held whole in every lane (a select chain: no dynamic register index, hence no scratch)
template <int DB>
__device__ __forceinline__ double ro_pick(const double (&v)[DB], int lane) {
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < DB; ++k) r = lane == k ? v[k] : r;
    return r;
}

// ------------------------------------------------------------------ values and gradients of K chains at n points
template <int DB>
__global__ __launch_bounds__(RO_WAVE * RO_VG_WAVES) void rff_value_grad_kernel(int d, int64_t n, const double* __restrict__ x,
                                                                             const double* __restrict__ P, int64_t plen,
                                                                             const mobocmf_rff_layer_desc* __restrict__ desc,
                                                                             double* __restrict__ vals,
                                                                             double* __restrict__ grads) {
    const int lane = threadIdx.x % RO_WAVE, k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * RO_VG_WAVES + threadIdx.x / RO_WAVE;
    if (i >= n) return;                                    // a whole wave leaves: nothing below is shared between waves
    double xr[DB], pg[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c) xr[c] = c < d ? x[i * d + c] : 0.0;
    const double f = ro_chain<DB, 1>(desc + (int64_t)k * MOBOCMF_RFF_MAX_LAYERS, P, plen, d, xr, pg, nullptr, lane, 0);
    ro_sum<1, DB>(pg, d, nullptr, lane, 0);
    const int64_t o = (int64_t)k * n + i;
    if (lane == 0) vals[o] = f;
    if (lane < d) grads[o * d + lane] = ro_pick<DB>(pg, lane);
}

extern "C" int mobocmf_rff_chains_value_grad(int32_t K, int32_t d, int64_t n, const double* x, const double* params,
                                             int64_t params_len, const mobocmf_rff_layer_desc* desc, double* vals,
                                             double* grads, mobocmf_stream_t stream) {
    if (K < 1 || K > 65535 || d < 1 || d > MOBOCMF_MAX_D || n < 1 || n > (int64_t)RO_VG_WAVES * 0x7fffffff || params_len < 1 ||
        !x || !params || !desc || !vals || !grads)
        return MOBOCMF_BAD_ARG;
    const dim3 grid((unsigned)((n + RO_VG_WAVES - 1) / RO_VG_WAVES), (unsigned)K), block(RO_WAVE * RO_VG_WAVES);
    hipStream_t s = (hipStream_t)stream;
#define ROVG_GO(D) hipLaunchKernelGGL((rff_value_grad_kernel<D>), grid, block, 0, s, d, n, x, params, params_len, desc, vals, grads)
    if (d <= 2) ROVG_GO(2); else if (d <= 8) ROVG_GO(8); else ROVG_GO(32);
#undef ROVG_GO
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

// ------------------------------------------------------------------ multi-start constrained refinement
static const mobocmf_rff_refine_options kDefaultRefine = {sizeof(mobocmf_rff_refine_options), 8, 30, 6, 4, 1, 0.05, 0.25, 2.0,
                                                          10.0, 4.0, 1e-4, 1e-9};

extern "C" int mobocmf_rff_refine_options_init(mobocmf_rff_refine_options* opt) {
    if (!opt) return MOBOCMF_BAD_ARG;
    *opt = kDefaultRefine;
    return MOBOCMF_OK;
}

static bool refine_options_ok(const mobocmf_rff_refine_options& o) {
    return o.struct_size == sizeof(mobocmf_rff_refine_options) && o.outer >= 1 && o.outer <= 64 && o.inner >= 1 &&
           o.inner <= 1024 && o.backtracks >= 0 && o.backtracks <= 32 && o.restore >= 0 && o.restore <= 32 && (o.recentre == 0 || o.recentre == 1) && o.step0 > 0.0 &&
           o.step0 <= 1e6 && o.step_shrink > 0.0 && o.step_shrink < 1.0 && o.step_grow >= 1.0 && o.step_grow <= 1e3 &&
           o.rho0 > 0.0 && o.rho0 <= 1e12 && o.rho_growth >= 1.0 && o.rho_growth <= 1e3 && o.armijo > 0.0 && o.armijo < 1.0 &&
           o.restore_margin >= 0.0 && o.restore_margin <= 1.0;
}

struct ro_problems {          // the problem table, a launch argument
    int32_t obj[MOBOCMF_REFINE_MAX_PROBLEMS], con_off[MOBOCMF_REFINE_MAX_PROBLEMS], con_cnt[MOBOCMF_REFINE_MAX_PROBLEMS];
};

#define RO_STEP_MAX 1e6
#define RO_STEP_MIN 1e-12

// One evaluation of problem p at xt (whole in every lane).  mode 0: the merit f + sum_i (max(0, lam_i - rho s_i)^2 - lam_i^2) /
// (2 rho) and its gradient; mode 1: V = 1/2 sum_i max(0, margin - s_i)^2 and its gradient.  The slacks go to slk (LDS).  f, the
// smallest slack, `feas` (f finite, every slack >= 0) and the merit are wave-uniform; gl = component `lane` of the gradient.
template <int DB, int NW>
__device__ __forceinline__ void ro_eval(int mode, int d, int K, int obj, int C, const int32_t* __restrict__ con,
                                        const double* __restrict__ thr, const double* __restrict__ P, int64_t plen,
                                        const mobocmf_rff_layer_desc* __restrict__ desc, const double (&xt)[DB],
                                        const double* lam, double* slk, double* red, double rho, double margin, int lane,
                                        int wave, double& f,
                                        double& smin, bool& feas, double& merit, double& gl) {
    double pg[DB], mg[DB];
    f = ro_chain<DB, NW>(desc + (int64_t)obj * MOBOCMF_RFF_MAX_LAYERS, P, plen, d, xt, pg, red, lane, wave);
#pragma unroll
    for (int k = 0; k < DB; ++k) mg[k] = mode == 0 ? pg[k] : 0.0;
    merit = mode == 0 ? f : 0.0;
    feas = f - f == 0.0;
    smin = __builtin_inf();
    for (int i = 0; i < C; ++i) {
        const int ci = con[i];
        double s = __builtin_nan("");
        if (ci >= 0 && ci < K) s = ro_chain<DB, NW>(desc + (int64_t)ci * MOBOCMF_RFF_MAX_LAYERS, P, plen, d, xt, pg, red, lane, wave) - thr[i];
        slk[i] = s;                                       // every lane stores the same value
        feas = feas && s >= 0.0;
        if (!(s >= smin)) smin = s;
        double coef = 0.0;
        if (mode == 0) {
            const double lm = lam[i], t = lm - rho * s;
            if (!(t <= 0.0)) {                            // NaN slack: the merit goes NaN and no trial is accepted
                merit += (t * t - lm * lm) / (2.0 * rho);
                coef = -t;
            } else {
                merit -= lm * lm / (2.0 * rho);
            }
        } else {
            const double v = margin - s;
            if (!(v <= 0.0)) {
                merit += 0.5 * v * v;
                coef = -v;
            }
        }
        if (coef != 0.0) {
#pragma unroll
            for (int k = 0; k < DB; ++k) mg[k] += coef * pg[k];
        }
    }
    ro_sum<NW, DB>(mg, d, red, lane, wave);
    gl = ro_pick<DB>(mg, lane);
}

// One workgroup of NW wavefronts = start r of problem p.  The iterate, its gradient, the trial point and the best point live
// one component per lane (xl, gl, xtl, bxl: lane k < d of EVERY wavefront, zero elsewhere; the wavefronts run the same
// optimiser on the same numbers, so every branch and barrier below is uniform over the workgroup); only the trial point is
// also held whole in every lane for the evaluation.
template <int DB, int NW>
__global__ __launch_bounds__(RO_WAVE * NW) void rff_refine_kernel(int d, int R, int K, ro_problems pr,
                                                             const int32_t* __restrict__ con_all,
                                                             const double* __restrict__ thr_all,
                                                             const double* __restrict__ x0, const double* __restrict__ P,
                                                             int64_t plen, const mobocmf_rff_layer_desc* __restrict__ desc,
                                                             mobocmf_rff_refine_options o, double* __restrict__ xs,
                                                             double* __restrict__ fs, double* __restrict__ slack_min) {
    __shared__ double lam[MOBOCMF_REFINE_MAX_CON], slk[MOBOCMF_REFINE_MAX_CON], slk_x[MOBOCMF_REFINE_MAX_CON];
    __shared__ double red[NW * DB];
    const int lane = threadIdx.x % RO_WAVE, wave = threadIdx.x / RO_WAVE, r = blockIdx.x, p = blockIdx.y;
    const int tid = threadIdx.x;
    const int obj = pr.obj[p], C = pr.con_cnt[p];
    const int32_t* con = con_all + pr.con_off[p];
    const double* thr = thr_all + pr.con_off[p];
    const int64_t sr = (int64_t)p * R + r;
    const bool comp = lane < d;
    double* xout = xs + sr * d;

    const double x0l = comp ? x0[sr * d + lane] : 0.0;
    if (__any(x0l != x0l)) {                               // a NaN start is not iterated (every wavefront sees the same start)
        if (comp && wave == 0) xout[lane] = x0l;
        if (tid == 0) fs[sr] = slack_min[sr] = __builtin_nan("");
        return;
    }
    auto clamp = [](double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); };
    double xl = clamp(x0l), gl = 0.0, xtl = xl, bxl = xl;
    if (tid < C) lam[tid] = 0.0;
    __syncthreads();

    double xt[DB];
    auto spread = [&](double vl) {                         // xt = the vector held one component per lane
#pragma unroll
        for (int k = 0; k < DB; ++k) xt[k] = k < d ? __shfl(vl, k, RO_WAVE) : 0.0;
    };
    bool has_best = false;
    double best_f = 0.0, best_smin = 0.0;
    auto consider = [&](double vl, double f, double smin, bool feas) {   // keeps the best feasible point evaluated
        if (feas && (!has_best || f < best_f)) {
            has_best = true;
            best_f = f;
            best_smin = smin;
            bxl = vl;
        }
    };

    double f = 0.0, smin = 0.0, M = 0.0, alpha = o.step0, rho = o.rho0, vprev = __builtin_inf();
    bool feas = false;
    for (int outer = 0; outer < o.outer; ++outer) {
        spread(xl);                                        // the merit of this round's multipliers at the iterate
        ro_eval<DB, NW>(0, d, K, obj, C, con, thr, P, plen, desc, xt, lam, slk, red, rho, 0.0, lane, wave, f, smin, feas, M, gl);
        consider(xl, f, smin, feas);
        __syncthreads();
        if (tid < C) slk_x[tid] = slk[tid];
        __syncthreads();
        for (int inner = 0; inner < o.inner; ++inner) {
            double a = alpha, ft = 0.0, smt = 0.0, Mt = 0.0, gtl = 0.0, dxl = 0.0;
            bool feast = false, accepted = false, stationary = false;
            for (int bt = 0; bt <= o.backtracks; ++bt) {
                xtl = comp ? clamp(xl - a * gl) : 0.0;
                dxl = xtl - xl;
                const double gd = ro_wave_sum(gl * dxl);
                if (!(gd < 0.0)) {                         // the projected gradient vanishes (or the merit is NaN)
                    stationary = true;
                    break;
                }
                spread(xtl);
                __syncthreads();                           // slk: the copy to slk_x of the previous accepted step is done
                ro_eval<DB, NW>(0, d, K, obj, C, con, thr, P, plen, desc, xt, lam, slk, red, rho, 0.0, lane, wave, ft, smt, feast, Mt,
                                gtl);
                consider(xtl, ft, smt, feast);
                if (Mt <= M + o.armijo * gd) {
                    accepted = true;
                    break;
                }
                a *= o.step_shrink;
            }
            if (stationary) break;
            if (!accepted) {
                alpha = a > RO_STEP_MIN ? a : RO_STEP_MIN;
                continue;
            }
            const double sy = ro_wave_sum(dxl * (gtl - gl)), ss = ro_wave_sum(dxl * dxl);
            alpha = sy > 0.0 ? ss / sy : a * o.step_grow;  // Barzilai-Borwein step where the curvature along the step is positive
            alpha = alpha > RO_STEP_MAX ? RO_STEP_MAX : (alpha < RO_STEP_MIN ? RO_STEP_MIN : alpha);
            xl = xtl, gl = gtl, f = ft, smin = smt, M = Mt, feas = feast;
            __syncthreads();
            if (tid < C) slk_x[tid] = slk[tid];
            __syncthreads();
        }
        __syncthreads();
        if (tid < C) {
            const double t = lam[tid] - rho * slk_x[tid];
            lam[tid] = t > 0.0 ? t : 0.0;
        }
        __syncthreads();
        const double viol = smin < 0.0 ? -smin : 0.0;
        if (viol > 0.25 * vprev) {
            rho *= o.rho_growth;
            // the round did not approach the feasible set (the iterate may sit in another basin of a nonconvex constraint):
            // the next one starts from the best feasible point so far
            if (o.recentre && has_best && outer + 1 < o.outer) xl = bxl;
        }
        vprev = viol;
    }
    // restoration: an iterate that ends outside the feasible set is walked back along the violated constraints' gradients
    if (C > 0 && !feas) {
        for (int it = 0; it <= o.restore; ++it) {
            double V = 0.0;
            spread(xl);
            __syncthreads();
            ro_eval<DB, NW>(1, d, K, obj, C, con, thr, P, plen, desc, xt, lam, slk, red, rho, o.restore_margin, lane, wave, f, smin,
                            feas, V, gl);
            consider(xl, f, smin, feas);
            if (it == o.restore || !(V > 0.0)) break;
            const double gg = ro_wave_sum(gl * gl);
            if (!(gg > 0.0)) break;
            xl = comp ? clamp(xl - (2.0 * V / gg) * gl) : 0.0;
        }
    }
    if (comp && wave == 0) xout[lane] = has_best ? bxl : xl;
    if (tid == 0) {
        fs[sr] = has_best ? best_f : __builtin_nan("");
        slack_min[sr] = has_best ? best_smin : smin;
    }
}

// the best start result of every problem: one thread per problem, starts in the order r = 0, 1, ...
__global__ void rff_refine_best_kernel(int P, int R, int d, const double* __restrict__ x0, const double* __restrict__ xs,
                                       const double* __restrict__ fs, double* __restrict__ x_best, double* __restrict__ f_best,
                                       int32_t* __restrict__ start_best, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int best = -1;
    double fb = __builtin_nan("");
    for (int r = 0; r < R; ++r) {
        const double f = fs[(int64_t)p * R + r];
        if (f == f && (best < 0 || f < fb)) best = r, fb = f;
    }
    f_best[p] = fb;
    start_best[p] = best;
    bool same = true;
    for (int k = 0; k < d; ++k) {
        double v = __builtin_nan("");
        if (best >= 0) {
            const int64_t e = ((int64_t)p * R + best) * d + k;
            const double s = x0[e];
            v = xs[e];
            same = same && v == (s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s));
        }
        x_best[(int64_t)p * d + k] = v;
    }
    status[p] = best < 0 ? 2 : (same ? 1 : 0);
}

extern "C" int mobocmf_rff_refine(int32_t P, int32_t R, int32_t d, int32_t K, const int32_t* obj, const int32_t* con_off,
                                  const int32_t* con_cnt, int32_t n_con, const int32_t* con, const double* thr,
                                  const double* x0, const double* params, int64_t params_len,
                                  const mobocmf_rff_layer_desc* desc, const mobocmf_rff_refine_options* opt, double* xs,
                                  double* fs, double* slack_min, double* x_best, double* f_best, int32_t* start_best,
                                  int32_t* status, mobocmf_stream_t stream) {
    if (P < 1 || P > MOBOCMF_REFINE_MAX_PROBLEMS || R < 1 || R > 65535 || d < 1 || d > MOBOCMF_MAX_D || K < 1 || n_con < 0 ||
        params_len < 1 || !obj || !con_off || !con_cnt || !x0 || !params || !desc || !xs || !fs || !slack_min || !x_best ||
        !f_best || !start_best || !status || (n_con > 0 && (!con || !thr)))
        return MOBOCMF_BAD_ARG;
    const mobocmf_rff_refine_options o = opt ? *opt : kDefaultRefine;
    if (!refine_options_ok(o)) return MOBOCMF_BAD_ARG;
    ro_problems pr = {};
    for (int p = 0; p < P; ++p) {
        if (obj[p] < 0 || obj[p] >= K || con_cnt[p] < 0 || con_cnt[p] > MOBOCMF_REFINE_MAX_CON || con_off[p] < 0 ||
            (int64_t)con_off[p] + con_cnt[p] > n_con)
            return MOBOCMF_BAD_ARG;
        pr.obj[p] = obj[p], pr.con_off[p] = con_off[p], pr.con_cnt[p] = con_cnt[p];
    }
    const dim3 grid((unsigned)R, (unsigned)P);
    hipStream_t s = (hipStream_t)stream;
#define ROR_GO(D, NW) hipLaunchKernelGGL((rff_refine_kernel<D, NW>), grid, dim3(RO_WAVE * NW), 0, s, d, R, K, pr, con, thr, x0, params, params_len, desc, o, xs, fs, slack_min)
    if (d <= 2) ROR_GO(2, 8); else if (d <= 8) ROR_GO(8, 8); else ROR_GO(32, 4);       // 4: one wavefront per SIMD, 512 registers each
#undef ROR_GO
    if (hipGetLastError() != hipSuccess) return MOBOCMF_HIP_ERROR;
    hipLaunchKernelGGL(rff_refine_best_kernel, dim3(1), dim3(MOBOCMF_REFINE_MAX_PROBLEMS), 0, s, P, R, d, x0, xs, fs, x_best,
                       f_best, start_best, status);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}
