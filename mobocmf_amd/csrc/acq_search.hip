// The device side of the acquisition search (JESMOC_MFDGP(search="device"), util/acq_search.py): what stands between the two
// one-launch model evaluations of an iterate -- the JES value of every test point from the predict group's raw moments with its
// gradient w.r.t. those moments and the best-iterate tracking, the projected Adam ascent step on the iterate -- and the
// selection of the k best of n values (the restarts among the raw candidates, the winner among the restarts).  The MES value
// of the exact-GP baselines (MESMOC_MFGP(search="device"), mobocmf_mes_group_forward) stands in the JES position of the same chain.
//
// All of them are latency-bound glue on a few hundred to a few thousand doubles: each is ONE launch, has no atomics and sums in a
// fixed order (two calls on the same inputs are bitwise equal), reads nothing on the host and keeps no state: capturable.
#include "common.h"

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR)
#define AS_BLOCK 256
#define AS_WAVE 64

namespace {

// v of one model at test point t (TinyPredictGroup.acquisition_moments): the moments over the S samples of mean_s, var_s + tau;
// mbar: the mean over the samples (what the seeds need).
__device__ __forceinline__ double as_model_v(const double* __restrict__ mean, const double* __restrict__ var, double tau,
                                             int64_t c0, int S, double* mbar) {
    if (S == 1) {
        *mbar = mean[c0];
        return var[c0] + tau;
    }
    double sm = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double m = mean[c0 + s];
        sm += m;
        s2 += (var[c0 + s] + tau) + m * m;
    }
    sm /= S;
    *mbar = sm;
    return s2 / S - sm * sm;
}

enum { JES_COUPLED = 0, JES_ALL_BOXES = 1, JES_SELECTED_BOX = 2 };

// Black-box p's term from the parked terms of its K conditioned models (u = p (1 + K): its unconditioned model): the k-sum in
// the order of k, then the product with 1 / K, ROUNDED -- nothing is fused onto it, here or where the caller adds it.
__device__ __forceinline__ double as_box_term(const double* s_term, int u, int K) {
#pragma clang fp contract(off)
    const double inv_k = 1.0 / K;
    double box = s_term[u + 1];
    for (int k = 2; k <= K; ++k) box += s_term[u + k];
    return inv_k * box;
}

// JES averaged over K sampled Pareto sets: black-box p owns the 1 + K consecutive models p (1 + K) (unconditioned) and
// p (1 + K) + 1 + k (conditioned on sample k).  ONE wavefront per test point (the replayed iterate has T = 5: one thread per test
// point would leave five lanes looping over every model and sample): lane m forms v and mbar of model m and parks log v in
// LDS; the lane of a conditioned model forms its term and whether the clamp passes.  Who sums and what is written is the MODE:
//   JES_COUPLED (mobocmf_jes_mc_group_forward): lane 0 adds the box terms from 0.0 in the order of p into acq[t] and tracks; every
//   lane writes its own model's seeds.  At K = 1 (mobocmf_jes_group_forward) 1.0 * the single term and 0.5 / (1 * v) are exact:
//   the pair expression 0.5 max(log v_u - log v_c, 0) of the public header, bit for bit;
//   JES_ALL_BOXES (mobocmf_jes_mc_box_forward, box_of_point NULL): the lane of the unconditioned model of box p writes
//   acq[p acq_ld + t] = term_p[t]; no seeds, no tracking (the host refuses them);
//   JES_SELECTED_BOX (the replayed decoupled iterate): b = box_of_point[t]; the lane of box b's unconditioned model writes acq[t]
//   and tracks; the 1 + K models of box b get the coupled seeds (a model's seeds depend on its own box only), EVERY other
//   model's seeds at the columns of t are written as 0.0 (the STEP_INPUT_GRADIENTS launch that follows reads them all);
//   b outside [0, n_boxes): acq[t] = NaN, every seed 0.0, nothing tracked.
// The box term is one expression (as_box_term) and the coupled sum adds it rounded: P1 - P3 of the public header hold by
// construction.  No atomics, static LDS only, every thread reaches every barrier (the grid is T workgroups).
template <int MODE>
__global__ void __launch_bounds__(AS_WAVE)
jes_kernel(const double* __restrict__ moments, const double* __restrict__ noise, int n_boxes, int K, int T, int S,
           double* __restrict__ acq, double* __restrict__ seeds, const double* __restrict__ x, int d,
           double* __restrict__ best_v, double* __restrict__ best_x, const int* __restrict__ box_of_point, int acq_ld) {
    __shared__ double s_lv[AS_WAVE], s_term[AS_WAVE];
    __shared__ int s_pass[AS_WAVE], s_win;
    const int t = blockIdx.x, m = threadIdx.x;
    const int stride = 1 + K, n_models = n_boxes * stride;
    const int64_t ncol = (int64_t)T * S, c0 = (int64_t)t * S;
    const bool mine = m < n_models;
    const int p = m / stride, k1 = m % stride;      // k1 = 0: the unconditioned model of box p; else sample k1 - 1
    const int b = MODE == JES_SELECTED_BOX ? box_of_point[t] : -1;
    const double* mu = moments + (int64_t)m * 2 * ncol;
    double v = 0.0, bar = 0.0;
    if (mine) {
        v = as_model_v(mu, mu + ncol, noise[m], c0, S, &bar);
        s_lv[m] = log(v);
    }
    __syncthreads();
    if (mine && k1 > 0) {
        const double diff = s_lv[p * stride] - s_lv[m];
        s_term[m] = 0.5 * (diff < 0.0 ? 0.0 : diff);      // (a NaN stays a NaN, as torch.clamp)
        s_pass[m] = diff >= 0.0;                           // torch.clamp's backward (a NaN passes nothing)
    }
    __syncthreads();
    if (MODE == JES_COUPLED ? m == 0 : mine && k1 == 0 && (MODE == JES_ALL_BOXES || p == b)) {
#pragma clang fp contract(off)      // (1/K) * (the box's sum) is rounded before it is added, as the restatement has it
        double a;
        if constexpr (MODE == JES_COUPLED) {
            a = 0.0;
            for (int q = 0; q < n_boxes; ++q) a += as_box_term(s_term, q * stride, K);
        } else {
            a = as_box_term(s_term, m, K);
        }
        if constexpr (MODE == JES_ALL_BOXES) {
            acq[(int64_t)p * acq_ld + t] = a;
        } else {
            acq[t] = a;
            int win = 0;
            if (best_v && a > best_v[t]) {      // strict; a NaN never wins
                best_v[t] = a;
                win = 1;
            }
            s_win = win;      // (whoever writes acq[t] says whether it won: one lane per test point)
        }
    }
    if (MODE == JES_SELECTED_BOX && m == 0 && (b < 0 || b >= n_boxes)) {      // (no lane above has p == b)
        acq[t] = __builtin_nan("");
        s_win = 0;
    }
    if (MODE != JES_ALL_BOXES && seeds && mine) {
        double* sm = seeds + (int64_t)m * 2 * ncol;
        if (MODE == JES_COUPLED || p == b) {
            double g;
            if (k1 > 0) {
                g = s_pass[m] ? -0.5 / (K * v) : 0.0;
            } else {
                int cnt = 0;
                for (int k = 1; k <= K; ++k) cnt += s_pass[m + k];
                g = cnt > 0 ? cnt * (0.5 / (K * v)) : 0.0;
            }
            const double inv_s = 1.0 / S;
            for (int s = 0; s < S; ++s) {
                sm[c0 + s] = g * (2.0 * (mu[c0 + s] - bar) / S);
                sm[ncol + c0 + s] = g * inv_s;
            }
        } else {
            for (int s = 0; s < S; ++s) {      // not g = 0 times the expression above: a NaN moment of another box stays out
                sm[c0 + s] = 0.0;
                sm[ncol + c0 + s] = 0.0;
            }
        }
    }
    __syncthreads();
    if (MODE != JES_ALL_BOXES && s_win && m < d) best_x[(int64_t)t * d + m] = x[(int64_t)t * d + m];
}

// MES on the exact-GP baselines (mobocmf_mes_group_forward): the JES kernel's shape -- ONE wavefront per test point, lane m forms
// the value of model m (an objective's truncated-Gaussian entropy term, a constraint's probability of feasibility) and its
// derivative w.r.t. that model's own mean and variance, the values meet in LDS, lane 0 adds the terms in the order of p,
// multiplies the probabilities in the order of c, writes acq[t] and tracks; every lane then scales its own derivative by what
// the product rule leaves for it, formed from the parked values in the same orders (a constraint: the product over the OTHER
// constraints).  Nothing is fused: the value is the host statement operation for operation.
__global__ void __launch_bounds__(AS_WAVE)
mes_kernel(const double* __restrict__ moments, const double* __restrict__ noise, const double* __restrict__ best, int n_obj,
           int n_con, int T, double* __restrict__ acq, double* __restrict__ seeds, const double* __restrict__ x, int d,
           double* __restrict__ best_v, double* __restrict__ best_x) {
#pragma clang fp contract(off)
    __shared__ double s_val[AS_WAVE];
    __shared__ int s_win;
    constexpr double E = 1.1920928955078125e-07, SQRT2 = 1.4142135623730951, SQRT_2PI = 2.5066282746310002;
    const int t = blockIdx.x, m = threadIdx.x, n_models = n_obj + n_con;
    const bool mine = m < n_models, con = m >= n_obj;
    double gm = 0.0, gv = 0.0;      // d (this model's value) / d (its mean, its variance)
    if (mine) {
        const double mean = moments[(int64_t)m * 2 * T + t], var = moments[(int64_t)m * 2 * T + T + t];
        const double s = sqrt(var), z = (best[m] - mean) / s;
        const double Phi = 0.5 * (1.0 + erf(z / SQRT2));
        const double pdf = exp(-0.5 * z * z) / SQRT_2PI;
        const double dz_dm = -1.0 / s, dz_dv = -0.5 * z / var;
        double val;
        if (con) {
            val = 1.0 - Phi;
            gm = -pdf * dz_dm;
            gv = -pdf * dz_dv;
        } else {
            const double cmax = 1.0 - E, tau = noise[m];
            const bool bind = Phi > cmax;                    // (a NaN stays a NaN, as torch.clamp)
            const double cdf = bind ? cmax : Phi;
            const double r = pdf / (1.0 - cdf);
            const double u = 1.0 + (z - r) * r;
            const bool floor = u < E;
            const double g = floor ? E : u;
            const double vt = var * g + tau;
            const double diff = 0.5 * log(var + tau) - 0.5 * log(vt);
            val = diff < 0.0 ? 0.0 : diff;
            if (seeds && diff >= 0.0) {                      // torch.clamp's backward: equality passes, a NaN passes nothing
                const double dr_dz = -z * r + (bind ? 0.0 : r * r);      // under the binding clamp the cdf is a constant
                const double du_dz = floor ? 0.0 : r + (z - 2.0 * r) * dr_dz;
                const double dlogvt_dz = 0.5 / vt * var * du_dz;
                gm = -(dlogvt_dz * dz_dm);
                gv = 0.5 / (var + tau) - 0.5 / vt * g - dlogvt_dz * dz_dv;
            }
        }
        s_val[m] = val;
    }
    __syncthreads();
    if (m == 0) {
        double sum = 0.0, feas = 1.0;
        for (int p = 0; p < n_obj; ++p) sum += s_val[p];
        for (int c = 0; c < n_con; ++c) feas *= s_val[n_obj + c];
        const double a = sum * feas;
        acq[t] = a;
        int win = 0;
        if (best_v && a > best_v[t]) {      // strict; a NaN never wins
            best_v[t] = a;
            win = 1;
        }
        s_win = win;
    }
    if (seeds && mine) {
        double scale = 1.0;      // d acq / d (this model's value)
        if (con) {
            double sum = 0.0;
            for (int p = 0; p < n_obj; ++p) sum += s_val[p];
            for (int c = 0; c < n_con; ++c)
                if (n_obj + c != m) scale *= s_val[n_obj + c];
            scale = sum * scale;
        } else {
            for (int c = 0; c < n_con; ++c) scale *= s_val[n_obj + c];
        }
        seeds[(int64_t)m * 2 * T + t] = scale * gm;
        seeds[(int64_t)m * 2 * T + T + t] = scale * gv;
    }
    __syncthreads();
    if (s_win && m < d) best_x[(int64_t)t * d + m] = x[(int64_t)t * d + m];
}

// One workgroup.  Every thread reads the step count, the workgroup meets, thread 0 advances it: no trailing launch.
__global__ void __launch_bounds__(AS_BLOCK)
ascent_adam_kernel(double* __restrict__ x, const double* __restrict__ gx, int n_models, int n, int d,
                   const double* __restrict__ lo, const double* __restrict__ hi, double* __restrict__ m,
                   double* __restrict__ v, double lr, double b1, double b2, double eps, int64_t* steps_done) {
#pragma clang fp contract(off)      // (nothing below is fused but what is written as a fused operation)
    const int64_t step = steps_done[0] + 1;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2s = sqrt(1.0 - pow(b2, (double)step));
    for (int i = threadIdx.x; i < n; i += AS_BLOCK) {
        double s = gx[i];
        for (int k = 1; k < n_models; ++k) s += gx[(int64_t)k * n + i];
        // From here on the arithmetic of adam_multi_kernel (elementwise.hip), bit for bit.  Which product of a sum of two the
        // compiler fuses is its choice per kernel; the fused operations are therefore spelled out here as that kernel has
        // them (m: the gradient's product fused onto the rounded b1 m; v: g * round((1 - b2) g) fused onto the rounded b2 v).
        const double gi = -s;
        const double mi = __builtin_fma(1.0 - b1, gi, b1 * m[i]);
        const double vi = __builtin_fma(gi, (1.0 - b2) * gi, b2 * v[i]);
        m[i] = mi;
        v[i] = vi;
        double xi = x[i];
        xi -= (lr / bc1) * mi / (sqrt(vi) / bc2s + eps);
        const double l = lo[i % d], h = hi[i % d];
        xi = xi < l ? l : xi;           // (a NaN stays a NaN, as torch.clamp_)
        xi = xi > h ? h : xi;
        x[i] = xi;
    }
    __syncthreads();
    if (threadIdx.x == 0) steps_done[0] = step;
}

// The order of the selection: larger value first, ties to the lower index, NaN after every number; index -1: no element.
__device__ __forceinline__ bool as_before(double va, int ia, double vb, int ib) {
    if (ia < 0 || ib < 0) return ib < 0 && ia >= 0;
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return nb;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}

// One workgroup, k rounds: every thread finds the first element (in the order above) of its share that comes strictly after
// the element of the previous round, a butterfly picks the wavefront's, the wavefronts' four meet in LDS.
__global__ void __launch_bounds__(AS_BLOCK)
select_topk_kernel(const double* __restrict__ vals, int n, int k, const double* __restrict__ x, int d,
                   double* __restrict__ out_vals, int64_t* __restrict__ out_idx, double* __restrict__ out_x) {
    __shared__ double red_v[AS_BLOCK / AS_WAVE];
    __shared__ int red_i[AS_BLOCK / AS_WAVE];
    const int lane = threadIdx.x & (AS_WAVE - 1), wave = threadIdx.x / AS_WAVE;
    double last_v = 0.0;
    int last_i = -1;
    for (int r = 0; r < k; ++r) {
        double bv = 0.0;
        int bi = -1;
        for (int i = threadIdx.x; i < n; i += AS_BLOCK) {
            const double vi = vals[i];
            if (last_i >= 0 && !as_before(last_v, last_i, vi, i)) continue;      // picked in an earlier round
            if (as_before(vi, i, bv, bi)) { bv = vi; bi = i; }
        }
#pragma unroll
        for (int off = AS_WAVE / 2; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, AS_WAVE);
            const int oi = __shfl_xor(bi, off, AS_WAVE);
            if (as_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        __syncthreads();                 // the readers of the previous round are done with red
        if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
        __syncthreads();
        bv = red_v[0];
        bi = red_i[0];
#pragma unroll
        for (int w = 1; w < AS_BLOCK / AS_WAVE; ++w)
            if (as_before(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
        last_v = bv;
        last_i = bi;                     // (k <= n: every round finds one)
        if (threadIdx.x == 0) { out_vals[r] = bv; out_idx[r] = bi; }
        if (out_x && bi >= 0 && (int)threadIdx.x < d) out_x[(int64_t)r * d + threadIdx.x] = x[(int64_t)bi * d + threadIdx.x];
    }
}

// The checks and the launch of the three JES entry points (the per-box one adds what the all-box mode refuses).
int jes_launch(int mode, const double* moments, const double* noise, int32_t n_boxes, int32_t K, int32_t T, int32_t S,
               const int32_t* box_of_point, double* acq, int32_t acq_ld, int32_t want_seeds, double* seeds, int32_t track,
               const double* x, int32_t d, double* best_v, double* best_x, mobocmf_stream_t stream) {
    if (!moments || !noise || !acq || n_boxes < 1 || K < 1 || T < 1 || S < 1) return MOBOCMF_BAD_ARG;
    if ((int64_t)n_boxes * (1 + (int64_t)K) > 2 * MOBOCMF_ACQ_MAX_PAIRS) return MOBOCMF_BAD_ARG;      // one lane per model
    if ((int64_t)T * S > MOBOCMF_ACQ_MAX_COLUMNS) return MOBOCMF_BAD_ARG;
    if (want_seeds < 0 || want_seeds > 1 || track < 0 || track > 1 || (want_seeds && !seeds)) return MOBOCMF_BAD_ARG;
    if (track && (!x || !best_v || !best_x || d < 1 || d > MOBOCMF_MAX_D)) return MOBOCMF_BAD_ARG;
    if (mode == JES_ALL_BOXES && (acq_ld < T || want_seeds || track)) return MOBOCMF_BAD_ARG;
    static_assert(2 * MOBOCMF_ACQ_MAX_PAIRS <= AS_WAVE && MOBOCMF_MAX_D <= AS_WAVE, "one lane per model, one per coordinate");
    const auto kernel = mode == JES_COUPLED ? jes_kernel<JES_COUPLED>
                                            : mode == JES_ALL_BOXES ? jes_kernel<JES_ALL_BOXES> : jes_kernel<JES_SELECTED_BOX>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)T), dim3(AS_WAVE), 0, (hipStream_t)stream, moments, noise, n_boxes, K, T, S,
                       acq, want_seeds ? seeds : (double*)nullptr, x, track ? d : 0, track ? best_v : (double*)nullptr, best_x,
                       (const int*)box_of_point, acq_ld);
    return CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int mobocmf_jes_mc_group_forward(const double* moments, const double* noise, int32_t n_boxes, int32_t K, int32_t T, int32_t S,
                                 double* acq, int32_t want_seeds, double* seeds, int32_t track, const double* x, int32_t d,
                                 double* best_v, double* best_x, mobocmf_stream_t stream) {
    return jes_launch(JES_COUPLED, moments, noise, n_boxes, K, T, S, nullptr, acq, 0, want_seeds, seeds, track, x, d, best_v,
                      best_x, stream);
}

// The pair form (model 2p unconditioned, 2p + 1 conditioned): K = 1 of the above, whose checks are then this entry point's own
// (n_pairs in 1 .. MOBOCMF_ACQ_MAX_PAIRS is n_boxes (1 + K) in 2 .. 2 MOBOCMF_ACQ_MAX_PAIRS).
int mobocmf_jes_group_forward(const double* moments, const double* noise, int32_t n_pairs, int32_t T, int32_t S,
                              double* acq, int32_t want_seeds, double* seeds, int32_t track, const double* x, int32_t d,
                              double* best_v, double* best_x, mobocmf_stream_t stream) {
    return jes_launch(JES_COUPLED, moments, noise, n_pairs, 1, T, S, nullptr, acq, 0, want_seeds, seeds, track, x, d, best_v,
                      best_x, stream);
}

// Per black-box: the all-box mode (box_of_point NULL) writes values alone.
int mobocmf_jes_mc_box_forward(const double* moments, const double* noise, int32_t n_boxes, int32_t K, int32_t T, int32_t S,
                               const int32_t* box_of_point, double* acq, int32_t acq_ld, int32_t want_seeds, double* seeds,
                               int32_t track, const double* x, int32_t d, double* best_v, double* best_x,
                               mobocmf_stream_t stream) {
    return jes_launch(box_of_point ? JES_SELECTED_BOX : JES_ALL_BOXES, moments, noise, n_boxes, K, T, S, box_of_point, acq, acq_ld,
                      want_seeds, seeds, track, x, d, best_v, best_x, stream);
}

int mobocmf_mes_group_forward(const double* moments, const double* noise, const double* best, int32_t n_obj, int32_t n_con,
                              int32_t T, double* acq, int32_t want_seeds, double* seeds, int32_t track, const double* x,
                              int32_t d, double* best_v, double* best_x, mobocmf_stream_t stream) {
    if (!moments || !noise || !best || !acq || n_obj < 1 || n_con < 0 || T < 1 || T > MOBOCMF_ACQ_MAX_COLUMNS) return MOBOCMF_BAD_ARG;
    if ((int64_t)n_obj + n_con > 2 * MOBOCMF_ACQ_MAX_PAIRS) return MOBOCMF_BAD_ARG;      // one lane per model
    if (want_seeds < 0 || want_seeds > 1 || track < 0 || track > 1 || (want_seeds && !seeds)) return MOBOCMF_BAD_ARG;
    if (track && (!x || !best_v || !best_x || d < 1 || d > MOBOCMF_MAX_D)) return MOBOCMF_BAD_ARG;
    hipLaunchKernelGGL(mes_kernel, dim3((unsigned)T), dim3(AS_WAVE), 0, (hipStream_t)stream, moments, noise, best, n_obj, n_con,
                       T, acq, want_seeds ? seeds : (double*)nullptr, x, track ? d : 0, track ? best_v : (double*)nullptr, best_x);
    return CHECK_LAUNCH();
}

int mobocmf_ascent_adam_step(double* x, const double* gx, int32_t n_models, int32_t T, int32_t d, const double* lo,
                             const double* hi, double* exp_avg, double* exp_avg_sq, double lr, double beta1, double beta2,
                             double eps, int64_t* steps_done, mobocmf_stream_t stream) {
    if (!x || !gx || !lo || !hi || !exp_avg || !exp_avg_sq || !steps_done) return MOBOCMF_BAD_ARG;
    if (n_models < 1 || n_models > 2 * MOBOCMF_ACQ_MAX_PAIRS || T < 1 || T > MOBOCMF_TOPK_MAX_N || d < 1 || d > MOBOCMF_MAX_D)
        return MOBOCMF_BAD_ARG;
    hipLaunchKernelGGL(ascent_adam_kernel, dim3(1), dim3(AS_BLOCK), 0, (hipStream_t)stream, x, gx, n_models, T * d, d, lo, hi,
                       exp_avg, exp_avg_sq, lr, beta1, beta2, eps, steps_done);
    return CHECK_LAUNCH();
}

int mobocmf_select_topk(const double* vals, int32_t n, int32_t k, const double* x, int32_t d, double* out_vals,
                        int64_t* out_idx, double* out_x, mobocmf_stream_t stream) {
    if (!vals || !out_vals || !out_idx || k < 1 || k > MOBOCMF_TOPK_MAX_K || n < k || n > MOBOCMF_TOPK_MAX_N)
        return MOBOCMF_BAD_ARG;
    if ((x != nullptr) != (out_x != nullptr) || (x && (d < 1 || d > MOBOCMF_MAX_D))) return MOBOCMF_BAD_ARG;
    hipLaunchKernelGGL(select_topk_kernel, dim3(1), dim3(AS_BLOCK), 0, (hipStream_t)stream, vals, n, k, x, x ? d : 0, out_vals,
                       out_idx, out_x);
    return CHECK_LAUNCH();
}

}  // extern "C"
