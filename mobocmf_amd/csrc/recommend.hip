// The recommendation evolved on the GPU (BlackBoxMFDGPFitter.recommend(search="evolve"), util/recommend_evolve.py): what stands
// between a predict group's forward launch and mobocmf_nsga_survive -- the objective values (the surrogates' predictive means over
// the S fixed samples) and the graded violation of the probabilistic feasibility rule of mobocmf_pareto_mask, from the group's raw
// top-layer moments (include/mobocmf_hip.h states every expression).
//
// ONE launch of T workgroups of one wavefront, a lane per model, as the JES kernel of acq_search.hip is built (a generation has
// T = Np <= 512 test points and a handful of models: one thread per test point would leave a few lanes looping over every model
// and sample): the lane sums its model's S samples in order, a constraint's lane parks its term in LDS, lane 0 adds the terms in
// the order of the constraints.  No atomics, static LDS only, every thread reaches the barrier; reads nothing on the host and
// keeps no state: capturable.
#include <float.h>
#include <math.h>

#include "common.h"

#define RS_WAVE 64

__global__ void __launch_bounds__(RS_WAVE)
recommend_scores_kernel(const double* __restrict__ moments, int n_obj, int n_con, int T, int S,
                        const double* __restrict__ scale, double p_min, double z_min, double* __restrict__ F, int64_t ldf,
                        double* __restrict__ viol) {
#pragma clang fp contract(off)      // the header's expressions in IEEE operations as written: the host restatement's bits
    __shared__ double s_term[RS_WAVE];
    const int t = blockIdx.x, m = threadIdx.x;
    if (m < n_obj + n_con) {
        const int64_t ncol = (int64_t)T * S;
        const double* mu = moments + (int64_t)m * 2 * ncol + (int64_t)t * S;
        const double* var = mu + ncol;
        double mbar, v;
        if (S == 1) {
            mbar = mu[0];
            v = var[0];
        } else {
            double a = 0.0, q = 0.0;
            for (int s = 0; s < S; ++s) {
                const double ms = mu[s];
                a = a + ms;
                q = q + (var[s] + ms * ms);
            }
            mbar = a / (double)S;
            v = q / (double)S - mbar * mbar;
        }
        if (scale) {
            const double shift = scale[2 * m], factor = scale[2 * m + 1];
            mbar = mbar * factor + shift;
            v = (v * factor) * factor;
        }
        if (m < n_obj) {
            F[(int64_t)m * ldf + t] = mbar;
        } else {
            // v < 0: sqrt is NaN; v == 0: z is +-inf (the sign of the mean decides) or NaN
            const double z = mbar / sqrt(v);
            const bool feas = 0.5 * erfc(-(z / 1.4142135623730951)) > p_min;
            double w;
            if (v < 0.0 || z != z) w = __builtin_inf();
            else if (feas) w = 0.0;
            else w = fmax(z_min - z, DBL_MIN);
            s_term[m - n_obj] = w;
        }
    }
    __syncthreads();
    if (m == 0 && viol) {
        double sum = 0.0;
        for (int c = 0; c < n_con; ++c) sum = sum + s_term[c];
        viol[t] = sum;
    }
}

extern "C" int mobocmf_recommend_scores(const double* moments, int32_t n_obj, int32_t n_con, int32_t T, int32_t S,
                                        const double* scale, double p_min, double z_min, double* F, int64_t ldf, double* viol,
                                        mobocmf_stream_t stream) {
    if (!moments || !F || n_obj < 1 || n_obj > MOBOCMF_PARETO_MAX_K || n_con < 0 || (int64_t)n_obj + n_con > RS_WAVE)
        return MOBOCMF_BAD_ARG;
    if (T < 1 || S < 1 || (int64_t)T * S > MOBOCMF_ACQ_MAX_COLUMNS || ldf < T || (n_con > 0 && !viol)) return MOBOCMF_BAD_ARG;
    if (!(p_min > 0.0 && p_min < 1.0) || !isfinite(z_min)) return MOBOCMF_BAD_ARG;      // (a NaN fails both)
    hipLaunchKernelGGL(recommend_scores_kernel, dim3((unsigned)T), dim3(RS_WAVE), 0, (hipStream_t)stream, moments, (int)n_obj,
                       (int)n_con, (int)T, (int)S, scale, p_min, z_min, F, ldf, viol);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}
