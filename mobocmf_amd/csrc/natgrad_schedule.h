// The gamma schedule of the natural-gradient steps (natgrad.hip, natgrad_small.hip), evaluated on the device from a step counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// gamma_t = min(gamma, gamma_init rho^t), rho = (gamma / gamma_init)^(1 / warmup): as gamma_init exp(t / warmup log(gamma /
// gamma_init)), whose rounding error does not grow with t
__device__ __forceinline__ double gamma_at(int64_t t, double gamma, double gamma_init, double log_ratio, int warmup) {
    if (warmup <= 0 || t >= warmup) return gamma;
    if (t < 0) t = 0;
    return fmin(gamma, gamma_init * exp((double)t / (double)warmup * log_ratio));
}
