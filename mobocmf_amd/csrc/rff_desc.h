// The bounds rule of a chain sample's layer descriptor, shared by every kernel that reads operands through one (rff.hip,
// rff_opt.hip): a layer that fails it is never dereferenced.
#pragma once
#include "common.h"

// operands of a layer descriptor inside params[0, len)
__device__ __forceinline__ bool rff_desc_ok(const mobocmf_rff_layer_desc& L, int l, int d, int64_t len) {
    if (L.kind != (l == 0 ? 0 : 1) || L.F < 1) return false;
    const int64_t F = L.F, Fd = F * d;
    auto in = [len](int64_t off, int64_t cnt) { return off >= 0 && off <= len - cnt; };
    if (!in(L.W1, Fd) || !in(L.b1, F) || !in(L.theta, L.kind == 0 ? F : 3 * F)) return false;
    return L.kind == 0 || (in(L.Wf, F) && in(L.W2, Fd) && in(L.b2, F));
}
