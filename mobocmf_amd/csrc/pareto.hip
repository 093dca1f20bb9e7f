// Recommendation and its score (the reference's BO driver, examples/toy_synthetic_2D_JESMOCMF: the probably-feasible,
// non-dominated grid points of the predicted objectives, scored by pymoo's exact hypervolume).
//
// (a) mobocmf_pareto_mask: feasibility of every row under K_con Gaussian constraint predictions, then the non-dominated rows
//     among the feasible ones -- the rule of MOOP.compute_pareto_front (row j removes row i when p_j <= p_i everywhere and
//     p_j != p_i somewhere or j < i), restricted to the feasible rows.  Three launches in stream order: feasibility, dominance,
//     finalize.  The mask word of a row moves 0 (not a candidate) / 1 (candidate) -> 2 (dominated) -> 0 / 1 (front).
// (b) mobocmf_hypervolume: volume of the union of the boxes [p, ref] by the (k-2)-dimensional grid of cells over objectives
//     2..k-1 (one wave per cell), each cell a 2-D sweep (prefix minimum in objective-0 rank order) times the cell's volume;
//     ranks by counting (ties by index), partials summed in a fixed order: bitwise reproducible, no floating-point atomics.
#include <math.h>
#include <string.h>

#include "common.h"

#define PM_T 256       // threads of the row-parallel launches
#define PD_TJ 128      // candidate rows per LDS tile of the dominance launch
#define HV_T 256       // threads of the hypervolume launches (4 waves)
#define HV_CPW 4       // cells per wave of the cell launch (a workgroup: 4 waves x HV_CPW cells -> one partial)

__device__ __forceinline__ int32_t ld_relaxed(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one integer atomic per wave: lane 0 adds the wave's count (integer sums are order-independent)
__device__ __forceinline__ void wave_count(int64_t* dst, bool pred) {
    const unsigned long long b = __ballot(pred);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)dst, (unsigned long long)__popcll(b));
}

// ------------------------------------------------------------------ (a) feasibility + non-dominated mask
__global__ __launch_bounds__(PM_T) void pareto_feasible_kernel(int k, int64_t n, const double* __restrict__ vals, int64_t ldv,
                                                               int K_con, const double* __restrict__ cm,
                                                               const double* __restrict__ cv, int64_t ldc,
                                                               const double* __restrict__ noise, double p_min,
                                                               int32_t* __restrict__ mask, int64_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PM_T + threadIdx.x;
    const bool live = i < n;
    bool feas = live, nan = false;
    if (live) {
        for (int c = 0; c < K_con && feas; ++c) {
            // v < 0: sqrt is NaN and the comparison false (torch: NaN ratio); v == 0: +-inf or NaN, the sign of m decides
            const double v = cv[(int64_t)c * ldc + i] - (noise ? noise[c] : 0.0);
            const double z = cm[(int64_t)c * ldc + i] / sqrt(v);
            feas = 0.5 * erfc(-z / 1.4142135623730951) > p_min;
        }
        for (int c = 0; c < k; ++c) nan = nan || isnan(vals[(int64_t)c * ldv + i]);
        mask[i] = feas && !nan ? 1 : 0;
    }
    wave_count(counts + 0, feas);
    wave_count(counts + 2, feas && nan);
}

// One wave per workgroup: 64 candidate rows i in registers against the rows j of this workgroup's split, staged through LDS
// PD_TJ at a time.  A row is done once it has a dominator (or is no candidate); the wave leaves when the ballot says all 64
// are.  Splits of the same rows run in other workgroups: a dominator found there is published by the relaxed store of 2 and
// picked up here at the next tile (an early exit only; the result is the OR of the splits either way).
template <int KB>
__global__ __launch_bounds__(64) void pareto_dominance_kernel(int k, int64_t n, const double* __restrict__ vals, int64_t ldv,
                                                              int64_t split_rows, int32_t* mask) {
    __shared__ double tile[PD_TJ][KB];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const int64_t jb = (int64_t)blockIdx.y * split_rows;
    const int64_t je = jb + split_rows < n ? jb + split_rows : n;
    double mine[KB];
    bool done = !(i < n && ld_relaxed(mask + i) == 1);
#pragma unroll
    for (int c = 0; c < KB; ++c) mine[c] = (!done && c < k) ? vals[(int64_t)c * ldv + i] : 0.0;
    for (int64_t j0 = jb; j0 < je; j0 += PD_TJ) {
        if (!done) done = ld_relaxed(mask + i) == 2;
        if (__all(done)) break;                          // uniform: the workgroup is this one wave
        const int cnt = je - j0 < PD_TJ ? (int)(je - j0) : PD_TJ;
        __syncthreads();
        for (int e = lane; e < cnt * k; e += 64) {
            const int c = e / cnt, jj = e - c * cnt;
            double q = vals[(int64_t)c * ldv + j0 + jj];
            if (c == 0 && ld_relaxed(mask + j0 + jj) == 0) q = __builtin_nan("");   // not a candidate: dominates nothing
            tile[jj][c] = q;
        }
        __syncthreads();
        if (!done) {
            bool found = false;
            for (int jj = 0; jj < cnt && !found; ++jj) {
                bool le = true, lt = false;
#pragma unroll
                for (int c = 0; c < KB; ++c) {
                    if (c < k) {
                        const double q = tile[jj][c];
                        le = le && q <= mine[c];
                        lt = lt || q < mine[c];
                    }
                }
                found = le && (lt || j0 + jj < i);
            }
            if (found) {
                done = true;
                st_relaxed(mask + i, 2);
            }
        }
    }
}

__global__ __launch_bounds__(PM_T) void pareto_finalize_kernel(int64_t n, int32_t* __restrict__ mask,
                                                               int64_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PM_T + threadIdx.x;
    bool front = false;
    if (i < n) {
        front = mask[i] == 1;
        mask[i] = front ? 1 : 0;
    }
    wave_count(counts + 1, front);
}

extern "C" int mobocmf_pareto_mask(int32_t k, int64_t n, const double* vals, int64_t ldv, int32_t K_con,
                                   const double* con_mean, const double* con_var, int64_t ldc, const double* noise,
                                   double p_min, int32_t* mask, int64_t* counts, mobocmf_stream_t stream) {
    if (k < 1 || k > MOBOCMF_PARETO_MAX_K || n < 0 || n > INT32_MAX || K_con < 0 || !counts || isnan(p_min))
        return MOBOCMF_BAD_ARG;
    if (n > 0 && (!vals || !mask || ldv < n)) return MOBOCMF_BAD_ARG;
    if (n > 0 && K_con > 0 && (!con_mean || !con_var || ldc < n)) return MOBOCMF_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s));
    if (n == 0) return MOBOCMF_OK;
    const dim3 rows((unsigned)((n + PM_T - 1) / PM_T));
    hipLaunchKernelGGL(pareto_feasible_kernel, rows, dim3(PM_T), 0, s, k, n, vals, ldv, K_con, con_mean, con_var, ldc,
                       noise, p_min, mask, counts);
    // split the rows j over grid.y until ~8192 waves are in flight, each split at least 16 tiles long
    const int64_t nb = (n + 63) / 64;
    int64_t splits = (8192 + nb - 1) / nb;
    const int64_t max_splits = (n + 16 * PD_TJ - 1) / (16 * PD_TJ);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    const int64_t split_rows = ((n + splits - 1) / splits + PD_TJ - 1) / PD_TJ * PD_TJ;
    splits = (n + split_rows - 1) / split_rows;
    const dim3 grid((unsigned)nb, (unsigned)splits);
#define PD_GO(KB) hipLaunchKernelGGL((pareto_dominance_kernel<KB>), grid, dim3(64), 0, s, k, n, vals, ldv, split_rows, mask)
    if (k == 1) PD_GO(1);
    else if (k == 2) PD_GO(2);
    else if (k == 3) PD_GO(3);
    else if (k == 4) PD_GO(4);
    else if (k <= 8) PD_GO(8);
    else PD_GO(16);
#undef PD_GO
    hipLaunchKernelGGL(pareto_finalize_kernel, rows, dim3(PM_T), 0, s, n, mask, counts);
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}

// ------------------------------------------------------------------ (b) exact hypervolume
static int64_t hv_max_points(int k) { return k <= 3 ? 65536 : k == 4 ? 1024 : 256; }

struct HvLayout {
    int64_t res, V, cov, rank, perm, X, Y, R, W, part, total;   // byte offsets
    int64_t cells, parts;
};

static HvLayout hv_layout(int k, int64_t P) {
    HvLayout L;
    const int g = k > 2 ? k - 2 : 0;
    L.cells = 1;
    for (int c = 0; c < g; ++c) L.cells *= P;
    L.parts = (L.cells + 4 * HV_CPW - 1) / (4 * HV_CPW);
    int64_t o = 0;
    auto take = [&o](int64_t bytes) { const int64_t at = o; o += round_up(bytes, 256); return at; };
    L.res = take(16);                       // double result, int32 status
    L.V = take(8 * k * P);                  // clamped values, objective-major
    L.cov = take(4 * P);                    // 1: the point weakly dominates ref
    L.rank = take(4 * k * P);
    L.perm = take(4 * k * P);
    L.X = take(8 * (P + 1));                // objective 0 in rank order, X[P] = ref[0]
    L.Y = take(8 * P);                      // objective 1 of the point of rank t (yref when it covers nothing)
    L.R = take(4 * g * P);                  // ranks in objectives 2.. of the point of objective-0 rank t
    L.W = take(8 * g * P);                  // cell widths of objectives 2..
    L.part = take(8 * L.parts);
    L.total = o;
    return L;
}

// NaN anywhere (points or ref) sets the status; a point that does not weakly dominate ref is moved onto ref (it covers
// nothing and its cells have no width), NaN onto 0, so that the ranks below are always a permutation
__global__ __launch_bounds__(HV_T) void hv_prep_kernel(int k, int64_t P, const double* __restrict__ pts, int64_t ldp,
                                                       const double* __restrict__ ref, double* __restrict__ V,
                                                       int32_t* __restrict__ cov, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * HV_T + threadIdx.x;
    if (i >= P) return;
    bool bad = false, in = true;
    for (int c = 0; c < k; ++c) {
        const double p = pts[i * ldp + c], r = ref[c];
        bad = bad || isnan(p) || isnan(r);
        in = in && p <= r;
    }
    for (int c = 0; c < k; ++c) {
        const double p = pts[i * ldp + c], r = ref[c];
        const double v = in ? p : r;
        V[(int64_t)c * P + i] = isnan(v) ? 0.0 : v;
    }
    cov[i] = in && !bad;
    if (bad) st_relaxed(status, 1);
}

// rank of point i in objective blockIdx.y: points with a smaller value, or the same value and a smaller index
__global__ __launch_bounds__(HV_T) void hv_rank_kernel(int64_t P, const double* __restrict__ V, int32_t* __restrict__ rank,
                                                       int32_t* __restrict__ perm) {
    __shared__ double t[HV_T];
    const int c = blockIdx.y;
    const double* v = V + (int64_t)c * P;
    const int64_t i = (int64_t)blockIdx.x * HV_T + threadIdx.x;
    const double me = i < P ? v[i] : 0.0;
    int32_t r = 0;
    for (int64_t j0 = 0; j0 < P; j0 += HV_T) {
        const int cnt = P - j0 < HV_T ? (int)(P - j0) : HV_T;
        __syncthreads();
        if (threadIdx.x < cnt) t[threadIdx.x] = v[j0 + threadIdx.x];
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
            const double q = t[jj];
            r += (q < me || (q == me && j0 + jj < i)) ? 1 : 0;
        }
    }
    if (i < P) {
        rank[(int64_t)c * P + i] = r;
        perm[(int64_t)c * P + r] = (int32_t)i;
    }
}

__global__ __launch_bounds__(HV_T) void hv_pack_kernel(int k, int64_t P, const double* __restrict__ ref,
                                                       const double* __restrict__ V, const int32_t* __restrict__ cov,
                                                       const int32_t* __restrict__ rank, const int32_t* __restrict__ perm,
                                                       double* __restrict__ X, double* __restrict__ Y,
                                                       int32_t* __restrict__ R, double* __restrict__ W) {
    const int64_t t = (int64_t)blockIdx.x * HV_T + threadIdx.x;
    if (t >= P) return;
    const double yref = k >= 2 ? ref[1] : 1.0;           // k = 1: every point covers height 1 (y = 0, yref = 1)
    const int32_t i = perm[t];
    X[t] = V[i];
    if (t == P - 1) X[P] = ref[0];
    Y[t] = cov[i] ? (k >= 2 ? V[P + i] : 0.0) : yref;
    for (int c = 2; c < k; ++c) {
        const double* v = V + (int64_t)c * P;
        const int32_t* pc = perm + (int64_t)c * P;
        R[(int64_t)(c - 2) * P + t] = rank[(int64_t)c * P + i];
        W[(int64_t)(c - 2) * P + t] = (t + 1 < P ? v[pc[t + 1]] : ref[c]) - v[pc[t]];
    }
}

// cells: mixed radix P over objectives 2..k-1 (objective 2 fastest).  A wave takes HV_CPW consecutive cells; a cell's volume
// is the product of its widths times the area that the points covering its lower corner (rank <= the cell's in every one of
// these objectives) dominate in objectives 0 and 1: the sweep over objective-0 ranks with an inclusive prefix minimum of y.
__global__ __launch_bounds__(HV_T) void hv_cells_kernel(int k, int64_t P, const double* __restrict__ ref,
                                                        const double* __restrict__ X, const double* __restrict__ Y,
                                                        const int32_t* __restrict__ R, const double* __restrict__ W,
                                                        int64_t cells, double* __restrict__ part) {
    __shared__ double wsum[HV_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = k > 2 ? k - 2 : 0;
    const double yref = k >= 2 ? ref[1] : 1.0;
    double acc = 0.0;                                     // uniform over the wave
    for (int q = 0; q < HV_CPW; ++q) {
        const int64_t cell = ((int64_t)blockIdx.x * (HV_T / 64) + wave) * HV_CPW + q;
        if (cell >= cells) break;
        int32_t rc[3] = {0, 0, 0};
        double w = 1.0;
        int64_t rest = cell;
        for (int c = 0; c < g; ++c) {
            rc[c] = (int32_t)(rest % P);
            rest /= P;
            w *= W[(int64_t)c * P + rc[c]];
        }
        if (w == 0.0) continue;
        double carry = yref, area = 0.0;
        for (int64_t t0 = 0; t0 < P; t0 += 64) {
            const int64_t t = t0 + lane;
            double y = yref, dx = 0.0;
            if (t < P) {
                bool in = true;
                for (int c = 0; c < g; ++c) in = in && R[(int64_t)c * P + t] <= rc[c];
                if (in) y = Y[t];
                dx = X[t + 1] - X[t];
            }
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const double o = __shfl_up(y, s);
                if (lane >= s) y = fmin(y, o);
            }
            y = fmin(y, carry);
            carry = __shfl(y, 63);
            area += dx * (yref - y);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) area += __shfl_xor(area, s);   // every lane: the same sum
        acc += w * area;
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}

__global__ __launch_bounds__(HV_T) void hv_reduce_kernel(int64_t parts, const double* __restrict__ part,
                                                         double* __restrict__ out) {
    __shared__ double s[HV_T];
    double a = 0.0;
    for (int64_t p = threadIdx.x; p < parts; p += HV_T) a += part[p];
    s[threadIdx.x] = a;
    for (int h = HV_T / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
    }
    if (threadIdx.x == 0) out[0] = s[0];
}

static bool hv_shape_ok(int32_t k, int64_t P) {
    return k >= 1 && k <= MOBOCMF_HV_MAX_K && P >= 0 && P <= hv_max_points(k);
}

extern "C" int mobocmf_hypervolume_workspace_bytes(int32_t k, int64_t P, size_t* bytes) {
    if (!bytes || !hv_shape_ok(k, P)) return MOBOCMF_BAD_ARG;
    *bytes = (size_t)hv_layout(k, P).total;
    return MOBOCMF_OK;
}

extern "C" int mobocmf_hypervolume(int32_t k, int64_t P, const double* pts, int64_t ldp, const double* ref, double* hv,
                                   void* workspace, size_t workspace_bytes, mobocmf_stream_t stream) {
    if (!hv || !hv_shape_ok(k, P) || !ref) return MOBOCMF_BAD_ARG;
    if (P > 0 && (!pts || ldp < k)) return MOBOCMF_BAD_ARG;
    if (P == 0) {                                         // ref still has to be a number
        double r[MOBOCMF_HV_MAX_K];
        HIP_TRY(hipMemcpyAsync(r, ref, sizeof(double) * k, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        for (int c = 0; c < k; ++c)
            if (isnan(r[c])) return MOBOCMF_BAD_ARG;
        *hv = 0.0;
        return MOBOCMF_OK;
    }
    const HvLayout L = hv_layout(k, P);
    if (!workspace || workspace_bytes < (size_t)L.total) return MOBOCMF_WORKSPACE_TOO_SMALL;
    char* ws = (char*)workspace;
    double* res = (double*)(ws + L.res);
    int32_t* status = (int32_t*)(ws + L.res + 8);
    double* V = (double*)(ws + L.V);
    int32_t* cov = (int32_t*)(ws + L.cov);
    int32_t* rank = (int32_t*)(ws + L.rank);
    int32_t* perm = (int32_t*)(ws + L.perm);
    double* X = (double*)(ws + L.X);
    double* Y = (double*)(ws + L.Y);
    int32_t* R = (int32_t*)(ws + L.R);
    double* W = (double*)(ws + L.W);
    double* part = (double*)(ws + L.part);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(ws + L.res, 0, 16, s));
    const dim3 pts_grid((unsigned)((P + HV_T - 1) / HV_T));
    hipLaunchKernelGGL(hv_prep_kernel, pts_grid, dim3(HV_T), 0, s, k, P, pts, ldp, ref, V, cov, status);
    hipLaunchKernelGGL(hv_rank_kernel, dim3(pts_grid.x, (unsigned)k), dim3(HV_T), 0, s, P, V, rank, perm);
    hipLaunchKernelGGL(hv_pack_kernel, pts_grid, dim3(HV_T), 0, s, k, P, ref, V, cov, rank, perm, X, Y, R, W);
    hipLaunchKernelGGL(hv_cells_kernel, dim3((unsigned)L.parts), dim3(HV_T), 0, s, k, P, ref, X, Y, R, W, L.cells, part);
    hipLaunchKernelGGL(hv_reduce_kernel, dim3(1), dim3(HV_T), 0, s, L.parts, part, res);
    HIP_TRY(hipGetLastError());
    double host[2];
    HIP_TRY(hipMemcpyAsync(host, res, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int32_t st;
    memcpy(&st, (const char*)host + 8, 4);
    if (st != 0) return MOBOCMF_BAD_ARG;
    *hv = host[0];
    return MOBOCMF_OK;
}
