// Mini-batches drawn on the device (the loader of blackbox_mfdgp_fitter.py:35, DataLoader(shuffle=True), and its use in the
// epoch loop :156-173), so that a replay of the captured ELBO step sees a fresh batch without the host.
//
// The epoch permutation is a stateless keyed bijection (minibatch_perm.h): position i of epoch e is a pure function of
// (seed, e, N, i) -- no N-sized buffer, no sort, no epoch-boundary launch.  Two launches per step:
//   mb_index_kernel   ONE workgroup.  Reads the device state {seed, step, status}, forms epoch = step / nb, k = step % nb, the source
//                     rows of positions kB .. min((k+1)B, N)-1, orders them stably by descending fidelity (per-thread runs of
//                     positions, one scan over the [level][thread] counts in LDS, a scatter: deterministic, no atomics), writes
//                     src and the per-level counts #{fid >= l}, and advances step.  Guard: the caller says how many rows it
//                     expects (its buffers and its captured graph are sized for them); if batch k has another number, or the
//                     status is already set, the launch sets status and writes neither src nor step.
//   mb_gather_kernel  grid-wide, whole rows: xb[r] = x[src[r]], yb[r] = y[src[r]], fidb[r] = fid[src[r]].  A row whose src is
//                     outside 0..N-1 (src was never written: the guard refused) is skipped, and so is everything when status is set.
// No workgroup waits on another; state, src and counts are each written by one launch and read by the launches after it.
// mb_accumulate_kernel adds the step's loss and scaled KL into per-epoch sums on the device (the sums :156-173 prints).
#include "common.h"
#include "minibatch_perm.h"

#define MB_T 1024                   // threads of the index launch
#define MB_L MOBOCMF_MINIBATCH_MAX_LEVELS
#define MB_KEEP 8                   // rows of its run a thread keeps in registers between the count and the scatter (B <= 8192:
                                    // the whole run; the permutation is the launch's arithmetic, ~60 Philox rounds per row)

__device__ __forceinline__ int mb_level(const double* __restrict__ fid, int64_t row, int L) {
    const int l = (int)fid[row];
    return l < 0 ? 0 : (l >= L ? L - 1 : l);
}

__global__ __launch_bounds__(MB_T) void mb_index_kernel(int64_t N, int64_t B, int L, const double* __restrict__ fid,
                                                        int ordered, int64_t rows_expected, int64_t* __restrict__ state,
                                                        int64_t* __restrict__ src, int64_t* __restrict__ counts) {
    __shared__ int32_t cnt[MB_L * MB_T];      // [bucket][thread]; bucket q holds level L-1-q (descending fidelity)
    __shared__ int32_t wave_sum[MB_T / 64];
    const int tid = threadIdx.x;
    const int64_t seed = state[0], step = state[1], status = state[2];
    const int64_t nb = (N + B - 1) / B;
    const int64_t epoch = step / nb, k = step % nb;
    const int64_t first = k * B;
    const int64_t rows = (N - first < B) ? N - first : B;
    // Uniform although the words are read per wavefront: seed and step are written only after the barriers below, which no
    // wavefront reaches on this path; a wavefront that loads status after thread 0 has stored it here sees it set and leaves too.
    // Nothing but status is written on the refusal path, so the return before the barriers is safe.
    if (status != 0 || step < 0 || rows != rows_expected) {
        if (tid == 0 && status == 0) state[2] = step < 0 ? MOBOCMF_MINIBATCH_BAD_STATE : MOBOCMF_MINIBATCH_ROWS_MISMATCH;
        return;
    }
    const mb_perm_key key = mb_perm_make(seed, epoch, N);
    const int64_t per = (rows + MB_T - 1) / MB_T;              // positions of the batch per thread: a contiguous run
    const int64_t lo = tid * per < rows ? tid * per : rows;
    const int64_t hi = lo + per < rows ? lo + per : rows;
    int32_t c[MB_L];
    int32_t keep[MB_KEEP];      // the first MB_KEEP rows of the run (N <= 2^31: they fit 32 bits as unsigned)
#pragma unroll
    for (int q = 0; q < MB_L; ++q) c[q] = 0;
#pragma unroll
    for (int j = 0; j < MB_KEEP; ++j) {
        keep[j] = 0;
        if (lo + j < hi) {
            const int64_t row = mb_perm_at(key, first + lo + j);
            keep[j] = (int32_t)(uint32_t)row;
            const int q = L - 1 - mb_level(fid, row, L);
#pragma unroll
            for (int u = 0; u < MB_L; ++u) c[u] += (u == q);
        }
    }
    for (int64_t i = lo + MB_KEEP; i < hi; ++i) {
        const int q = L - 1 - mb_level(fid, mb_perm_at(key, first + i), L);
#pragma unroll
        for (int u = 0; u < MB_L; ++u) c[u] += (u == q);
    }
#pragma unroll
    for (int q = 0; q < MB_L; ++q)
        if (q < L) cnt[q * MB_T + tid] = c[q];
    __syncthreads();
    // exclusive scan of the flattened [bucket][thread] counts: entry (q, t) becomes the output offset of thread t's first row
    // of bucket q.  Thread t owns the L consecutive entries t*L .. t*L+L-1.
    int32_t own = 0;
    for (int u = 0; u < L; ++u) own += cnt[tid * L + u];
    int32_t incl = own;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int32_t o = __shfl_up(incl, s);
        if ((tid & 63) >= s) incl += o;
    }
    if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
    __syncthreads();
    int32_t base = incl - own;
    for (int w = 0; w < (tid >> 6); ++w) base += wave_sum[w];
    for (int u = 0; u < L; ++u) {
        const int32_t v = cnt[tid * L + u];
        cnt[tid * L + u] = base;
        base += v;
    }
    __syncthreads();
    if (tid < L) counts[tid] = tid == 0 ? rows : (int64_t)cnt[(L - tid) * MB_T];      // #{fid >= l}: the buckets before level l-1's
    if (ordered) {
        int32_t off[MB_L];
#pragma unroll
        for (int q = 0; q < MB_L; ++q) off[q] = q < L ? cnt[q * MB_T + tid] : 0;
#pragma unroll
        for (int j = 0; j < MB_KEEP; ++j)
            if (lo + j < hi) {
                const int64_t row = (int64_t)(uint32_t)keep[j];
                const int q = L - 1 - mb_level(fid, row, L);
                int32_t o = 0;
#pragma unroll
                for (int u = 0; u < MB_L; ++u) {
                    if (u == q) o = off[u];
                    off[u] += (u == q);
                }
                src[o] = row;
            }
        for (int64_t i = lo + MB_KEEP; i < hi; ++i) {
            const int64_t row = mb_perm_at(key, first + i);
            const int q = L - 1 - mb_level(fid, row, L);
            int32_t o = 0;
#pragma unroll
            for (int u = 0; u < MB_L; ++u) {
                if (u == q) o = off[u];
                off[u] += (u == q);
            }
            src[o] = row;
        }
    } else {
#pragma unroll
        for (int j = 0; j < MB_KEEP; ++j)
            if (lo + j < hi) src[lo + j] = (int64_t)(uint32_t)keep[j];
        for (int64_t i = lo + MB_KEEP; i < hi; ++i) src[i] = mb_perm_at(key, first + i);
    }
    if (tid == 0) state[1] = step + 1;      // every thread took its copy of the word before the barriers above
}

// V = 2: rows of d / 2 double2 (16-byte accesses), V = 1: rows of d doubles
template <int V>
__global__ __launch_bounds__(256) void mb_gather_kernel(int64_t N, int d, int64_t rows, const double* __restrict__ x,
                                                        const double* __restrict__ y, const double* __restrict__ fid,
                                                        const int64_t* __restrict__ src, const int64_t* __restrict__ state,
                                                        double* __restrict__ xb, double* __restrict__ yb,
                                                        double* __restrict__ fidb) {
    if (state[2] != 0) return;
    const int u = d / V;                      // units per row
    const int64_t total = rows * u, nt = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += nt) {
        const int64_t r = e / u;
        const int cidx = (int)(e - r * u);
        const int64_t s = src[r];
        if (s < 0 || s >= N) continue;
        if (V == 2) ((double2*)xb)[r * u + cidx] = ((const double2*)x)[s * u + cidx];
        else xb[r * u + cidx] = x[s * u + cidx];
        if (cidx == 0) {
            yb[r] = y[s];
            fidb[r] = fid[s];
        }
    }
}

// sums[0..1]: loss / scaled KL summed over the steps of the epoch in progress; sums[2..3]: the sums of the last finished epoch.
// One thread; state[1] is the step count AFTER this step's index launch.
__global__ void mb_accumulate_kernel(int64_t N, int64_t B, const int64_t* __restrict__ state, const double* __restrict__ loss,
                                     const double* __restrict__ kl, double* __restrict__ sums) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || state[2] != 0 || state[1] < 1) return;
    const int64_t nb = (N + B - 1) / B, k = (state[1] - 1) % nb;
    const double a = (k == 0 ? 0.0 : sums[0]) + loss[0], b = (k == 0 ? 0.0 : sums[1]) + kl[0];
    sums[0] = a;
    sums[1] = b;
    if (k == nb - 1) { sums[2] = a; sums[3] = b; }
}

static bool mb_shape_ok(int64_t N, int64_t B) {
    return N >= 1 && N <= MOBOCMF_MINIBATCH_MAX_ROWS && B >= 1 && B < MOBOCMF_MINIBATCH_MAX_ROWS;
}

extern "C" int mobocmf_minibatch_permutation_host(int64_t seed, int64_t epoch, int64_t N, int64_t* out) {
    if (!out || N < 1 || N > MOBOCMF_MINIBATCH_MAX_ROWS || epoch < 0) return MOBOCMF_BAD_ARG;
    const mb_perm_key key = mb_perm_make(seed, epoch, N);
    for (int64_t i = 0; i < N; ++i) out[i] = mb_perm_at(key, i);
    return MOBOCMF_OK;
}

extern "C" int mobocmf_minibatch_indices(int64_t N, int64_t B, int32_t L, const double* fid, int32_t order_by_fidelity,
                                         int64_t rows_expected, int64_t* state, int64_t* src, int64_t* counts,
                                         mobocmf_stream_t stream) {
    if (!mb_shape_ok(N, B) || L < 1 || L > MOBOCMF_MINIBATCH_MAX_LEVELS || (order_by_fidelity != 0 && order_by_fidelity != 1))
        return MOBOCMF_BAD_ARG;
    if (rows_expected < 1 || rows_expected > B || rows_expected > N) return MOBOCMF_BAD_ARG;
    if (!fid || !state || !src || !counts) return MOBOCMF_BAD_ARG;
    hipLaunchKernelGGL(mb_index_kernel, dim3(1), dim3(MB_T), 0, (hipStream_t)stream, N, B, (int)L, fid, (int)order_by_fidelity,
                       rows_expected, state, src, counts);
    HIP_TRY(hipGetLastError());
    return MOBOCMF_OK;
}

extern "C" int mobocmf_minibatch_gather(int64_t N, int32_t d, int64_t rows, const double* x, const double* y, const double* fid,
                                        const int64_t* src, const int64_t* state, double* xb, double* yb, double* fidb,
                                        mobocmf_stream_t stream) {
    if (N < 1 || N > MOBOCMF_MINIBATCH_MAX_ROWS || d < 1 || d > MOBOCMF_MAX_D || rows < 1 || rows > N) return MOBOCMF_BAD_ARG;
    if (!x || !y || !fid || !src || !state || !xb || !yb || !fidb) return MOBOCMF_BAD_ARG;
    const bool wide = d % 2 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)xb & 15) == 0;
    const int64_t total = rows * (wide ? d / 2 : d);
    const int64_t want = (total + 255) / 256;
    const int grid = (int)(want < 2048 ? want : 2048);
    hipStream_t s = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL(mb_gather_kernel<2>, dim3(grid), dim3(256), 0, s, N, (int)d, rows, x, y, fid, src, state, xb, yb, fidb);
    else hipLaunchKernelGGL(mb_gather_kernel<1>, dim3(grid), dim3(256), 0, s, N, (int)d, rows, x, y, fid, src, state, xb, yb, fidb);
    HIP_TRY(hipGetLastError());
    return MOBOCMF_OK;
}

extern "C" int mobocmf_minibatch_accumulate(int64_t N, int64_t B, const int64_t* state, const double* loss, const double* kl,
                                            double* sums, mobocmf_stream_t stream) {
    if (!mb_shape_ok(N, B) || !state || !loss || !kl || !sums) return MOBOCMF_BAD_ARG;
    hipLaunchKernelGGL(mb_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, N, B, state, loss, kl, sums);
    HIP_TRY(hipGetLastError());
    return MOBOCMF_OK;
}
