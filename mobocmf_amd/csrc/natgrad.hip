// Natural-gradient step of q(u) = N(m, L_S L_S^T) for up to MAX_ZL layers of equal M ("Natural gradients").
//   Psi   = sym(Phi(L_S^T g_LS))             G_S = dloss/dS = L_S^-T Psi L_S^-1   (the reverse-mode Cholesky rule)
//   B     = I + 2 gamma_t Psi                S_new = L_S B^-1 L_S^T
//   J B J = C C^T  (J reverses the real M indices; the padding up to Mp is identity),  T = J C^-T J  lower, T T^T = B^-1
//   L_new = L_S T                            m_new = m - gamma_t L_new (L_new^T g_m)
// The Cholesky, the triangular inverse, Phi and the two M x M products run on the z-batched launchers of the layer chain; this
// file holds the glue around them and the call's orchestration.  gamma_t is evaluated on the device from the step counter; a
// layer whose factorisation reports a pivot keeps its m and L_S bitwise and counts the step in `skipped`.  No host read, no
// floating-point atomics, fixed summation orders: capturable and bitwise reproducible.
#include <math.h>

#include "common.h"
#include "natgrad_schedule.h"

#define TRY(x)               \
    do {                     \
        int _rc = (x);       \
        if (_rc) return _rc; \
    } while (0)
#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR)
#define GRIDZ(n, nz) dim3((unsigned)(((n) + 255) / 256), 1, (unsigned)(nz)), dim3(256)

namespace {

// the user tensors of the call's layers (not strided: tables by value)
struct NgTensors {
    double* m[MAX_ZL];
    double* LS[MAX_ZL];
    const double* gm[MAX_ZL];
    const double* gLS[MAX_ZL];
    int32_t* skipped[MAX_ZL];
    const int32_t* info[MAX_ZL];
};

// LSp = tril(L_S) zero-padded to Mp x Mp, LST its transpose, Gp = scale tril(g_LS) padded, gp = scale g_m padded
__global__ void natgrad_pad_kernel(NgTensors t, int M, int Mp, double scale, double* LSp, double* LST, double* Gp, double* gp,
                                   int64_t zs) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Mp * Mp) return;
    const int z = blockIdx.z;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    const bool low = i < M && j <= i, up = j < M && i <= j;
    LSp[z * zs + idx] = low ? t.LS[z][(int64_t)i * M + j] : 0.0;
    LST[z * zs + idx] = up ? t.LS[z][(int64_t)j * M + i] : 0.0;
    Gp[z * zs + idx] = low ? scale * t.gLS[z][(int64_t)i * M + j] : 0.0;
    if (idx < Mp) gp[z * zs + idx] = idx < M ? scale * t.gm[z][idx] : 0.0;
}

// Brev = J (I + 2 gamma_t sym(P)) J on the real M x M block, identity on the padding; P = Phi(L_S^T g_LS) (lower, halved
// diagonal).  The first thread of the launch leaves gamma_t in gam[0] for the write-back.
__global__ void natgrad_form_b_kernel(const double* P, int M, int Mp, double* Brev, const int64_t* step_count, double gamma,
                                      double gamma_init, double log_ratio, int warmup, double* gam, int64_t zs) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Mp * Mp) return;
    const int z = blockIdx.z;
    const double g = gamma_at(step_count[0], gamma, gamma_init, log_ratio, warmup);
    if (z == 0 && idx == 0) gam[0] = g;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    double b = i == j ? 1.0 : 0.0;
    if (i < M && j < M) {
        const int r = M - 1 - i, c = M - 1 - j;
        const int hi = r > c ? r : c, lo = r > c ? c : r;
        const double p = P[z * zs + (int64_t)hi * Mp + lo];
        b += 2.0 * g * (r == c ? p : 0.5 * p);
    }
    Brev[z * zs + idx] = b;
}

// T = J C^-T J on the real block (lower triangular), zero elsewhere
__global__ void natgrad_form_t_kernel(const double* Cinv, int M, int Mp, double* Tp, int64_t zs) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Mp * Mp) return;
    const int z = blockIdx.z;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    Tp[z * zs + idx] = (i < M && j <= i) ? Cinv[z * zs + (int64_t)(M - 1 - j) * Mp + (M - 1 - i)] : 0.0;
}

// v = L_new^T gp over the real lower triangle: 64 columns per workgroup, four row classes per column summed in a fixed order
__global__ __launch_bounds__(256) void natgrad_ltg_kernel(const double* Lnew, const double* gp, int M, int Mp, double* v,
                                                          int64_t zs) {
    __shared__ double part[4][64];
    const int z = blockIdx.y;
    Lnew += z * zs; gp += z * zs; v += z * zs;
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    double acc = 0.0;
    if (j < M)
        for (int i = j + rg; i < M; i += 4) acc += Lnew[(int64_t)i * Mp + j] * gp[i];
    part[rg][c] = acc;
    __syncthreads();
    if (rg == 0 && j < M) v[j] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

// Guarded write-back, one wavefront per row i: w_i = sum_{j <= i} L_new[i][j] v[j]; if the layer's factorisation succeeded,
// L_S[i][0..i] <- L_new[i][0..i] and m[i] -= gamma_t w_i, else nothing of the layer is written and `skipped` counts the step.
// The step counter advances here: every reader of it (natgrad_form_b_kernel) has finished.
__global__ __launch_bounds__(256) void natgrad_writeback_kernel(NgTensors t, const double* Lnew, const double* v, const double* gam,
                                                                int64_t* step_count, int M, int Mp, int64_t zs) {
    const int z = blockIdx.y;
    const bool ok = t.info[z][0] == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (!ok) t.skipped[z][0] += 1;
        if (z == 0) step_count[0] += 1;
    }
    if (!ok) return;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= M) return;
    const double* row = Lnew + z * zs + (int64_t)i * Mp;
    const double* vz = v + z * zs;
    double* out = t.LS[z] + (int64_t)i * M;
    double acc = 0.0;
    for (int j = lane; j <= i; j += 64) {
        const double l = row[j];
        acc += l * vz[j];
        out[j] = l;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) t.m[z][i] -= gam[0] * acc;
}

struct NgWs {
    double *LSp, *LST, *Gp, *T2, *P, *Brev, *Cinv, *Tscr, *Tp, *Lnew, *Dinv, *Ld, *ws, *gp, *v, *gam;
    int64_t ws_elems;
};

// one block per layer, the blocks `*block_bytes` apart; base == 0: size query
void carve(uintptr_t base, int Mp, NgWs& w, size_t* block_bytes) {
    size_t off = 0;
    auto take = [&](int64_t n) {
        double* r = base ? (double*)(base + off) : nullptr;
        off += ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
        return r;
    };
    const int64_t mm = (int64_t)Mp * Mp, dd = (int64_t)(Mp / NB) * NB * NB;
    w.LSp = take(mm); w.LST = take(mm); w.Gp = take(mm); w.T2 = take(mm); w.P = take(mm); w.Brev = take(mm);
    w.Cinv = take(mm); w.Tscr = take(mm); w.Tp = take(mm); w.Lnew = take(mm);
    w.Dinv = take(dd); w.Ld = take(dd);
    // slabs of the k-sliced products and the hand-over words of the one-launch factorisation: the size the chain gives its own
    // ws (api.hip carve_chain_fwd), so that the same products take the same slab counts here as there
    w.ws_elems = 16 * mm;
    w.ws = take(w.ws_elems);
    w.gp = take(Mp); w.v = take(Mp); w.gam = take(4);
    *block_bytes = off;
}

bool shape_ok(int32_t n, int32_t M) { return n >= 1 && n <= MAX_ZL && M >= 1 && M <= MOBOCMF_NATGRAD_MAX_M; }

GemmArgs mm_gemm(const double* A, const double* B, double* C, int Mp, int M, int tri, int n, int64_t zs) {
    GemmArgs g = {};
    g.A = A; g.lda = Mp; g.B = B; g.ldb = Mp; g.C = C; g.ldc = Mp;
    g.Mr = Mp; g.Nc = Mp; g.Kd = Mp; g.tri = tri; g.alpha = 1.0;
    g.Kreal = M;      // the contraction's padded tail multiplies zeros
    if (n > 1) { g.zlayers = n; g.zsA = g.zsB = g.zsC = zs; }
    return g;
}

}  // namespace

extern "C" {

int mobocmf_natgrad_workspace_bytes(int32_t M, int32_t n, size_t* bytes) {
    if (!bytes || !shape_ok(n, M)) return MOBOCMF_BAD_ARG;
    NgWs w;
    size_t block = 0;
    carve(0, (int)round_up(M, TILE), w, &block);
    *bytes = block * (size_t)n;
    return MOBOCMF_OK;
}

int mobocmf_natgrad_step(int32_t n, int32_t M, double* const* m, double* const* L_S, const double* const* g_m,
                         const double* const* g_LS, double gamma, double gamma_init, int32_t warmup_steps, double scale,
                         int64_t* step_count, int32_t* const* skipped, int32_t* const* info, void* workspace, size_t bytes,
                         const mobocmf_tuning* tuning, mobocmf_stream_t stream) {
    if (!shape_ok(n, M) || !m || !L_S || !g_m || !g_LS || !step_count || !skipped || !info || !workspace || !tuning_ok(tuning))
        return MOBOCMF_BAD_ARG;
    if (!(gamma > 0.0) || !(gamma_init > 0.0) || !(gamma_init <= gamma) || !(gamma < INFINITY) || warmup_steps < 0 ||
        !(scale > 0.0) || !(scale < INFINITY))
        return MOBOCMF_BAD_ARG;
    NgTensors t = {};
    for (int z = 0; z < n; ++z) {
        if (!m[z] || !L_S[z] || !g_m[z] || !g_LS[z] || !skipped[z] || !info[z]) return MOBOCMF_BAD_ARG;
        t.m[z] = m[z]; t.LS[z] = L_S[z]; t.gm[z] = g_m[z]; t.gLS[z] = g_LS[z]; t.skipped[z] = skipped[z]; t.info[z] = info[z];
    }
    if ((uintptr_t)workspace & 255) return MOBOCMF_BAD_ARG;
    const int Mp = (int)round_up(M, TILE);
    NgWs w;
    size_t block = 0;
    carve((uintptr_t)workspace, Mp, w, &block);
    if (bytes / (size_t)n < block) return MOBOCMF_WORKSPACE_TOO_SMALL;
    TuneScope tune_scope(tuning);
    hipStream_t s = (hipStream_t)stream;
    const int64_t zs = (int64_t)(block / sizeof(double)), mm = (int64_t)Mp * Mp;
    const double log_ratio = log(gamma / gamma_init);

    hipLaunchKernelGGL(natgrad_pad_kernel, GRIDZ(mm, n), 0, s, t, (int)M, Mp, scale, w.LSp, w.LST, w.Gp, w.gp, zs);
    TRY(CHECK_LAUNCH());
    // T2 = L_S^T (scale g_LS), P = Phi(T2), Brev = J (I + 2 gamma_t sym(P)) J
    TRY(launch_gemm_auto(mm_gemm(w.LST, w.Gp, w.T2, Mp, M, TRI_UPPER_A | TRI_LOWER_B, n, zs), false, w.ws, w.ws_elems, s));
    TRY(launch_phi_z(w.T2, Mp, w.P, n, zs, s));
    hipLaunchKernelGGL(natgrad_form_b_kernel, GRIDZ(mm, n), 0, s, (const double*)w.P, (int)M, Mp, w.Brev,
                       (const int64_t*)step_count, gamma, gamma_init, log_ratio, (int)warmup_steps, w.gam, zs);
    TRY(CHECK_LAUNCH());
    // Brev = C C^T in place, Cinv = C^-1 (the last launch of the factorisation clears Cinv above the block diagonal)
    int inv_done = 0;
    TRY(launch_potrf_z(w.Brev, Mp, Mp, M, w.Dinv, w.Ld, info, n, zs, w.Cinv, nullptr, w.ws, &inv_done, s));
    if (!inv_done) TRY(launch_trtri_z(w.Brev, Mp, Mp, w.Dinv, w.Cinv, w.Tscr, w.ws, w.ws_elems, n, zs, s));
    hipLaunchKernelGGL(natgrad_form_t_kernel, GRIDZ(mm, n), 0, s, (const double*)w.Cinv, (int)M, Mp, w.Tp, zs);
    TRY(CHECK_LAUNCH());
    // L_new = L_S T (lower x lower); the write-back reads its lower triangle only
    {
        GemmArgs g = mm_gemm(w.LSp, w.Tp, w.Lnew, Mp, M, TRI_LOWER_A | TRI_LOWER_B, n, zs);
        g.lower_out = 1;
        TRY(launch_gemm_auto(g, false, w.ws, w.ws_elems, s));
    }
    hipLaunchKernelGGL(natgrad_ltg_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)n), dim3(256), 0, s, (const double*)w.Lnew,
                       (const double*)w.gp, (int)M, Mp, w.v, zs);
    TRY(CHECK_LAUNCH());
    hipLaunchKernelGGL(natgrad_writeback_kernel, dim3((unsigned)((M + 3) / 4), (unsigned)n), dim3(256), 0, s, t,
                       (const double*)w.Lnew, (const double*)w.v, (const double*)w.gam, step_count, (int)M, Mp, zs);
    return CHECK_LAUNCH();
}

}  // extern "C"
