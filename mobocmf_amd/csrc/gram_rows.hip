// Row-side input gradient of the Gram kernels (gram.hip), gfx950: with L = sum G . K, rows [x1_m, f1_m] and columns
// [x2_n, f2_j] (column j = base row j / xdiv),
//
//   g_x1[m][k] = sum_j G[m][j] ( a1 E1 (nu f2_j f1_m + af Ef) / ls1_k^2 + a2 E2 / ls2_k^2 ) (x2_nk - x1_mk)       (kind 1)
//   g_x1[m][k] = sum_j G[m][j]   alpha E / ls_k^2 (x2_nk - x1_mk)                                                   (kind 0)
//
// the gradient with respect to the inducing inputs Z_x when the rows are the inducing points.  gram_bwd_kernel gives a data
// column to a thread; here the ownership is transposed: a THREAD owns one row m, keeps x1_m and its 2 x DB accumulators
// (sum W1 (x - z) and sum W2 (x - z); the 1 / ls^2 are applied once at the end) in registers and walks the columns, so no
// cross-lane reduction is needed.  A workgroup is 4 wavefronts on the same 64 rows; each wavefront takes `wb` base columns
// of the workgroup's chunk in tiles of 32 (replicated) columns: the G tile is loaded row-major (coalesced, 256 bytes per
// row) into LDS with a pitch of 33 doubles and read transposed -- lane m reads tile[m][c], 33 odd: the 32 lanes of a
// half-wavefront hit 32 different 8-byte bank pairs -- and the tile's x2 rows and f2 values are read from LDS as broadcasts.
// The difference x - z is formed first (as gram_bwd_kernel does): a column sitting on a row contributes with its own small
// magnitude.  The four wavefronts' sums are combined through LDS in a fixed order and written as ONE partial per (chunk,
// row, k); launch_sum_partials_multi adds the chunks.  No atomics: two launches give the same bits.
#include "common.h"

#define RR 64        // rows per workgroup (one per lane)
#define RW 4         // wavefronts per workgroup
#define RTC 32       // columns per tile
#define RPITCH 33    // doubles between two rows of the LDS tile

template <int KIND, int DB>
__global__ __launch_bounds__(RR * RW) void gram_bwd_rows_kernel(GramRowsArgs g) {
    __shared__ double tiles[RW][RR * RPITCH];
    __shared__ double xs[RW][RTC][DB];
    __shared__ double fs[RW][RTC];
    __shared__ double il1[DB], il2[DB];
    static_assert(RW * DB * 64 <= RW * RR * RPITCH, "the wavefronts' sums are combined in the tile store");
    constexpr int TILE_LOADS_IN_FLIGHT = DB <= 8 ? RR / 2 : 8;
    const int d = g.d, xdiv = g.xdiv;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double* hyp = g.hyp;
    double a1, af = 0, nu = 0, a2 = 0, ilf = 0;
    if (KIND == 0) {
        a1 = hyp[0];
        if (tid < DB) il1[tid] = tid < d ? 1.0 / hyp[1 + tid] : 0.0;
    } else {
        a1 = hyp[0]; af = hyp[1]; nu = hyp[2]; a2 = hyp[3]; ilf = 1.0 / hyp[4];
        if (tid < DB) { il1[tid] = tid < d ? 1.0 / hyp[5 + tid] : 0.0; il2[tid] = tid < d ? 1.0 / hyp[5 + d + tid] : 0.0; }
    }
    const int64_t row0 = (int64_t)blockIdx.y * RR;
    const int64_t m = row0 + lane;
    const bool rowreal = m < g.n1;
    // columns k >= d of the DB-wide rows are zero (z, the staged x rows, the inverse lengthscales): no test per column
    double z[DB], A1[DB], A2[KIND == 1 ? DB : 1];
#pragma unroll
    for (int k = 0; k < DB; ++k) {
        z[k] = (rowreal && k < d) ? g.x1[m * d + k] : 0.0;
        A1[k] = 0.0;
        if (KIND == 1) A2[k] = 0.0;
    }
    const double zfm = (KIND == 1 && rowreal) ? g.f1[m] : 0.0;
    // this wavefront's base columns [b0, b1) and columns [c0, c1)
    int64_t b0 = ((int64_t)blockIdx.x * RW + w) * g.wb;
    if (b0 > g.nbase2) b0 = g.nbase2;
    const int64_t b1 = b0 + g.wb < g.nbase2 ? b0 + g.wb : g.nbase2;
    const int64_t c0 = b0 * xdiv, c1 = b1 * xdiv;
    const int ntiles = (g.wb * xdiv + RTC - 1) / RTC;      // the same for every wavefront: the barriers below are uniform
    double* tile = tiles[w];
    for (int t = 0; t < ntiles; ++t) {
        const int64_t t0 = c0 + (int64_t)t * RTC;
        const int ncols = t0 < c1 ? (int)(c1 - t0 < RTC ? c1 - t0 : RTC) : 0;
        // a tile overlaps at most two 128-column blocks of G; one with no active column is neither read nor walked
        bool act = ncols > 0;
        if (act && g.colact) act = g.colact[t0 >> 7] != 0 || g.colact[(t0 + ncols - 1) >> 7] != 0;
        const int64_t nb0 = t0 / xdiv;      // first base column of the tile
        __syncthreads();                    // the previous tile has been read (and il1 / il2 written)
        if (act) {
            for (int e = lane; e < RTC * DB; e += 64) {
                const int j = e / DB, k = e % DB;
                const int64_t n0 = nb0 + j;
                xs[w][j][k] = (n0 < b1 && k < d) ? g.x2[n0 * d + k] : 0.0;
            }
            if (KIND == 1 && lane < RTC) fs[w][lane] = lane < ncols ? g.f2[t0 + lane] : 0.0;
            const int col = lane & (RTC - 1), rs = lane >> 5;
            const bool colok = col < ncols && (!g.colact || g.colact[(t0 + col) >> 7] != 0);
            const double* gp = g.G + (row0 + rs) * g.ldk + t0 + col;
            // all 32 row loads of the tile in flight where the registers allow it (the accumulators of the 32-wide
            // instantiation leave room for eight)
#pragma unroll TILE_LOADS_IN_FLIGHT
            for (int i = 0; i < RR / 2; ++i) {
                const int r = 2 * i + rs;
                tile[r * RPITCH + col] = (colok && row0 + r < g.n1) ? gp[(int64_t)(2 * i) * g.ldk] : 0.0;
            }
        }
        __syncthreads();
        if (!act) continue;
        const double* trow = tile + lane * RPITCH;
        int cc = 0, j = 0;
        int s = (int)(t0 - nb0 * xdiv);     // replica of the tile's first column (a base row may straddle two tiles: its
        while (cc < ncols) {                // columns in each tile are walked, and added, on their own)
            const int seg = xdiv - s < ncols - cc ? xdiv - s : ncols - cc;
            double d1 = 0.0, d2 = 0.0;
#pragma unroll
            for (int k = 0; k < DB; ++k) {
                const double df = xs[w][j][k] - z[k];
                const double t1 = df * il1[k];
                d1 += t1 * t1;
                if (KIND == 1) { const double t2 = df * il2[k]; d2 += t2 * t2; }
            }
            const double E1 = exp(-0.5 * d1);
            double W1, W2 = 0.0;
            if (KIND == 0) {
                double Gsum = 0.0;
                for (int r = 0; r < seg; ++r) Gsum += trow[cc + r];
                W1 = Gsum * a1 * E1;
            } else {
                const double E2 = exp(-0.5 * d2);
                double G2s = 0.0, S1 = 0.0, S2 = 0.0;
                // four replicas at a time: their exponentials are independent and overlap (the sums keep the replicas' order)
                int r = 0;
                for (; r + 4 <= seg; r += 4) {
                    double Gv[4], Ef[4], fn[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        Gv[u] = trow[cc + r + u];
                        fn[u] = fs[w][cc + r + u];
                        const double fd = (fn[u] - zfm) * ilf;
                        Ef[u] = exp(-0.5 * fd * fd);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        G2s += Gv[u];
                        S1 += Gv[u] * fn[u];
                        S2 += Gv[u] * Ef[u];
                    }
                }
                for (; r < seg; ++r) {
                    const double Gv = trow[cc + r], fn = fs[w][cc + r];
                    const double fd = (fn - zfm) * ilf;
                    G2s += Gv;
                    S1 += Gv * fn;
                    S2 += Gv * exp(-0.5 * fd * fd);
                }
                W1 = a1 * E1 * (nu * zfm * S1 + af * S2);
                W2 = G2s * a2 * E2;
            }
#pragma unroll
            for (int k = 0; k < DB; ++k) {
                const double df = xs[w][j][k] - z[k];
                A1[k] += W1 * df;
                if (KIND == 1) A2[k] += W2 * df;
            }
            cc += seg;
            ++j;
            s = 0;
        }
    }
    // the four wavefronts' sums, (w0 + w1) + (w2 + w3), one partial per (chunk, row, k)
    __syncthreads();
    double* comb = &tiles[0][0];      // [RW][DB][64]
#pragma unroll
    for (int k = 0; k < DB; ++k) {
        double v = A1[k] * (il1[k] * il1[k]);
        if (KIND == 1) v += A2[k] * (il2[k] * il2[k]);
        comb[(w * DB + k) * 64 + lane] = v;
    }
    __syncthreads();
    const double sc = g.symmetric ? 2.0 : 1.0;      // K_mm: the column side equals the row side (G symmetric)
    for (int e = tid; e < d * 64; e += RR * RW) {
        const int k = e >> 6, r = e & 63;
        if (row0 + r < g.n1) {
            const double v = (comb[(0 * DB + k) * 64 + r] + comb[(1 * DB + k) * 64 + r]) +
                             (comb[(2 * DB + k) * 64 + r] + comb[(3 * DB + k) * 64 + r]);
            g.part[((int64_t)blockIdx.x * g.n1 + row0 + r) * d + k] = sc * v;
        }
    }
}

// Base columns per wavefront: tiles of 32 columns, one per wavefront, doubled while the grid has more than 2048 workgroups
// (every chunk costs n1 d doubles of partials and one addend of the reduction).
void gram_rows_geometry(int64_t n1, int64_t nbase2, int xdiv, int64_t* chunks, int* groups, int* wb) {
    const int64_t gr = (n1 + RR - 1) / RR;
    int tiles = 1;
    int64_t b, ch;
    for (;;) {
        b = ((int64_t)RTC * tiles + xdiv - 1) / xdiv;
        ch = (nbase2 + RW * b - 1) / (RW * b);
        if (ch * gr <= 2048 || tiles >= 64) break;
        tiles *= 2;
    }
    *chunks = ch; *groups = (int)gr; *wb = (int)b;
}

int launch_gram_bwd_rows(const GramRowsArgs& g0, hipStream_t s) {
    GramRowsArgs g = g0;
    if (g.d < 1 || g.d > 32 || g.xdiv < 1 || g.n1 < 1 || g.nbase2 < 1) return MOBOCMF_BAD_ARG;
    int64_t chunks;
    int groups;
    gram_rows_geometry(g.n1, g.nbase2, g.xdiv, &chunks, &groups, &g.wb);
    if (chunks > 0x7fffffff || groups > 65535) return MOBOCMF_BAD_ARG;
    const dim3 grid((unsigned)chunks, (unsigned)groups, 1);
    const int db = g.d <= 2 ? 2 : (g.d <= 8 ? 8 : 32);
#define GR(K, D) hipLaunchKernelGGL((gram_bwd_rows_kernel<K, D>), grid, dim3(RR * RW), 0, s, g)
    if (g.kind == 0) { if (db == 2) GR(0, 2); else if (db == 8) GR(0, 8); else GR(0, 32); }
    else { if (db == 2) GR(1, 2); else if (db == 8) GR(1, 8); else GR(1, 32); }
#undef GR
    return hipGetLastError() == hipSuccess ? MOBOCMF_OK : MOBOCMF_HIP_ERROR;
}
