"""References and direct C-ABI callers shared by the kernel conformance tests ("Kernel conformance tests").

Three things live here so that the CPU proof (tests/test_kernel_reference_cpu.py) and the GPU tests use the same objects:

* exact inputs -- integer operands in [-4, 4], optionally times powers of two along dimensions an output does not sum over.
  Every product and every partial sum of them is an integer (times one power of two) below 2^53, hence exactly
  representable: the float64 result does not depend on summation order, FMA use, k-slicing, slab reduction or tile shape,
  and a correct kernel is BITWISE equal to the reference under every tuning;
* high-precision references (numpy.longdouble with a 64-bit significand, else mpmath) for inexact data, with the a-priori
  componentwise bounds the rounding tests assert;
* callers of the product / Gram / ELBO entry points that pass pointers, leading dimensions and tunings through unchanged
  (functional._prep would make every operand contiguous).

At the end: the variational layer as a whole -- well-conditioned cases, a dtype-generic reference with its magnitude shadow,
the measured constants of the layer bound and direct callers of the whole-call and the split layer entry points; then the
whole model of the one-launch steps as a composition of the same layer statements, with its composed shadow, its cases,
its measured constants per depth and the direct callers of mobocmf_tiny_elbo_step / mobocmf_coop_elbo_step.
"""
import ctypes

import numpy as np
import torch

U = 2.0 ** -53                       # unit roundoff of float64
NAN = float("nan")

# ------------------------------------------------------------------------------------------------------- shapes (Mr, Nc, Kd)
# Product families of mobocmf_gemm_f64 and the tuning that forces each (gemm_f64.hip: launch_gemm_auto).  The tiled shapes
# miss the whole-block panel kernel by their size (Kd no multiple of 128, or Mr > 512); the square one needs small_panel_max.
TILED = dict(small_gemm_max=16, mid_gemm_max=0)
GEMM_FAMILIES = {
    "small": [((16, 16, 16), {}), ((48, 32, 80), {}), ((384, 384, 384), {})],
    "mid4": [(s, dict(mid_gemm_waves=4)) for s in ((512, 512, 512), (64, 448, 128), (1024, 64, 192), (640, 640, 640))],
    "mid8": [(s, dict(mid_gemm_waves=8)) for s in ((512, 512, 512), (64, 448, 128), (1024, 64, 192), (640, 640, 640))],
    "mid32": [(s, dict(mid_gemm_waves=32)) for s in ((512, 512, 512), (64, 448, 128), (1024, 64, 192), (640, 640, 640))],
    "tiled": [((128, 128, 16), TILED), ((256, 384, 144), TILED), ((1152, 128, 128), TILED), ((1152, 128, 128), {}),
              ((256, 256, 256), dict(TILED, small_panel_max=16))],
}
# The whole-block panel kernel under the plain entry point, at widths below one 128-column tile: every other kernel declines
# these (A B form only).  GEMM_DECLINED (shape, trans_b, tuning): no kernel takes them, MOBOCMF_BAD_ARG.
GEMM_PANEL = [((512, 48, 512), {}), ((256, 48, 256), TILED), ((128, 16, 128), TILED)]
GEMM_DECLINED = [((512, 48, 512), 1, {}), ((1152, 64, 1152), 0, {}), ((256, 48, 256), 0, dict(TILED, small_panel_max=16)),
                 ((64, 128, 128), 0, TILED), ((512, 48, 520), 0, {})]
BAD_ARG = 1                             # MOBOCMF_BAD_ARG (include/mobocmf_hip.h)
TRI_FLAGS = (0, 1, 2, 4, 8, 1 | 4, 1 | 8, 2 | 4)      # every combination the chain, the Cholesky and natgrad launch
EPI_MR = (128, 256, 384, 640)                           # Kd = Mr; 384 and 640: an odd number of row blocks
EPI_NC_TILED = (128, 384)
EPI_NC_PANEL = (16, 48, 144, 128, 384)
SYRK_MR = (128, 256, 384, 640)
SYRK_KD = (128, 256, 1024, 2176)


def gemm_shapes():
    return sorted({s for fam in GEMM_FAMILIES.values() for s, _ in fam} | {s for s, _ in GEMM_PANEL})


# ------------------------------------------------------------------------------------------------------------ exact inputs
def exact_ints(shape, seed):
    """Integers in [-4, 4] as int64."""
    return np.random.default_rng(seed).integers(-4, 5, size=shape).astype(np.int64)


def tile_scales(n, block, seed):
    """2^e per index, e in [-100, 100]: constant on blocks of ``block`` indices, neighbouring blocks >= 2^160 apart (even
    blocks 2^80..2^100, odd blocks 2^-100..2^-80) -- a block that is wrong but quiet cannot hide behind a loud one."""
    rng = np.random.default_rng(seed)
    nb = (n + block - 1) // block
    e = np.where(np.arange(nb) % 2 == 0, rng.integers(80, 101, nb), -rng.integers(80, 101, nb))
    return np.exp2(np.repeat(e, block)[:n].astype(np.float64))


def tri_mask(n, lower):
    i = np.arange(n)
    return (i[:, None] >= i[None, :]) if lower else (i[:, None] <= i[None, :])


def gemm_operands(Mr, Nc, Kd, tri, seed=0):
    """Integer A [Mr x Kd] and logical B [Kd x Nc] with the zeros of the triangles ``tri`` names (int64)."""
    A, B = exact_ints((Mr, Kd), seed + 1), exact_ints((Kd, Nc), seed + 2)
    if tri & 3:
        assert Mr == Kd
        A = A * tri_mask(Mr, bool(tri & 1))
    if tri & 12:
        assert Kd == Nc
        B = B * tri_mask(Kd, bool(tri & 4))
    return A, B


def tri_ok(tri, Mr, Nc, Kd):
    return (not (tri & 3) or Mr == Kd) and (not (tri & 12) or Kd == Nc)


def exactness_margin(absA, absB):
    """max_i sum_k |a_ik| max_j |b_kj| >= sum_k |a_ik||b_kj| for every output -- an upper bound of EVERY partial sum in EVERY
    order; the result is exact while it stays below 2^53."""
    return int((np.abs(absA).astype(np.int64) @ np.abs(absB).astype(np.int64).max(1)).max())


def imatmul(A, B):
    """Exact int64 product (torch's integer matmul: numpy's runs one scalar loop)."""
    return (torch.from_numpy(np.ascontiguousarray(A, dtype=np.int64)) @ torch.from_numpy(np.ascontiguousarray(B, dtype=np.int64))).numpy()


def fmatmul(A, B):
    """The same product through float64 BLAS, as int64: tests/test_kernel_reference_cpu.py proves it bitwise equal to
    imatmul for every shape used (that IS the exactness condition), so the references below take the fast one."""
    return (np.asarray(A, np.float64) @ np.asarray(B, np.float64)).astype(np.int64)


def unused_block_poison(a, lower, block=128):
    """Copy of the float matrix ``a`` (a triangular operand stored with its zeros) with NaN in every block x block block
    that lies wholly in the unused triangle -- where the contract of mobocmf_gemm_f64 says nothing is read."""
    a = a.copy()
    n = a.shape[0]
    bi = np.arange(n) // block
    beyond = (bi[:, None] < bi[None, :]) if lower else (bi[:, None] > bi[None, :])
    a[beyond] = np.nan
    return a


EPI_ALPHA = -0.5


def epilogue_case(Mr, Nc, tri, seed=0, scaled=None):
    """Operands of mobocmf_gemm_f64_epilogue at Kd = Mr as (integers, scales): A triangular per ``tri`` (1 lower, 2 upper, 0
    dense), B, Aaux [Mr x Nc], avec [Mr], bscale / gmu / cgv [Nc].  ``scaled``: None | 'rows' (A, avec, Aaux rows times
    2^e per 128-row block: every output that does not sum over rows -- C, the row dots -- stays exact) | 'cols' (B, gmu, cgv
    columns times 2^e per 128-column block: C and the column statistics stay exact)."""
    c = dict(A=gemm_operands(Mr, Nc, Mr, tri & 3, seed)[0], B=exact_ints((Mr, Nc), seed + 2),
             Aaux=exact_ints((Mr, Nc), seed + 3), avec=exact_ints(Mr, seed + 4), bscale=exact_ints(Nc, seed + 5),
             gmu=exact_ints(Nc, seed + 6), cgv=exact_ints(Nc, seed + 7))
    c["rs"] = tile_scales(Mr, 128, seed + 8) if scaled == "rows" else np.ones(Mr)
    c["cs"] = tile_scales(Nc, 128, seed + 9) if scaled == "cols" else np.ones(Nc)
    return c


def epilogue_inputs(c):
    """The float64 operands a kernel is given (integers times their power-of-two scales: exact)."""
    f = lambda a: a.astype(np.float64)
    rs, cs = c["rs"], c["cs"]
    return dict(A=f(c["A"]) * rs[:, None], B=f(c["B"]) * cs[None, :], Aaux=f(c["Aaux"]) * rs[:, None], avec=f(c["avec"]) * rs,
                bscale=f(c["bscale"]), gmu=f(c["gmu"]) * cs, cgv=f(c["cgv"]) * cs)


def epilogue_ref_int(c, epi):
    """Exact integer results, scales left out: 2 C, and for epi 1 (4 colsq, 2 coldot), for epi 2 the row dots (alpha = -1/2)."""
    AB = fmatmul(c["A"], c["B"])
    if epi < 2:
        C2 = -AB
        return dict(C2=C2, colsq4=(C2 * C2).sum(0), coldot2=c["avec"] @ C2)
    C2 = -c["bscale"][None, :] * AB + 2 * c["avec"][:, None] * c["gmu"][None, :] - 4 * c["Aaux"] * c["cgv"][None, :]
    return dict(C2=C2, rowdot=c["Aaux"] @ c["gmu"])


def epilogue_ref(c, epi):
    """The same as float64 with the scales applied (exact: integers below 2^53 times powers of two)."""
    r = epilogue_ref_int(c, epi)
    f = lambda a: a.astype(np.float64)
    rs, cs = c["rs"], c["cs"]
    out = dict(C=f(r["C2"]) * 0.5 * rs[:, None] * cs[None, :])
    if epi == 1:
        out["colsq"] = f(r["colsq4"]) * 0.25 * cs * cs
        out["coldot"] = f(r["coldot2"]) * 0.5 * cs
    if epi == 2:
        out["rowdot"] = f(r["rowdot"]) * rs
    return out


def syrk_case(Mr, Kd, seed=0, kact=None, scaled=False):
    """A [Mr x Kd], w [Kd] integers (w zero on the 128-blocks ``kact`` marks inactive), row scales of A."""
    A, w = exact_ints((Mr, Kd), seed + 11), exact_ints(Kd, seed + 12)
    if kact is not None:
        w = w * np.repeat(np.asarray(kact, np.int64), 128)
    return dict(A=A, w=w, rs=tile_scales(Mr, 128, seed + 13) if scaled else np.ones(Mr))


def syrk_ref(c):
    H = fmatmul(c["A"] * c["w"][None, :], c["A"].T)
    return H.astype(np.float64) * c["rs"][:, None] * c["rs"][None, :]


ACTIVITY = {"all": lambda n: [1] * n, "none": lambda n: [0] * n, "first": lambda n: [1] + [0] * (n - 1),
            "last": lambda n: [0] * (n - 1) + [1]}


# ------------------------------------------------------------------------------------------- high-precision references
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63


def matmul_hp(A, B):
    """A @ B in extended precision, returned as longdouble (error K 2^-64 |A||B|: 2^-11 of the float64 bound)."""
    if HAVE_LONGDOUBLE:
        return np.asarray(A, np.longdouble) @ np.asarray(B, np.longdouble)
    import mpmath
    mpmath.mp.dps = 50
    C = mpmath.matrix(np.asarray(A, np.float64).tolist()) * mpmath.matrix(np.asarray(B, np.float64).tolist())
    return np.array(C.tolist(), dtype=np.float64).astype(np.longdouble)


def ld(a):
    return np.asarray(a, np.longdouble)


def componentwise_ok(got, ref, R, n_ops):
    """|got - ref| <= (n_ops + 2) 2^-53 R elementwise; returns (ok, worst ratio err / (2^-53 R))."""
    err = np.abs(ld(got) - ref)
    bound = (n_ops + 2) * ld(U) * R
    ratio = float(np.max(np.where(R > 0, err / np.where(R > 0, ld(U) * R, 1), np.where(err > 0, np.inf, 0))))
    return bool(np.all(err <= bound)), ratio


# ---- Gram kernels (include/mobocmf_hip.h, mobocmf_layer_desc):
#   kind 0  k = alpha exp(-arg1),                                   arg = 1/2 sum_k ((x_k - z_k) / ls_k)^2
#   kind 1  k = a1 E1 nu f f' + a1 E1 af Ef + a2 E2                 (three terms, exponents arg1, arg1 + argf, arg2)
# Per-element bound c (2 + |arg|) 2^-53 |term|, summed over the terms.  c is MEASURED on the float64 CPU restatement
# (oracle/mfdgp_oracle.gram) against the longdouble reference on the inputs of gram_case below, by
# tests/test_kernel_reference_cpu.py::test_gram_constant_is_the_measured_one: worst ratio err / ((2 + |arg|) 2^-53 sum|term|)
# over kind 0 / 1, d in {1, 2, 3, 8, 9, 32}, measured 7.24 (kind 0, d = 2, where the restatement's x / ls - z / ls cancels; 2.9 to
# 4.6 at the other d), recorded rounded up as GRAM_RATIO_MEASURED; the device uses another summation order, FMA and
# precomputed reciprocal lengthscales, each worth a few u |arg|, hence c = 4 x that = 29.2.
GRAM_RATIO_MEASURED = 7.3
GRAM_C = 4.0 * GRAM_RATIO_MEASURED
GRAM_D = (1, 2, 3, 8, 9, 32)
GRAM_XDIV = (1, 3, 8, 16, 48)
GRAM_N1 = (1, 31, 33)
GRAM_NBASE2 = (1, 127, 129)


def gram_case(kind, d, n1, nbase2, xdiv, seed=0):
    """Inputs of one Gram case (float64 numpy): lengthscales log-uniform in [0.05, 1.5] (d <= 3) or [0.05, 0.08] (|arg|
    reaches the thousands at d = 32), some columns sitting on rows of x1 so that entries of order one exist beside the underflowing ones."""
    rng = np.random.default_rng(1000 * kind + 10 * d + seed)
    x1 = rng.random((n1, d))
    x2 = rng.random((nbase2, d))
    k = min(n1, nbase2, 5)
    x2[:k] = x1[:k] + 1e-3 * rng.standard_normal((k, d))
    hi = 1.5 if d <= 3 else 0.08                 # many short lengthscales at large d: exponents past float64's range
    ls = lambda n: np.exp(rng.uniform(np.log(0.05), np.log(hi if n > 1 else 1.5), n))
    if kind == 0:
        hyp = np.concatenate([[0.7 + rng.random()], ls(d)])
        return dict(x1=x1, f1=None, x2=x2, f2=None, hyp=hyp)
    hyp = np.concatenate([[0.6 + rng.random(), 0.5 + rng.random(), 0.5 + rng.random(), 0.05 + 0.1 * rng.random()],
                          ls(1), ls(d), ls(d)])
    return dict(x1=x1, f1=0.5 * rng.standard_normal(n1), x2=x2, f2=rng.standard_normal(nbase2 * xdiv), hyp=hyp)


def gram_hp(kind, c, xdiv):
    """(K, sum_t (2 + |arg_t|) |term_t|, knn) in longdouble: rows = x1, columns = x2 rows replicated xdiv times."""
    assert HAVE_LONGDOUBLE
    return _gram(kind, c, xdiv, ld)[:3]


def _gram(kind, c, xdiv, T):
    """gram_hp's statements in the number format ``T`` converts to, and sum_t |term_t| as a fourth result."""
    x1, x2, hyp = T(c["x1"]), T(c["x2"]), T(c["hyp"])
    d = x1.shape[1]
    half = T(0.5)

    def arg(a, b, ls):
        t = (a[:, None, :] - b[None, :, :]) / ls
        return half * (t * t).sum(-1)

    if kind == 0:
        a1 = np.repeat(arg(x1, x2, hyp[1:1 + d]), xdiv, axis=1)
        K = hyp[0] * np.exp(-a1)
        return K, (2 + a1) * np.abs(K), np.full(K.shape[1], hyp[0]), np.abs(K)
    a1_, af_, nu, a2_, lsf = hyp[:5]
    f1, f2 = T(c["f1"]), T(c["f2"])
    g1 = np.repeat(arg(x1, x2, hyp[5:5 + d]), xdiv, axis=1)
    g2 = np.repeat(arg(x1, x2, hyp[5 + d:5 + 2 * d]), xdiv, axis=1)
    gf = half * ((f1[:, None] - f2[None, :]) / lsf) ** 2
    T1 = a1_ * np.exp(-g1) * nu * f1[:, None] * f2[None, :]
    T2 = a1_ * np.exp(-(g1 + gf)) * af_
    T3 = a2_ * np.exp(-g2)
    W = (2 + g1) * np.abs(T1) + (2 + g1 + gf) * np.abs(T2) + (2 + g2) * np.abs(T3)
    return T1 + T2 + T3, W, a1_ * (nu * f2 * f2 + af_) + a2_, np.abs(T1) + np.abs(T2) + np.abs(T3)


def gram_violations(got, K, W, c=None):
    """Elements outside the bound: c 2^-53 W where the reference is >= 1e-290, else |got - ref| <= 1e-300.  Returns
    (count, worst ratio err / (2^-53 W) over the regular elements)."""
    c = GRAM_C if c is None else c
    err = np.abs(ld(got) - K)
    tiny = np.abs(K) < ld(1e-290)
    ratio = np.where(tiny, 0, err / np.where(tiny, 1, ld(U) * W))
    bad = np.where(tiny, err > ld(1e-300), ratio > c)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0


# ---- Gram backward (gram.hip: gram_bwd_kernel + sum_partials_multi_kernel; include/mobocmf_hip.h, mobocmf_gram_backward)
# With L = sum G . K + sum gknn . knn every output component theta is a sum of ADDENDS G_mn dterm_mn/dtheta over (m, n, term)
# (plus gknn_n dknn_n/dtheta, exponent 0), the three terms and their exponents being those of gram_hp.  The addends cancel
# (sum |addend| / |sum| of 20 .. 2e5), so the bound is on the sum of their magnitudes, never on the value:
#     |got - ref| <= 2^-53 (c W + D A),    A = sum |G| |dterm/dtheta|,    W = sum (2 + |arg_term|) |G| |dterm/dtheta|.
# c W covers the evaluation of each addend (exponent, exp, the products); c = GRAM_BWD_C = 4 x GRAM_BWD_RATIO_MEASURED, the
# ratio being the worst err / (2^-53 W) of the float64 CPU restatement gram_bwd_f64 below (these statements in float64 with
# numpy's pairwise sums) over the cases of tests/test_kernel_reference_cpu.py::test_gram_backward_constant_is_the_measured_one,
# recorded rounded up.  Measured 4.05 (kind 1, d = 32; 0.7 .. 1.4 at d <= 3, 2.3 .. 2.9 at d = 8, 9).  Autograd over the oracle
# is NOT the restatement: it forms x / ls - z / ls, which loses 2 u |x| / |x - z| of the d/dx and d/dls addends -- err / (2^-53 W)
# of 1e3 .. 2e4 at gram_case's near-coincident columns -- while the device, like gram_bwd_f64, takes the difference first.
# D A covers the additions on the device, first order, worst case: D (gram_bwd_depth) is the number of roundings a partial sum
# holding the addend can pass through.
GRAM_BWD_RATIO_MEASURED = 4.1
GRAM_BWD_C = 4.0 * GRAM_BWD_RATIO_MEASURED
GRAM_BWD_NBASE2 = (1, 127, 129, 257)
GRAM_BWD_OUTPUTS = ("hyp", "g_f1", "g_f2", "g_x2")


def gram_bwd_inputs(n1, Np, seed=0, active=None):
    """(G [n1 x Np], gknn [Np]) standard normal; gknn zero in the inactive 128-column blocks, as a layer's is."""
    rng = np.random.default_rng(77 + seed)
    G, gk = rng.standard_normal((n1, Np)), rng.standard_normal(Np)
    if active is not None:
        gk = np.where(column_mask(active, Np), gk, 0.0)
    return G, gk


def column_mask(active, Np):
    """bool [Np] from one activity word per 128 columns."""
    assert len(active) == (Np + 127) // 128
    return np.repeat(np.asarray(active) != 0, 128)[:Np]


def sum_form(P, length):
    """The form launch_sum_partials_multi picks for a task of P partials and ``length`` outputs: 0 serial (one thread adds
    the P partials in turn), 1 wide (P >= 64 and length <= 4096: 256 threads stride over the partials, a wavefront butterfly,
    four wavefront sums), 2 four-way (P >= 16: four threads take every fourth partial, combined pairwise)."""
    return 1 if (P >= 64 and length <= 4096) else (2 if P >= 16 else 0)


def sum_depth(P, length):
    """Additions a partial can pass through in that reduction.  serial: v = 0, v += part[p]: P.  wide: ceil(P / 256) strided
    adds, six butterfly steps, sh[0] + sh[1] + sh[2] + sh[3]: ceil(P / 256) + 9.  four-way: ceil(P / 4) strided adds, then
    (s0 + s1) + (s2 + s3): ceil(P / 4) + 2."""
    form = sum_form(P, length)
    return -(-P // 256) + 9 if form == 1 else (-(-P // 4) + 2 if form == 2 else P)


GRAM_BWD_MULS = 6


def gram_bwd_tasks(kind, d, n1, nbase2, xdiv, geometry):
    """{output: (P, length)} of the reduction tasks mobocmf_gram_backward launches, from the geometry of the size query."""
    gx, gy, _ = geometry
    t = {"hyp": (gx * gy, 1 + d if kind == 0 else 5 + 2 * d), "g_x2": (gy, nbase2 * d)}
    if kind == 1:
        t["g_f2"], t["g_f1"] = (gy, nbase2 * xdiv), (gx, n1)
    return t


def gram_bwd_depth(kind, d, n1, nbase2, xdiv, geometry):
    """D per output: the roundings a partial sum that holds a given addend can pass through on the device, read off
    gram_bwd_kernel (gm = geometry[2] rows of x1 per workgroup, walked serially by a thread that owns one base row and its
    xdiv replicas) and sum_partials_multi_kernel.  Additions:
      hyp   the replica sums (Gsum; S1 .. S4, G2s): xdiv; nu zf S1 + af S2: 1; the thread's accumulator (s_a1 .., aL1, aL2)
            over its rows: gm (the k_nn addends enter it first: xdiv + gm, no more); wave_sum: 6; red[0] + red[1]: 1; the
            reduction over grid x * grid y partials.                                       xdiv + gm + 8 + sum_depth
      g_f1  the replica sums: xdiv; aE1 nu S1 + c_b S3: 1; wave_sum: 6; the two wavefronts' LDS atomic adds into a zeroed
            slot: 2; the reduction over grid x partials.                                   xdiv + 9 + sum_depth
      g_f2  Gv c_a - T c_b: 1; the general path's acc = 0 + that: 1; the column's accumulator over the rows: gm; the k_nn
            term: 1; the reduction over grid y partials.                                   gm + 3 + sum_depth
      g_x2  the replica sums and nu zf S1 + af S2: xdiv + 1; W1 t1 il1 + W2 t2 il2: 1; aX over the rows: gm; the reduction
            over grid y partials.                                                          xdiv + gm + 2 + sum_depth
    Products applied to a sum of addends round it once more each; the most any output sees is six (aE1 * (nu * zf * S1 + ..),
    W1 * t1 * t1, the final * il1): GRAM_BWD_MULS, added to every D.  Products inside one addend belong to c W."""
    gm = geometry[2]
    tasks = gram_bwd_tasks(kind, d, n1, nbase2, xdiv, geometry)
    chain = {"hyp": xdiv + gm + 8, "g_f1": xdiv + 9, "g_f2": gm + 3, "g_x2": xdiv + gm + 2}
    return {k: chain[k] + GRAM_BWD_MULS + sum_depth(*pl) for k, pl in tasks.items()}


def _gram_bwd(kind, c, xdiv, G, gknn, active, T, sf2=None):
    """The gradients and their weights in the number format ``T`` converts to: {output: (value, W, A)}.  ``sf2`` [nbase2 xdiv]
    (kind 1, the model's composed shadow): f2 itself carries an error of u sf2, so every addend |G| |d term / d theta| of W and
    A is joined by |G| |d^2 term / d theta d f2| sf2; the values are untouched."""
    x1, x2, hyp = T(c["x1"]), T(c["x2"]), T(c["hyp"])
    n1, d = x1.shape
    nb = x2.shape[0]
    Np = nb * xdiv
    G = T(G)                                                           # (a longdouble G -- the layer reference's dK -- stays one)
    assert G.shape == (n1, Np)
    if active is not None:
        G = np.where(column_mask(active, Np)[None, :], G, T(0.0))     # inactive blocks may hold NaN: they count as zero
    G = G.reshape(n1, nb, xdiv)
    aG = np.abs(G)
    Gs, aGs = G.sum(2), aG.sum(2)
    half = T(0.5)
    diff = [x1[:, None, k] - x2[None, :, k] for k in range(d)]         # d matrices n1 x nb

    def arg(ls):
        s = 0
        for k in range(d):
            t = diff[k] / ls[k]
            s = s + t * t
        return half * s

    def red(terms, axes, extra=()):
        """terms: (signed weight G or Gs, its magnitude, d term / d theta, 2 + |arg|) -> (value, W, A) summed over ``axes``."""
        v = sum((g * dt).sum(axes) for g, _, dt, _ in terms)
        A = sum((a * np.abs(dt)).sum(axes) for _, a, dt, _ in terms)
        W = sum((w * a * np.abs(dt)).sum(axes) for _, a, dt, w in terms)
        for a, dt, w in extra:                                         # (magnitude, d / d f2 of an addend's factor, 2 + |arg|)
            A = A + (a * np.abs(dt)).sum(axes)
            W = W + (w * a * np.abs(dt)).sum(axes)
        return [v, W, A]

    ALL2, ALL3 = (0, 1), (0, 1, 2)
    if kind == 0:
        alpha, ls = hyp[0], hyp[1:1 + d]
        g1 = arg(ls)
        E, w = np.exp(-g1), 2 + g1
        K = alpha * E
        hy = [red([(Gs, aGs, E, w)], ALL2)]
        gx = []
        for k in range(d):
            t = diff[k] / ls[k]
            hy.append(red([(Gs, aGs, K * t * t / ls[k], w)], ALL2))
            gx.append(red([(Gs, aGs, K * diff[k] / (ls[k] * ls[k]), w)], 0))
        out = {"hyp": tuple(np.array([h[i] for h in hy], dtype=x1.dtype) for i in range(3)),
               "g_x2": tuple(np.stack([g[i] for g in gx], 1) for i in range(3))}
        return _gram_bwd_knn(kind, c, out, gknn, T)
    a1, af, nu, a2, lsf = hyp[:5]
    ls1, ls2 = hyp[5:5 + d], hyp[5 + d:5 + 2 * d]
    f1, f2 = T(c["f1"]), T(c["f2"]).reshape(nb, xdiv)
    g1, g2 = arg(ls1), arg(ls2)
    E1, E2 = np.exp(-g1)[:, :, None], np.exp(-g2)
    fdif = f2[None, :, :] - f1[:, None, None]
    gf = half * (fdif / lsf) ** 2
    Ef = np.exp(-gf)
    p = f1[:, None, None] * f2[None, :, :]
    w1 = (2 + g1)[:, :, None] + 0 * gf
    w2, w3 = w1 + gf, 2 + g2
    T1, T2, T3 = a1 * E1 * nu * p, a1 * E1 * af * Ef, a2 * E2
    e0 = e1 = e2 = e4 = xg1 = xg2 = ()
    if sf2 is not None:
        # d / d f2 of every factor that holds f2: p = f1 f2 -> f1; Ef -> -Ef rr with rr = (f2 - f1) / lsf^2; the lsf addend
        # T2 (f2 - f1)^2 / lsf^3 and the f addends T2 rr by the product rule, each part taken by its magnitude
        aS = aG * T(sf2).reshape(nb, xdiv)[None, :, :]
        f1b, rr = f1[:, None, None] + 0 * gf, fdif / (lsf * lsf)
        e0 = ((aS, E1 * nu * f1b, w1), (aS, E1 * af * Ef * rr, w2))
        e1 = ((aS, a1 * E1 * Ef * rr, w2),)
        e2 = ((aS, a1 * E1 * f1b, w1),)
        e4 = ((aS, T2 * 2 * fdif / lsf ** 3, w2), (aS, T2 * rr * (2 * gf) / lsf, w2))
        xg2 = ((aS, T2 / (lsf * lsf), w2), (aS, T2 * rr * rr, w2))
        xg1 = ((aS, a1 * E1 * nu + 0 * gf, w1),) + xg2
    hy = [red([(G, aG, E1 * nu * p, w1), (G, aG, E1 * af * Ef, w2)], ALL3, e0),
          red([(G, aG, a1 * E1 * Ef, w2)], ALL3, e1),
          red([(G, aG, a1 * E1 * p, w1)], ALL3, e2),
          red([(Gs, aGs, E2, w3)], ALL2),
          red([(G, aG, T2 * (2 * gf) / lsf, w2)], ALL3, e4)]
    # the x-only factors: per (row, base row) the replica sums of G (T1 + T2), of their magnitudes and of the weighted ones
    Qv, QA, QW = (G * (T1 + T2)).sum(2), (aG * (np.abs(T1) + np.abs(T2))).sum(2), (aG * (w1 * np.abs(T1) + w2 * np.abs(T2))).sum(2)
    if sf2 is not None:
        d1, d2 = np.abs(a1 * E1 * nu * f1b), np.abs(T2 * rr)
        QA, QW = QA + (aS * (d1 + d2)).sum(2), QW + (aS * (w1 * d1 + w2 * d2)).sum(2)
    R3 = aGs * np.abs(T3)
    l1, l2, gx = [], [], []
    for k in range(d):
        r1, r2 = (diff[k] / ls1[k]) ** 2 / ls1[k], (diff[k] / ls2[k]) ** 2 / ls2[k]
        l1.append([(Qv * r1).sum(), (QW * r1).sum(), (QA * r1).sum()])
        l2.append(red([(Gs, aGs, T3 * r2, w3)], ALL2))
        s1, s2 = diff[k] / (ls1[k] * ls1[k]), diff[k] / (ls2[k] * ls2[k])
        gx.append([(Qv * s1 + Gs * T3 * s2).sum(0), (QW * np.abs(s1) + w3 * R3 * np.abs(s2)).sum(0),
                   (QA * np.abs(s1) + R3 * np.abs(s2)).sum(0)])
    hy = hy + l1 + l2
    dT2 = T2 * fdif / (lsf * lsf)
    gf1 = red([(G, aG, a1 * E1 * nu * f2[None, :, :], w1), (G, aG, dT2, w2)], (1, 2), xg1)
    gf2 = [a.reshape(Np) for a in red([(G, aG, a1 * E1 * nu * f1[:, None, None] + 0 * gf, w1), (G, aG, -dT2, w2)], 0, xg2)]
    out = {"hyp": tuple(np.array([h[i] for h in hy], dtype=x1.dtype) for i in range(3)),
           "g_f1": tuple(gf1), "g_f2": tuple(gf2), "g_x2": tuple(np.stack([g[i] for g in gx], 1) for i in range(3))}
    return _gram_bwd_knn(kind, c, out, gknn, T, sf2)


def _gram_bwd_knn(kind, c, ref, gknn, T, sf2=None):
    """``ref`` (the G part) plus the addends gknn_n dknn_n / dtheta (exponent 0: weight 2), knn = alpha (kind 0) or
    a1 (nu f^2 + af) + a2: into alpha, or into a1 (two terms), af, nu, a2 and g_f2.  ``sf2``: as in _gram_bwd -- the weights
    gain |gknn| |d^2 knn / dtheta df| sf2 (``ddf``)."""
    if gknn is None:
        return ref
    gk, hyp = T(gknn), T(c["hyp"])
    ref = {k: tuple(a.copy() for a in v) for k, v in ref.items()}

    def add(o, i, dknn, ddf=None):
        v, W, A = o
        t = gk * dknn
        if i is None:
            v += t; W += 2 * np.abs(t); A += np.abs(t)
        else:
            v[i] += t.sum(); W[i] += 2 * np.abs(t).sum(); A[i] += np.abs(t).sum()
        if sf2 is not None and ddf is not None:
            e = np.abs(gk * ddf) * T(sf2)
            if i is None:
                W += 2 * e; A += e
            else:
                W[i] += 2 * e.sum(); A[i] += e.sum()

    if kind == 0:
        add(ref["hyp"], 0, 1 + 0 * gk)
        return ref
    a1, af, nu = hyp[0], hyp[1], hyp[2]
    f = T(c["f2"])
    add(ref["hyp"], 0, nu * f * f, 2 * nu * f)
    add(ref["hyp"], 0, af + 0 * gk)
    add(ref["hyp"], 1, a1 + 0 * gk)
    add(ref["hyp"], 2, a1 * f * f, 2 * a1 * f)
    add(ref["hyp"], 3, 1 + 0 * gk)
    add(ref["g_f2"], None, 2 * a1 * nu * f, 2 * a1 * nu + 0 * f)
    return ref


def gram_bwd_hp(kind, c, xdiv, G, gknn=None, active=None):
    """{output: (gradient, W, A)} in longdouble for ``c`` = gram_case(...): 'hyp' [1 + d | 5 + 2 d], 'g_f1' [n1] and 'g_f2'
    [nbase2 xdiv] (kind 1), 'g_x2' [nbase2 x d].  G [n1 x nbase2 xdiv] float64; the columns of 128-blocks that ``active`` (one
    word per block) marks inactive count as zero whatever they hold; gknn [nbase2 xdiv] or None enters at every column."""
    assert HAVE_LONGDOUBLE
    return _gram_bwd(kind, c, xdiv, G, gknn, active, ld)


def gram_bwd_hp_with_knn(kind, c, ref, gknn):
    """gram_bwd_hp(..., gknn) from ``ref`` = gram_bwd_hp(..., None) of the same case: the k_nn addends do not depend on G."""
    return _gram_bwd_knn(kind, c, ref, gknn, ld)


def gram_bwd_f64(kind, c, xdiv, G, gknn=None, active=None):
    """The same statements in float64 (numpy's pairwise sums): one of the two restatements behind GRAM_BWD_RATIO_MEASURED."""
    return _gram_bwd(kind, c, xdiv, G, gknn, active, lambda a: np.asarray(a, np.float64))


def gram_bwd_hp_blocks(kind, c, xdiv, blocks, Gb, gkb):
    """The reference of a wide launch of which only the 128-column blocks ``blocks`` (sorted) are active: Gb [n1 x 128
    len(blocks)] and gkb hold G and gknn on those columns, gknn is zero elsewhere.  Needs 128 % xdiv == 0 and a width that is a
    multiple of 128 (a block then owns whole base rows).  Returns the dict of gram_bwd_hp at the full width, zeros (value and
    weights) outside the blocks."""
    nb = c["x2"].shape[0]
    Np = nb * xdiv
    assert 128 % xdiv == 0 and Np % 128 == 0
    cols = np.concatenate([np.arange(128 * b, 128 * b + 128) for b in blocks])
    rows = cols[::xdiv] // xdiv
    sub = dict(c, x2=c["x2"][rows], f2=None if kind == 0 else c["f2"][cols])
    r = gram_bwd_hp(kind, sub, xdiv, Gb, gkb)
    out = {"hyp": r["hyp"]}
    if kind == 1:
        out["g_f1"] = r["g_f1"]
        out["g_f2"] = tuple(_scatter(Np, cols, a) for a in r["g_f2"])
    out["g_x2"] = tuple(_scatter((nb, c["x2"].shape[1]), rows, a) for a in r["g_x2"])
    return out


def _scatter(shape, idx, a):
    full = np.zeros(shape, np.longdouble)
    full[idx] = a
    return full


def gram_bwd_violations(got, ref, D, c=None):
    """Components outside |got - ref| <= 2^-53 (c W + D A), or, where W < 1e-290 (zero included), outside |got - ref| <= 1e-300
    -- gram_violations' rule for the underflowing elements.  (|got| <= 1e-300 there would refuse the reference itself: at d = 32
    the exponents straddle float64's range and hundreds of components have a W, and a value, between 1e-300 and 1e-290.)
    Returns (count, worst err / (2^-53 W), worst fraction of the bound) over the outputs of ``ref``."""
    c = GRAM_BWD_C if c is None else c
    bad, ratio, frac = 0, 0.0, 0.0
    for k, (v, W, A) in ref.items():
        g = ld(got[k]).reshape(np.shape(v))
        err = np.abs(g - v)
        tiny = W < ld(1e-290)
        safe = np.where(tiny, 1, W)
        r = np.where(tiny, 0, err / (ld(U) * safe))
        fr = np.where(tiny, 0, err / (ld(U) * (c * safe + D[k] * np.where(tiny, 1, A))))
        with np.errstate(invalid="ignore"):
            b = np.where(tiny, ~(err <= ld(1e-300)), ~(fr <= 1))       # a NaN is outside
        bad += int(np.sum(b))
        ratio, frac = max(ratio, float(np.nanmax(r, initial=0.0))), max(frac, float(np.nanmax(fr, initial=0.0)))
    return bad, ratio, frac


# ---- fused ELBO (variational_elbo_mf.py:24-51; include/mobocmf_hip.h, mobocmf_elbo_forward)
LOG_2PI = ld(2) * np.arctan(ld(1)) * 4
LOG_2PI = np.log(LOG_2PI)


def elbo_hp(layers, y, fid, kls, scale, g_elbo, g_skl):
    """layers[l] = None | dict(mean, var (B*div each), raw, lo, hi, div, rows).  Returns a dict of longdouble references:
    out3, abs3 (sum of |terms| behind out3[0] / out3[1]), n_terms, g_mean[l], g_var[l] (NaN beyond the prefix), g_raw[l],
    g_raw_abs[l], n_raw[l], g_kl."""
    y, fid = ld(y), np.asarray(fid)
    data, dabs, n = ld(0), ld(0), 0
    ge = ld(0 if g_elbo is None else g_elbo)
    gs = ld(0 if g_skl is None else g_skl)
    out = dict(g_mean=[], g_var=[], g_raw=[], g_raw_abs=[], n_raw=[])
    for l, lay in enumerate(layers):
        if lay is None:
            for k in ("g_mean", "g_var", "g_raw", "g_raw_abs", "n_raw"):
                out[k].append(None)
            continue
        div, rows = lay["div"], lay["rows"]
        lo, hi, raw = ld(lay["lo"]), ld(lay["hi"]), ld(lay["raw"])
        sg = 1 / (1 + np.exp(-raw))
        tau = lo + (hi - lo) * sg if hi > lo else raw
        chain = (hi - lo) * sg * (1 - sg) if hi > lo else ld(1)
        nn = rows * div
        mean, var = ld(lay["mean"][:nn]), ld(lay["var"][:nn])
        b = np.arange(nn) // div
        mask = fid[b] == float(l)
        dlt = y[b] - mean
        term = np.where(mask, -ld(0.5) * ((dlt * dlt + var) / tau + np.log(tau) + LOG_2PI), 0) / div
        data += term.sum()
        dabs += np.abs(term).sum()
        n += int(mask.sum())
        gm = np.full(lay["mean"].shape[0], np.nan, np.longdouble)
        gv = gm.copy()
        gm[:nn] = np.where(mask, ge / div * dlt / tau, 0)
        gv[:nn] = np.where(mask, -ld(0.5) * ge / div / tau, 0)
        st = np.where(mask, ld(0.5) * ((dlt * dlt + var) / (tau * tau) - 1 / tau), 0) / div * ge * chain
        sa = np.where(mask, ld(0.5) * ((dlt * dlt + var) / (tau * tau) + 1 / tau), 0) / div * np.abs(ge) * np.abs(chain)
        out["g_mean"].append(gm)
        out["g_var"].append(gv)
        out["g_raw"].append(st.sum())
        out["g_raw_abs"].append(sa.sum())
        out["n_raw"].append(int(mask.sum()))
    kl = sum((ld(k) for k in kls), ld(0))
    kabs = sum((abs(ld(k)) for k in kls), ld(0))
    sc = ld(scale)
    out["out3"] = np.array([data - sc * kl, sc * kl, -(data - sc * kl)], np.longdouble)
    out["abs3"] = np.array([dabs + abs(sc) * kabs, abs(sc) * kabs, dabs + abs(sc) * kabs], np.longdouble)
    out["n_terms"] = n + len(kls)
    out["g_kl"] = sc * (gs - ge)
    out["g_kl_abs"] = abs(sc) * (abs(gs) + abs(ge))
    return out


# ------------------------------------------------------------- factorisation chain: cases, references, a-priori bounds
# (chol.hip: three factorisation forms selected by mobocmf_tuning.potrf_cols, two routes of launch_trtri_z and the one-launch
# form's own inverse; elementwise.hip: gemv_rows, exact_gp_mll_kernel; the column statistics of mobocmf_exact_gp_predict.)
FACTOR_FAMILIES = ("rbf", "rbf_scaled", "signed")
POTRF_FORMS = (0, 1, 4)                  # potrf_cols: one launch | one column per hand-over | four columns per hand-over
FACTOR_ORDERS = (1, 15, 16, 17, 63, 64, 65, 80, 127, 128, 129, 191, 192, 193, 257, 320, 384, 385)
FACTOR_ORDER_COOP_CAPS = 640             # potrf_cols = 0, family rbf only: both workgroup caps of potrf_coop_workgroups bind
PREDICT_N = (80, 200, 320)
PREDICT_NT = (1, 127, 129, 300)
_RBF = {2: 0.6, 3: 0.9}                  # lengthscale per input dimension (n >= 63; 2.5 below): cond(K) within 1e6 .. 1e9


def _rbf_points(n, seed):
    """(training points, lengthscale) of the rbf families at order n."""
    d = 2 + (n + seed) % 2
    return np.random.default_rng(7919 * n + seed).random((n, d)), (2.5 if n < 63 else _RBF[d])


def factor_families(n):
    """The families run at order n: all three below 320; from 320 on the host's longdouble products dominate a test, so
    every order keeps ``rbf`` (the workload) and the other two alternate (rbf_scaled at 320 and 385, signed at 384)."""
    if n < 320:
        return FACTOR_FAMILIES
    if n == FACTOR_ORDER_COOP_CAPS:
        return ("rbf",)
    return ("rbf", "signed") if n == 384 else ("rbf", "rbf_scaled")


def one_launch_runs(n, cols):
    """launch_potrf_z takes potrf_coop_kernel for potrf_cols = 0 and 3 <= nreal <= 16 real 64-blocks (129 <= n <= 1024)."""
    return cols == 0 and 3 <= (n + 63) // 64 <= 16


_factor_cache = {}


def factor_case(family, n, seed=0):
    """(K [n x n], y [n]) as float64 numpy, read-only and cached.
    rbf         exp(-|x - x'|^2 / 2 l^2) + 1e-6 I on uniform points in [0, 1]^d, d = 2 (n + seed even) or 3, l = 0.6 / 0.9
                (2.5 below n = 63, where few points need a longer lengthscale to be as dependent): the workload's
                conditioning, cond(K) 1e6 .. 1e9 from n = 15 on (n = 1 has cond 1: the largest eigenvalue, <= n, cannot
                reach 1e6 against a jitter of 1e-6); test_factor_cases_have_the_stated_conditioning.
    rbf_scaled  D K_rbf D and D y with D = tile_scales(n, 64, .): powers of two in 2^+-[80, 100], constant on 64-blocks,
                neighbours >= 2^160 apart.  Every rounding commutes with them and every bound below is invariant, so a quiet
                64-block cannot hide behind a loud one.  chol.hip documents no dependence on magnitude (pivots are tested by
                !(a > 0) alone), entries stay within 2^+-200 and every intermediate -- squares of factor entries, products of
                L and L^-1 blocks -- within 2^+-400: the full exponent range of tile_scales is kept.
    signed      W W^T + n I, W = exact_ints((n, n)): exactly representable, cond < 100, off-diagonals of mixed sign (an RBF
                matrix has none).  y integer."""
    key = (family, n, seed)
    if key not in _factor_cache:
        if family == "signed":
            W = exact_ints((n, n), 31 * n + seed).astype(np.float64)
            K = W @ W.T + n * np.eye(n)
            y = exact_ints(n, 31 * n + seed + 1).astype(np.float64)
        else:
            assert family in ("rbf", "rbf_scaled"), family
            x, ls = _rbf_points(n, seed)
            d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
            K = np.exp(-0.5 * d2 / ls ** 2) + 1e-6 * np.eye(n)
            y = np.random.default_rng(7919 * n + seed + 1).standard_normal(n)
            if family == "rbf_scaled":
                D = tile_scales(n, 64, 17 * n + seed)
                K, y = D[:, None] * K * D[None, :], D * y
        K.setflags(write=False)
        y.setflags(write=False)
        _factor_cache[key] = (K, y)
    return _factor_cache[key]


def cross_kernel(family, n, nt, seed=0):
    """(Kts [n x nt], kss [nt]) for the predict tests: the family's kernel between the training points of factor_case and
    nt fresh uniform points (rbf; kss = 1 + 1e-6), or signed integers (signed; kss integer >= 0)."""
    if family == "signed":
        return exact_ints((n, nt), 5 * n + nt + seed).astype(np.float64), np.abs(exact_ints(nt, n + 7 * nt + seed)).astype(np.float64)
    assert family == "rbf"
    x, ls = _rbf_points(n, seed)                                        # the training points of factor_case
    xt = np.random.default_rng(104729 * n + nt + seed).random((nt, x.shape[1]))
    d2 = ((x[:, None, :] - xt[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2 / ls ** 2), np.full(nt, 1.0 + 1e-6)


def tri_inverse_hp(L):
    """Inverse of the lower triangle of L by forward substitution, row by row, in extended precision (longdouble; mpmath at
    50 digits where longdouble is no wider than float64).  numpy.linalg.inv -- a general LU -- misses the componentwise
    bounds below by factors of 1e3 .. 1e13 and is no reference."""
    n = L.shape[0]
    if HAVE_LONGDOUBLE:
        Lq = np.tril(ld(L))
        X = np.zeros((n, n), np.longdouble)
        for i in range(n):
            row = -(Lq[i, :i] @ X[:i, :i]) if i else np.zeros(0, np.longdouble)
            X[i, :i] = row / Lq[i, i]
            X[i, i] = 1 / Lq[i, i]
        return X
    import mpmath
    mpmath.mp.dps = 50
    Lm = [[mpmath.mpf(float(v)) for v in r] for r in np.asarray(L, np.float64)]
    X = [[mpmath.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = (mpmath.mpf(1) if i == j else mpmath.mpf(0)) - sum((Lm[i][k] * X[k][j] for k in range(j, i)), mpmath.mpf(0))
            X[i][j] = s / Lm[i][i]
    return np.array([[float(v) for v in r] for r in X], dtype=np.float64).astype(np.longdouble)


# Constants of the bounds.  u = 2^-53; every bound is first order in u (k u <= 1.2e-13 at k = 1024: the second-order terms are
# below 1e-12 of the bound).  None is fitted to device output; the CPU proof (test_kernel_reference_cpu.py) holds float64
# restatements of the same algorithms to HALF of each.
#
# CHOL_CR.  Entry (i, j), i >= j, k = j + 1 terms: the code forms s_ij = a_ij - sum_{t<j} l_it l_jt, r_j = rsqrt_nr(s_jj) =
# (1 + d_r) / sqrt(s_jj), and l_ij = fl(s_ij r_j), l_jj = fl(s_jj r_j) (no divide, no sqrt: potrf_panel2/4_kernel,
# chol64_pad_rows, chol_inv_tile16).  Hence l_ij l_jj = s_ij (1 + d_r)^2 (1 + d)(1 + d'): the k - 1 subtractions of the sum
# and the two multiplies give the classical k + 1 (Higham, Accuracy and Stability, Thm 10.3 / Lemma 8.4, which has a divide
# and a sqrt in their place), the reciprocal root adds 2 |d_r|.  rsqrt_nr is documented (chol.hip) as ~1 ulp, and 1 ulp is at
# most 2 u relative: + 4.  The updates do not run one term at a time: a 64-column step subtracts a 64-term partial sum formed
# on the matrix cores (syrk64_update_kernel, pc_tasks), the four-column panel subtracts a 4-term one; either costs the first
# term of a group one rounding more than a term-by-term chain: + 1.  That is k + 6; C_r = 8 leaves 2 u for the "~" (a
# reciprocal root 1.5 ulp off).  (Read the other way -- "~1 ulp" doubled to 4 u, entering twice -- it is 8 as well.)
CHOL_CR = 8
# TRINV_CX.  |Xh - X| <= (n + C_x) u |X||L||X| is the forward-error bound of inversion by substitution (Higham, Ch. 14:
# |X - Xh| <= c_n u |L^-1||L||L^-1| for the unblocked methods).  The code runs substitution only inside a 64-block (with the
# reciprocal root r_i in place of a divide: x_i = fl(s r_i), (1 + d_r)(1 + d), + 3 at |d_r| <= 2 u; + 1 for l_ii = fl(s_ii r_i)
# being the diagonal it inverts) and the block recursion X21 = -X22 (L21 X11) above it.  One level of it on halves of order m:
#   Xh21 - X21 = -(Xh22 - X22) L21 X11 - X22 L21 (Xh11 - X11) - X22 E_T + E_2,  |E_T| <= m u |L21||X11|, |E_2| <= m u |X22||L21 X11|
# so with c(m) for the halves, c(2m) = c(m) + 2m IF the inherited terms |X22||L22||X22| |L21||X11| and |X22||L21| |X11||L11||X11|
# are measured by |X22||L22||X21| + |X22||L21||X11| + |X21||L11||X11| = (|X||L||X|)_21.  Componentwise that replaces
# |X22||L21||X11| by |X21| = |X22 L21 X11|: exact where the product does not cancel, and where it cancels the block recursion
# is known to satisfy only the weaker bound with one more factor |L||X| (Higham, section 14.2.2, on block methods).  The
# recursion then gives c(n) = n + c(64) - 64, also for the block-row route (products of order 128 i and 128 per block row)
# and the right-looking one-launch inverse (one 64-term product per step), so C_x = c(64) - 64 = 4, doubled for the level-0
# kernel's two 64-term products on top of the two 64-blocks: C_x = 8.  The issue fixes this form; the CPU proof measures how
# far inside it the float64 restatement of the recursion stays on every case the GPU tests use.
TRINV_CX = 8
# MLL_CLOG.  exact_gp_mll_kernel sums t_i = -a_i^2 / 2 - log(l_ii) over a thread chain and a block tree (<= n roundings),
# then subtracts fl(n / 2 * log 2 pi).  Per term: a_i^2 / 2 one rounding (the halving is exact), log at most 1 ulp = 2 u (HIP
# programming guide, "HIP math API", double-precision functions: log, maximum error 1 ULP), the subtraction 1; the constant's
# own rounding, its product with n / 2 and the last subtraction 3: C_log = 1 + 2 + 1 + 3 = 7, taken as 8.
MLL_CLOG = 8


def _ratio(err, R):
    """worst err / (u R) over the entries given (R = 0: any error is infinite)."""
    if err.size == 0:
        return 0.0
    pos = R > 0
    return float(np.max(np.where(pos, err / np.where(pos, ld(U) * R, 1), np.where(err > 0, np.inf, 0))))


def chol_bound_units(Lh, Xh=None):
    """The allowed |Lh Lh^T - K| in units of u as (B, R), R = |Lh||Lh^T| (float64; n x n, the lower triangle counts).
    Xh None -- the substitution forms (potrf_cols 1 and 4, every form at n <= 128): B = (min(i, j) + 1 + C_r) R.
    Xh given -- the one-launch form, Xh its inverse, whose diagonal 64-blocks (16-tiles) ARE the explicit inverses the
    kernel multiplies with.  potrf_coop_kernel forms EVERY block below the diagonal block J as a product with the computed
    inverse: the look-ahead block in the panel workgroup (D), all others in the trailing workgroups (do_row), and inside the
    diagonal block the 16-tiles below a pivot tile likewise (L_is = A_is L_ss^-T).  For such a block, m = 64 (16):
        Lh_iJ = S_iJ Xh^T + E_1,                       |E_1| <= m u |S_iJ||Xh^T|      (an m-term product)
        Lh_iJ Lh_JJ^T - S_iJ = S_iJ (Lh_JJ Xh - I)^T + E_1 Lh_JJ^T
        |Lh_JJ Xh - I| = |Lh_JJ (Xh - X)| <= (m + C_x) u |Lh_JJ||X||Lh_JJ||X|        (the inverse's forward error)
    and |S_iJ| <= |Lh_iJ||Lh_JJ^T| to first order, so with G = |Xh_JJ^T||Lh_JJ^T| the block's residual carries, on top of the
    substitution bound (which covers S_iJ's own sum), u |Lh_iJ| |Lh_JJ^T| (m G + (m + C_x) G G).  A substitution-form panel has
    no such term: that is why the classical bound does not hold for this form (ratio 1.2 .. 7.7 on RBF matrices)."""
    Lh = np.tril(np.asarray(Lh, np.float64))
    n = Lh.shape[0]
    aL = np.abs(Lh)
    R = aL @ aL.T
    i = np.arange(n)
    B = (np.minimum(i[:, None], i[None, :]) + 1 + CHOL_CR) * R
    if Xh is not None:
        aX = np.abs(np.asarray(Xh, np.float64))
        for m in (64, 16):
            for j0 in range(0, n, m):
                j1 = min(j0 + m, n)
                r1 = n if m == 64 else min((j0 // 64 + 1) * 64, n)      # 16-tiles: the rows of the same 64-block only
                if j1 >= r1:
                    continue
                LJt = aL[j0:j1, j0:j1].T
                G = aX[j0:j1, j0:j1].T @ LJt
                B[j1:r1, j0:j1] += aL[j1:r1, j0:j1] @ (LJt @ (m * G + (m + TRINV_CX) * (G @ G)))
    return B, R


def chol_check(Lh, K, Xh=None):
    """(ok, worst |Lh Lh^T - K| / (u R), worst fraction of the bound) over the lower triangle; residual in extended precision."""
    Lh = np.tril(np.asarray(Lh, np.float64))
    n = Lh.shape[0]
    err = np.abs(matmul_hp(Lh, Lh.T) - ld(K))
    B, R = chol_bound_units(Lh, Xh)
    low = tri_mask(n, True)
    return bool(np.all(err[low] <= ld(U) * B[low])), _ratio(err[low], R[low]), _ratio(err[low], B[low])


def trinv_check(Xh, Lh, X=None):
    """Forward error of the inverse against X = tri_inverse_hp(Lh) -- the inverse of the factor GIVEN, so the factorisation's
    error is not counted again: |Xh - X| <= (n + C_x) u |X||Lh||X| on the lower triangle.  (ok, worst ratio in u R)."""
    Lh = np.tril(np.asarray(Lh, np.float64))
    n = Lh.shape[0]
    X = tri_inverse_hp(Lh) if X is None else X
    aX = np.abs(np.asarray(X, np.float64))
    R = aX @ np.abs(Lh) @ aX
    err = np.abs(ld(Xh) - X)
    low = tri_mask(n, True)
    return bool(np.all(err[low] <= (n + TRINV_CX) * ld(U) * R[low])), _ratio(err[low], R[low])


def solve_check(ah, Xh, y):
    """a = L^-1 y as gemv_rows forms it (a row's i + 1 non-zero terms: a lane chain and a butterfly, zeros add exactly):
    |ah - Xh y| <= (n + 2) u |Xh||y|, against extended precision on the inverse GIVEN."""
    n = len(y)
    ref = matmul_hp(np.tril(Xh), np.asarray(y)[:, None])[:, 0]
    R = np.abs(np.tril(Xh)) @ np.abs(y)
    err = np.abs(ld(ah) - ref)
    return bool(np.all(err <= (n + 2) * ld(U) * R)), _ratio(err, R)


def mll_check(mll, Lh, ah):
    """mll against -1/2 sum a^2 - sum log l_ii - n/2 log 2 pi in extended precision on the factor and the a GIVEN; tolerance
    (n + C_log) u (1/2 sum a^2 + sum |log l_ii| + n/2 log 2 pi)."""
    n = len(ah)
    a, lg = ld(ah), np.log(ld(np.diag(Lh)))
    half = ld(0.5)
    ref = -half * (a * a).sum() - lg.sum() - half * n * LOG_2PI
    R = half * (a * a).sum() + np.abs(lg).sum() + half * n * LOG_2PI
    err = np.abs(ld(mll) - ref)
    return bool(err <= (n + MLL_CLOG) * ld(U) * R), float(err / (ld(U) * R))


def predict_check(mean, var, Xh, ah, Kts, kss):
    """With A = Xh Kts exactly (the device: an n-term triangular product, then an n-term column sum in partial rows):
    |mean_j - sum_i A_ij a_i| <= (2n + 4) u (|a|^T |Xh||Kts|)_j,  |var_j - (kss_j - sum_i A_ij^2)| <= (2n + 4) u (|kss_j| +
    sum_i (|Xh||Kts|)_ij^2).  Returns (ok_mean, ratio_mean, ok_var, ratio_var), ratios in u R."""
    n = len(ah)
    Xl = np.tril(np.asarray(Xh, np.float64))
    A = matmul_hp(Xl, Kts)
    mref = (A * ld(ah)[:, None]).sum(0)
    vref = ld(kss) - (A * A).sum(0)
    G = np.abs(Xl) @ np.abs(Kts)
    Rm, Rv = np.abs(ah) @ G, np.abs(kss) + (G * G).sum(0)
    em, ev = np.abs(ld(mean) - mref), np.abs(ld(var) - vref)
    c = (2 * n + 4) * ld(U)
    return bool(np.all(em <= c * Rm)), _ratio(em, Rm), bool(np.all(ev <= c * Rv)), _ratio(ev, Rv)


# ------------------------------------------------------------------------------------------------ direct C-ABI callers
def lib():
    from mobocmf_amd import _lib
    return _lib.require_device()


def make_tuning(**kw):
    """An explicit mobocmf_tuning: the compiled-in defaults with ``kw`` on top."""
    from mobocmf_amd import _lib
    t = _lib.Tuning()
    _lib.check(_lib.load().mobocmf_tuning_init(ctypes.byref(t)), "mobocmf_tuning_init")
    for k, v in kw.items():
        assert k in _lib.Tuning.KNOBS, k
        setattr(t, k, int(v))
    return t


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Strided:
    """A rows x width device matrix inside a NaN-filled backing store: leading dimension ``ldim`` >= width (the columns
    width..ldim are slack) and ``offset`` doubles in front of the base pointer (offset 2: a base that is only 16-byte
    aligned).  ``slack_untouched()``: every slack double is still NaN -- no stray write."""

    def __init__(self, rows, width, pad=0, offset=0, fill=None, dtype=torch.float64, device="cuda"):
        self.rows, self.width, self.ld, self.offset = rows, width, width + pad, offset
        self.back = torch.full((offset + rows * self.ld,), NAN, dtype=dtype, device=device)
        self.full = self.back[offset:].view(rows, self.ld)
        self.view = self.full[:, :width]
        self.mask = torch.ones(self.back.shape, dtype=torch.bool, device=device)
        self.mask[offset:].view(rows, self.ld)[:, :width] = False
        if fill is not None:
            self.set(fill)

    def set(self, a):
        self.view.copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(self.view.device))
        return self

    def poison(self):
        self.back.fill_(NAN)
        return self

    def slack_untouched(self):
        return bool(torch.isnan(self.back[self.mask]).all())

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())


def gemm(A, B, C, Mr, Nc, Kd, tri=0, trans_b=0, alpha=1.0, accumulate=0, tune=None, check=True):
    """mobocmf_gemm_f64 on Strided operands, pointers and leading dimensions as they are (check=False: the status is
    returned, not raised)."""
    from mobocmf_amd import _lib
    rc = lib().mobocmf_gemm_f64(tri, int(trans_b), Mr, Nc, Kd, A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld, float(alpha),
                                int(accumulate), ctypes.byref(tune) if tune is not None else None, _stream())
    if check:
        _lib.check(rc, "mobocmf_gemm_f64")
    return rc


def colstat_rows(tri, Mr, Nc, Kd, tune):
    from mobocmf_amd import _lib
    rows = ctypes.c_int32()
    _lib.check(lib().mobocmf_gemm_colstat_rows(tri, Mr, Nc, Kd, ctypes.byref(tune), ctypes.byref(rows)), "colstat_rows")
    return rows.value


def gemm_epilogue(A, B, C, Mr, Nc, Kd, tri, epi, alpha=1.0, stream_out=0, colsq=None, coldot=None, avec=None, bscale=None,
                  gmu=None, cgv=None, Aaux=None, rowdot=None, colact=None, tune=None):
    """mobocmf_gemm_f64_epilogue; Aaux shares C's leading dimension (a Strided of C's layout)."""
    from mobocmf_amd import _lib
    assert Aaux is None or Aaux.ld == C.ld
    rc = lib().mobocmf_gemm_f64_epilogue(tri, epi, Mr, Nc, Kd, A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld, float(alpha),
                                         int(stream_out), _p(colsq), _p(coldot), _p(avec), _p(bscale), _p(gmu), _p(cgv),
                                         Aaux.ptr if Aaux is not None else None, _p(rowdot), _p(colact),
                                         ctypes.byref(tune) if tune is not None else None, _stream())
    _lib.check(rc, "mobocmf_gemm_f64_epilogue")


def syrk(A, w, H, Mr, Kd, kact=None, tune=None):
    """mobocmf_syrk_weighted_f64 with a NaN-filled workspace of exactly the reported size."""
    from mobocmf_amd import _lib
    nb = ctypes.c_size_t()
    tp = ctypes.byref(tune) if tune is not None else None
    _lib.check(lib().mobocmf_syrk_workspace_bytes(Mr, Kd, tp, ctypes.byref(nb)), "mobocmf_syrk_workspace_bytes")
    ws = torch.full((max(nb.value // 8, 1),), NAN, dtype=torch.float64, device=H.device)
    rc = lib().mobocmf_syrk_weighted_f64(Mr, Kd, A.ptr, A.ld, _p(w), _p(H), _p(ws), nb.value, _p(kact), tp, _stream())
    _lib.check(rc, "mobocmf_syrk_weighted_f64")


def gram_rep(kind, d, x1, f1, n1, x2, f2, nbase2, xdiv, hyp, K, ldk, knn=None):
    """mobocmf_gram_forward_rep with the pointers as given (f2 may be a view that is only 8-byte aligned)."""
    from mobocmf_amd import _lib
    rc = lib().mobocmf_gram_forward_rep(kind, d, _p(x1), _p(f1), n1, _p(x2), _p(f2), nbase2, xdiv, _p(hyp), _p(K), ldk,
                                        _p(knn), _stream())
    _lib.check(rc, "mobocmf_gram_forward_rep")


def gram_bwd_geometry(kind, d, n1, nbase2, xdiv, want_dx):
    """(workspace bytes, (grid x, grid y, rows per workgroup)) of mobocmf_gram_backward: a host computation, no device needed."""
    from mobocmf_amd import _lib
    nb, geo = ctypes.c_size_t(), (ctypes.c_int32 * 3)()
    _lib.check(_lib.load().mobocmf_gram_backward_workspace_bytes(kind, d, n1, nbase2, xdiv, int(want_dx), ctypes.byref(nb), geo),
               "mobocmf_gram_backward_workspace_bytes")
    return nb.value, tuple(geo)


class GramBwd:
    """What gram_bwd leaves behind: the outputs as float64 numpy ('hyp', 'g_f1', 'g_f2', 'g_x2'; absent ones missing),
    ``geometry`` and ``untouched``: every guard double behind an output and behind the workspace is still NaN."""


def gram_bwd(kind, d, x1, f1, n1, x2, f2, nbase2, xdiv, hyp, G, ldk, gknn=None, colact=None, want_dx=True, guard=8,
             ws_bytes=None, check=True):
    """mobocmf_gram_backward with the pointers as given (f2 / G may be views that are only 8-byte aligned): outputs and a
    workspace of exactly the reported size (``ws_bytes``: that size instead) NaN before the call, ``guard`` NaN doubles
    behind each.  Returns a GramBwd, or the status if ``check`` is False and the call is refused."""
    from mobocmf_amd import _lib
    nbytes, geo = gram_bwd_geometry(kind, d, n1, nbase2, xdiv, want_dx)
    assert nbytes % 8 == 0
    Np = nbase2 * xdiv
    new = lambda n: torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda")
    lens = {"hyp": 1 + d if kind == 0 else 5 + 2 * d}
    if kind == 1:
        lens["g_f1"], lens["g_f2"] = n1, Np
    if want_dx:
        lens["g_x2"] = nbase2 * d
    buf = {k: new(n) for k, n in lens.items()}
    use = nbytes if ws_bytes is None else ws_bytes
    ws = new(max(nbytes, use) // 8)
    rc = lib().mobocmf_gram_backward(kind, d, _p(x1), _p(f1), n1, _p(x2), _p(f2), nbase2, xdiv, _p(hyp), _p(G), ldk, _p(gknn),
                                     _p(colact), _p(buf["hyp"]), _p(buf.get("g_f1")), _p(buf.get("g_f2")), _p(buf.get("g_x2")),
                                     _p(ws), use, _stream())
    if not check and rc != 0:
        return rc
    _lib.check(rc, "mobocmf_gram_backward")
    r = GramBwd()
    r.geometry = geo
    r.out = {k: buf[k][:n].cpu().numpy() for k, n in lens.items()}
    r.untouched = all(bool(torch.isnan(buf[k][n:]).all()) for k, n in lens.items()) and bool(torch.isnan(ws[nbytes // 8:]).all())
    # the workspace's own slack: the partials (hyp | df | dzf | dx, in the header's geometry) start on 256-byte boundaries
    gx, gy, _ = geo
    parts = [gx * gy * lens["hyp"]] + ([gy * Np, gx * ((n1 + 31) // 32 * 32)] if kind == 1 else []) + ([gy * nbase2 * d] if want_dx else [])
    off = 0
    for n in parts:
        end = off + (n + 31) // 32 * 32
        r.untouched = r.untouched and bool(torch.isnan(ws[off + n:end]).all())
        off = end
    assert off == nbytes // 8, (off, nbytes)
    if "g_x2" in r.out:
        r.out["g_x2"] = r.out["g_x2"].reshape(nbase2, d)
    return r


def _tab(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[0 if t is None else t.data_ptr() for t in ts])


def _elbo_tables(layers, B):
    L = len(layers)
    get = lambda k, dflt: [dflt if lay is None else lay[k] for lay in layers]
    return (L, (ctypes.c_int32 * L)(*get("div", 1)), (ctypes.c_double * L)(*get("lo", 0.0)),
            (ctypes.c_double * L)(*get("hi", 0.0)), (ctypes.c_int64 * L)(*get("rows", B)))


def elbo_forward(layers, y, fid, kls, scale):
    """mobocmf_elbo_forward; layers[l] = None | dict(mean, var, raw: device tensors; div, lo, hi, rows).  Returns out3."""
    from mobocmf_amd import _lib
    B = y.numel()
    L, div, lo, hi, rows = _elbo_tables(layers, B)
    T = lambda k: _tab([None if lay is None else lay[k] for lay in layers])
    out = torch.full((3,), NAN, dtype=torch.float64, device=y.device)
    scratch = torch.full((8 * 512,), NAN, dtype=torch.float64, device=y.device)
    rc = lib().mobocmf_elbo_forward(L, T("mean"), T("var"), div, T("raw"), lo, hi, _p(y), _p(fid), B, rows, len(kls),
                                    _tab(kls) if kls else None, float(scale), _p(out), _p(scratch), scratch.numel() * 8,
                                    _stream())
    _lib.check(rc, "mobocmf_elbo_forward")
    return out


def elbo_backward(layers, y, fid, scale, g_elbo, g_skl):
    """mobocmf_elbo_backward into NaN-filled gradient buffers of B * div entries per layer.
    Returns (g_mean, g_var, g_raw lists, g_kl)."""
    from mobocmf_amd import _lib
    B = y.numel()
    L, div, lo, hi, rows = _elbo_tables(layers, B)
    T = lambda k: _tab([None if lay is None else lay[k] for lay in layers])
    new = lambda lay, n: None if lay is None else torch.full((n,), NAN, dtype=torch.float64, device=y.device)
    gm = [new(lay, 0 if lay is None else lay["mean"].numel()) for lay in layers]
    gv = [new(lay, 0 if lay is None else lay["mean"].numel()) for lay in layers]
    gr = [new(lay, 1) for lay in layers]
    gkl = torch.full((1,), NAN, dtype=torch.float64, device=y.device)
    scratch = torch.full((8 * 512,), NAN, dtype=torch.float64, device=y.device)
    rc = lib().mobocmf_elbo_backward(L, T("mean"), T("var"), div, T("raw"), lo, hi, _p(y), _p(fid), B, rows, float(scale),
                                     _p(g_elbo), _p(g_skl), _tab(gm), _tab(gv), _tab(gr), _p(gkl), _p(scratch),
                                     scratch.numel() * 8, _stream())
    _lib.check(rc, "mobocmf_elbo_backward")
    return gm, gv, gr, gkl


# ---- exact GP (mobocmf_exact_gp_factor / _predict) and mobocmf_mf_kernel_combine
def factors(st, n):
    """(L, L^-1, npad) as padded views of an exact-GP state (anything with a byte tensor ``state``): L at 0, L^-1 at the next
    256-byte boundary behind npad^2 doubles (api.hip carve_exact_state)."""
    npad = (n + 127) // 128 * 128
    buf = st.state.view(torch.float64)
    L = buf[:npad * npad].view(npad, npad)
    off = (npad * npad * 8 + 255) // 256 * 256 // 8
    Li = buf[off:off + npad * npad].view(npad, npad)
    return L, Li, npad


class ExactGP:
    """What exact_gp leaves behind: state / scratch (byte tensors, NaN before the call), views L, Li (npad x npad), a (npad),
    mll (0-d), info (int), the Strided K."""


def _exact_bytes(n, nt):
    from mobocmf_amd import _lib
    sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib().mobocmf_exact_gp_workspace_bytes(n, nt, ctypes.byref(sb), ctypes.byref(cb)), "mobocmf_exact_gp_workspace_bytes")
    assert sb.value % 8 == 0 and cb.value % 8 == 0
    return sb.value, cb.value


def _nan_bytes(nbytes):
    return torch.full((nbytes // 8,), NAN, dtype=torch.float64, device="cuda").view(torch.uint8)


def exact_gp(K, ldk, y, tune, state=None):
    """mobocmf_exact_gp_factor through the C ABI: K (n x n numpy) inside a NaN-filled store of leading dimension ``ldk``,
    sizes from mobocmf_exact_gp_workspace_bytes, state and scratch NaN before the call (``state``: reuse that one, poisoned
    again), ``ldk`` and the explicit ``tune`` passed unchanged.  Returns an ExactGP."""
    from mobocmf_amd import _lib
    n = K.shape[0]
    sb, cb = _exact_bytes(n, 1)
    g = ExactGP()
    g.n, g.K = n, Strided(n, n, pad=ldk - n, fill=np.array(K))
    g.state = _nan_bytes(sb) if state is None else state
    g.state.view(torch.float64).fill_(NAN)
    g.scratch = _nan_bytes(cb)
    g.mll = torch.full((), NAN, dtype=torch.float64, device="cuda")
    info = torch.full((), -77, dtype=torch.int32, device="cuda")
    yd = torch.as_tensor(np.array(y), dtype=torch.float64).cuda()
    rc = lib().mobocmf_exact_gp_factor(n, g.K.ptr, ldk, _p(yd), _p(g.mll), _p(info), _p(g.state), sb, _p(g.scratch), cb,
                                       ctypes.byref(tune), _stream())
    _lib.check(rc, "mobocmf_exact_gp_factor")
    torch.cuda.synchronize()
    g.info = int(info)
    g.L, g.Li, g.npad = factors(g, n)
    off = (g.npad * g.npad * 8 + 255) // 256 * 256 // 8
    g.a = g.state.view(torch.float64)[2 * off:2 * off + g.npad]
    return g


def exact_gp_predict_direct(g, Kts, ld, kss, tune, guard=8):
    """mobocmf_exact_gp_predict on the state of ``g``: Kts (n x nt numpy) with leading dimension ``ld`` (slack NaN), scratch
    of the reported size NaN before the call, mean / var inside stores with ``guard`` sentinels behind them.  Returns
    (mean, var, untouched): float64 numpy and whether every sentinel and all slack of Kts is as it was."""
    from mobocmf_amd import _lib
    n, nt = Kts.shape
    sb, cb = _exact_bytes(n, nt)
    assert sb == g.state.numel()
    Kd = Strided(n, nt, pad=ld - nt, fill=Kts)
    scratch = _nan_bytes(cb)
    kd = torch.as_tensor(np.ascontiguousarray(kss), dtype=torch.float64).cuda()
    SENT = -12345.0
    mean = torch.full((nt + guard,), SENT, dtype=torch.float64, device="cuda")
    var = torch.full((nt + guard,), SENT, dtype=torch.float64, device="cuda")
    rc = lib().mobocmf_exact_gp_predict(n, nt, Kd.ptr, ld, _p(kd), _p(mean), _p(var), _p(g.state), sb, _p(scratch), cb,
                                        ctypes.byref(tune), _stream())
    _lib.check(rc, "mobocmf_exact_gp_predict")
    torch.cuda.synchronize()
    untouched = bool((mean[nt:] == SENT).all()) and bool((var[nt:] == SENT).all()) and Kd.slack_untouched()
    return mean[:nt].cpu().numpy(), var[:nt].cpu().numpy(), untouched


def mf_combine(Ks, Kn, s1, s2, l1, l2, ntab, diag, out, n1, n2, rows_p, cols_p):
    """mobocmf_mf_kernel_combine on Strided Ks / Kn (one leading dimension) and a Strided ``out`` of rows_p x cols_p; s1 / s2
    may be None (NULL)."""
    from mobocmf_amd import _lib
    assert Ks.ld == Kn.ld and out.rows >= rows_p and out.width == cols_p
    rc = lib().mobocmf_mf_kernel_combine(n1, n2, Ks.ptr, Kn.ptr, Ks.ld, _p(s1), _p(s2), _p(l1), _p(l2), _p(ntab), float(diag),
                                         out.ptr, out.ld, rows_p, cols_p, _stream())
    _lib.check(rc, "mobocmf_mf_kernel_combine")


# ------------------------------------------------------------------------------- the variational layer: cases and reference
# (api.hip: chain_forward / panel_forward / panel_backward / chain_backward; DESIGN.md, "The layer bound".)
#
# layer_ref runs the DEVICE's algebraic form -- explicit X = L^-1, A = X K_mn, a = X m, U = X L_S, mean = A^T a, C = U^T A, q, r,
# var, KL; backwards dC, dA, da, dU, dK_mn = X^T dA, g_m, g_LS, Y, dL, Phi(L^T dL), dK_mm = sym(X^T Phi X), the Gram backwards
# -- in the number format asked for: numpy.longdouble is the reference, numpy.float64 the restatement.  Its SHADOW S is the
# same chain of statements with every operand replaced by its magnitude and every subtraction by an addition: the leaves are
# |m|, |L_S|, |g_mean|, |g_var|, |g_kl|, sum_t |term_t| of K_mn, |L| of the factor (a Cholesky factor is determined by K_mm to
# within |L||L^T|: its own magnitude is its scale), the comparison inverse of |L| (forward substitution with additions:
# >= |L^-1| entrywise, the scale of Higham's |X||L||X|) and |log .| in the KL.  The Gram-derived outputs take the A output of
# _gram_bwd (sum |G||d term / d theta|) fed with the shadow of dK.  The gate is |got - ref| <= C_g u S per component, and
# components with S = 0 (the strict upper triangle of g_LS, gradients of columns that got none) must be exactly zero.
#
# C_g is not fitted to the device.  Per output group two float64 algorithms are measured against the longdouble reference on
# every case the GPU tests run (tests/test_layer_reference_cpu.py, on every run): the float64 run of layer_ref, and float64
# autograd over oracle.layer_moments + kl_layer (triangular solves, no explicit inverse).  LAYER_RATIO_MEASURED records the
# larger of the two worst ratios err / (u S), rounded up; C_g = 4 x that, the room DESIGN 5.5 gives the Gram constants for a
# third summation order, FMA and the reciprocal-root Cholesky.
LAYER_GROUPS = {"forward": ("mean", "var", "kl"), "chain": ("g_m", "g_LS"), "gram": ("g_hyp", "g_x", "g_f", "g_zf")}
# Measured: forward 13.1 (oracle; restatement 6.0), chain 128.7 (oracle; restatement 75.7: both g_LS of the kind 1, M = 128
# case when only the KL is differentiated -- g_LS = g_kl (tril(K_mm^-1 L_S) - diag(1 / LS_ii)) cancels on the diagonal and
# carries the factor's forward error, which |L| as a leaf does not scale with; 47 at M = 129 under the KL alone, at most 27
# with all three upstream gradients), gram 95.4 (oracle: its x / ls - z / ls; restatement 13.8).  The figures move by a few per
# cent with the BLAS blocking of the host, so they are recorded a quarter above the measurement: another blocking stays
# inside [recorded / 2, recorded].
LAYER_RATIO_MEASURED = {"forward": 17.0, "chain": 165.0, "gram": 125.0}
LAYER_C = {k: 4.0 * v for k, v in LAYER_RATIO_MEASURED.items()}
LAYER_COND_MAX = 1e3
LAYER_MARGIN = 1e-9
CLAMP_JITTER = -2e-3


def layer_group(name):
    return next(g for g, names in LAYER_GROUPS.items() if name in names)


def hyp_dict(kind, hyp, d):
    """The oracle's hyper-parameter dict from the packed vector (include/mobocmf_hip.h, mobocmf_layer_desc)."""
    if kind == 0:
        return {"alpha": hyp[0], "ls": hyp[1:1 + d]}
    return {"a1": hyp[0], "af": hyp[1], "nu": hyp[2], "a2": hyp[3], "lsf": hyp[4], "ls1": hyp[5:5 + d], "ls2": hyp[5 + d:5 + 2 * d]}


_layer_cases = {}


def layer_case(kind, d, M, nbase, xdiv, seed=0, clamp=0, floor=False, branch=0, want_dx=1):
    """One well-conditioned layer problem as a dict of float64 numpy arrays and the descriptor's scalars (cached, read-only).
    Z_x: a lattice of spacing h jittered by 0.15 h (d <= 3) or uniform points (d > 3: they are far apart anyway), lengthscales
    0.55 .. 0.8 h resp. 0.25 .. 0.32, so that K_mm is diagonally dominant: cond(K_mm + jitter I) <= 1e3 (asserted by the CPU
    test, as are the margins below).  The data rows sit 0.6 lengthscales from randomly chosen inducing rows: K_mn has entries
    of order one.  ``clamp`` = k > 0: the first k base rows lie ON inducing rows (row i on Z[i % M], f on zf) and jitter =
    CLAMP_JITTER < 0, so that q > k_nn there (training branch: clamp(k_nn - q, 0) active in those columns, and in any other that lies as close).  ``floor``:
    min_var is raised to half the median variance -- the columns below sit on the floor.  Upstream gradients g_mean, g_var
    standard normal, g_kl = 0.37."""
    key = (kind, d, M, nbase, xdiv, seed, clamp, floor, branch, want_dx)
    if key in _layer_cases:
        return _layer_cases[key]
    rng = np.random.default_rng(100003 * kind + 1009 * M + 31 * nbase + 7 * d + xdiv + 131071 * seed)
    if d <= 3:
        side = int(np.ceil(M ** (1.0 / d)))
        h = 1.0 / side
        grid = np.stack(np.meshgrid(*[np.arange(side)] * d, indexing="ij"), -1).reshape(-1, d)
        Zx = (grid[rng.permutation(len(grid))[:M]] + 0.5 + 0.15 * rng.uniform(-1, 1, (M, d))) * h
        ls = lambda: h * rng.uniform(0.55, 0.8, d)
    else:
        Zx = rng.random((M, d))
        ls = lambda: rng.uniform(0.25, 0.32, d)
    Np = nbase * xdiv
    if kind == 0:
        hyp = np.concatenate([[0.7 + rng.random()], ls()])
        zf = f = None
        lsx = hyp[1:]
    else:
        lsx = ls()
        hyp = np.concatenate([[0.6 + rng.random(), 0.5 + rng.random(), 0.5 + rng.random(), 0.05 + 0.1 * rng.random(),
                               0.7 + rng.random()], lsx, ls()])
        zf = 0.5 * rng.standard_normal(M)
        f = rng.standard_normal(Np)
    near = rng.integers(0, M, nbase)
    x = Zx[near] + 0.6 * lsx * rng.standard_normal((nbase, d)) / np.sqrt(d)
    if clamp:
        assert branch == 0 and clamp <= nbase
        rows = np.arange(clamp) % M
        x[:clamp] = Zx[rows]
        if kind == 1:
            f[:clamp * xdiv] = np.repeat(zf[rows], xdiv)
    c = dict(kind=kind, d=d, M=M, nbase=nbase, xdiv=xdiv, Np=Np, branch=branch, want_dx=want_dx, clamp=clamp, floor=floor,
             jitter=CLAMP_JITTER if clamp else 1e-6, min_var=1e-10, x=x, f=f, Zx=Zx, zf=zf, hyp=hyp,
             m=0.3 * rng.standard_normal(M), L_S=0.2 * np.eye(M) + 0.05 * np.tril(rng.standard_normal((M, M))),
             g_mean=rng.standard_normal(Np), g_var=rng.standard_normal(Np), g_kl=0.37, key=key)
    if floor:
        c["min_var"] = 0.5 * float(np.median(_layer_forward(c, _f64)[0]["varraw"]))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _layer_cases[key] = c
    return c


def with_upstream(c, g_mean=None, g_var=None, g_kl=0.0, tag=None):
    """A copy of the case with other upstream gradients (None: exact zeros -- the entry points take no NULL there)."""
    z = np.zeros(c["Np"])
    return dict(c, g_mean=z if g_mean is None else g_mean, g_var=z if g_var is None else g_var, g_kl=float(g_kl),
                key=c["key"] + (tag,))


def _f64(a):
    return np.asarray(a, np.float64)


def _chol_columns(K):
    """The Cholesky factor by a plain column loop in K's number format."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        s = K[j, j] - L[j, :j] @ L[j, :j]
        assert s > 0, (j, float(s))
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _tri_inverse(L, shadow=False):
    """L^-1 by forward substitution, row by row (tri_inverse_hp's statements) in L's number format; ``shadow``: the
    subtraction becomes an addition -- the inverse of the comparison matrix of |L|."""
    n = L.shape[0]
    X = np.zeros_like(L)
    sg = 1 if shadow else -1
    for i in range(n):
        if i:
            X[i, :i] = sg * (L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = 1 / L[i, i]
    return X


def _gram_operands(c):
    return (dict(x1=c["Zx"], f1=c["zf"], x2=c["Zx"], f2=c["zf"], hyp=c["hyp"]),
            dict(x1=c["Zx"], f1=c["zf"], x2=c["x"], f2=c["f"], hyp=c["hyp"]))


def _gram_df2_abs(c, xdiv, T):
    """(sum_t |d term_t / d f2| of K [n1 x nbase2 xdiv], |d knn / d f2|) of a kind 1 Gram case, in ``T``'s number format."""
    x1, x2, hyp, f1, f2 = T(c["x1"]), T(c["x2"]), T(c["hyp"]), T(c["f1"]), T(c["f2"])
    d = x1.shape[1]
    a1, af, nu, _, lsf = hyp[:5]
    t = (x1[:, None, :] - x2[None, :, :]) / hyp[5:5 + d]
    g1 = np.repeat(T(0.5) * (t * t).sum(-1), xdiv, axis=1)
    fd = f2[None, :] - f1[:, None]
    gf = T(0.5) * (fd / lsf) ** 2
    return (np.abs(a1 * np.exp(-g1) * nu * f1[:, None]) + np.abs(a1 * np.exp(-(g1 + gf)) * af * fd / (lsf * lsf)),
            np.abs(2 * a1 * nu * f2))


def _layer_forward(c, T):
    """(state, shadow state) of the forward in the number format ``T`` converts to.  As a layer of a model (_model_run) ``c``
    may hold "sf", the shadow of its f column [N']: f then carries an error of u sf, which the leaves it enters -- K_mn and
    k_nn -- pass on through their derivatives, |d K / d f| sf joining sum |term| and |d knn / d f| sf joining k_nn.
    With "chain" -- a GIVEN chain state -- the statements are _chain_forward's."""
    if c.get("chain") is not None:
        return _chain_forward(c, T)
    M = c["M"]
    cmm, cmn = _gram_operands(c)
    Kmm = _gram(c["kind"], cmm, 1, T)[0] + T(c["jitter"]) * np.eye(M, dtype=T(0.0).dtype)
    Kmn, _, knn, Kabs = _gram(c["kind"], cmn, c["xdiv"], T)
    sknn = knn
    if c.get("sf") is not None:
        dK, dknn = _gram_df2_abs(cmn, c["xdiv"], T)
        Kabs, sknn = Kabs + dK * T(c["sf"])[None, :], knn + dknn * T(c["sf"])
    L = _chol_columns(Kmm)
    m, LS = T(c["m"]), np.tril(T(c["L_S"]))
    out = []
    for sh in (False, True):
        ab = np.abs if sh else (lambda v: v)
        X = _tri_inverse(ab(L), sh)
        A, a, U = X @ (Kabs if sh else Kmn), X @ ab(m), X @ ab(LS)
        mean, C = A.T @ a, U.T @ A
        q, r = (A * A).sum(0), (C * C).sum(0)
        s = sknn + q if sh else knn - q
        pos = s > 0
        if c["branch"] == 0 and not sh:
            s = np.where(pos, s, 0)
        varraw = s + r
        lgL, lgS = np.log(np.diag(L)), np.log(np.diag(LS) ** 2)
        kl = T(0.5) * (2 * ab(lgL).sum() + (ab(lgS).sum() if sh else -lgS.sum()) + (U * U).sum() + (a * a).sum() + (M if sh else -M))
        out.append(dict(L=ab(L), X=X, A=A, a=a, U=U, C=C, LS=ab(LS), q=q, r=r, knn=knn, pos=pos, varraw=varraw, mean=mean,
                        var=varraw if sh else np.maximum(varraw, T(c["min_var"])), kl=kl, Kmm=Kmm))
    return out


def _layer_backward(c, st, sst, T, phi_diag=0.5):
    """(gradients, their shadows) from the forward states.  ``phi_diag``: the factor on Phi's diagonal (1/2; the CPU test's
    mutation drops it).  As a layer of a model ``c`` may hold "s_g_mean" / "s_g_var", the SHADOWS of its upstream gradients,
    which then stand where |g_mean| / |g_var| stand for a layer by itself, and "sf" (see _layer_forward).  With "chain" the
    statements are _chain_backward's."""
    if c.get("chain") is not None:
        return _chain_backward(c, st, sst, T)
    kind, xdiv = c["kind"], c["xdiv"]
    cmm, cmn = _gram_operands(c)
    gm, gkl = T(c["g_mean"]), T(c["g_kl"])
    gv = np.where(st["varraw"] > T(c["min_var"]), T(c["g_var"]), 0)            # clamp_min passes gradient above the floor only
    cgv = gv if c["branch"] else np.where(st["pos"], gv, 0)
    res = []
    for sh, s in ((False, st), (True, sst)):
        ab = np.abs if sh else (lambda v: v)
        sg = 1 if sh else -1
        X, A, a, U, C, L, LS = (s[k] for k in ("X", "A", "a", "U", "C", "L", "LS"))
        g, w, cw, k = ab(gm), ab(gv), ab(cgv), ab(gkl)
        if sh and c.get("s_g_mean") is not None:                              # a layer of a model: the shadows handed down
            g = T(c["s_g_mean"])
            w = np.where(st["varraw"] > T(c["min_var"]), T(c["s_g_var"]), 0)
            cw = w if c["branch"] else np.where(st["pos"], w, 0)
        dC = 2 * C * w[None, :]
        dA = U @ dC + np.outer(a, g) + sg * 2 * A * cw[None, :]
        da = A @ g + k * a
        dU = np.tril(A @ dC.T) + k * U
        dKmn = X.T @ dA
        g_m = X.T @ da
        g_LS = np.tril(X.T @ dU)
        g_LS[np.diag_indices_from(g_LS)] += sg * k / np.diag(LS)
        Y = dA @ A.T + np.outer(da, a) + dU @ U.T
        dL = sg * np.tril(X.T @ Y)
        dL[np.diag_indices_from(dL)] += k / np.diag(L)
        P = np.tril(L.T @ dL)
        P[np.diag_indices_from(P)] *= T(phi_diag)
        Sm = X.T @ P @ X
        dKmm = T(0.5) * (Sm + Sm.T)
        pick = 2 if sh else 0
        bmn = _gram_bwd(kind, cmn, xdiv, dKmn, cw, None, T, c.get("sf") if sh else None)
        bmm = _gram_bwd(kind, cmm, 1, dKmm, None, None, T)
        o = dict(g_m=g_m, g_LS=g_LS, g_hyp=bmn["hyp"][pick] + bmm["hyp"][pick],
                 g_hyp_mn=bmn["hyp"][pick], g_hyp_mm=bmm["hyp"][pick])
        if c["want_dx"]:
            o["g_x"] = bmn["g_x2"][pick]
        if kind == 1:
            o["g_f"] = bmn["g_f2"][pick]
            o["g_zf_mn"], o["g_zf_mm"] = bmn["g_f1"][pick], bmm["g_f1"][pick] + bmm["g_f2"][pick]
            o["g_zf"] = o["g_zf_mn"] + o["g_zf_mm"]
        res.append(o)
    return res


def _gram_df2(c, xdiv, T):
    """(d K / d f2 [n1 x nbase2 xdiv], d knn / d f2), signed, of a kind 1 Gram case (_gram_df2_abs's terms before the magnitudes)."""
    x1, x2, hyp, f1, f2 = T(c["x1"]), T(c["x2"]), T(c["hyp"]), T(c["f1"]), T(c["f2"])
    d = x1.shape[1]
    a1, af, nu, _, lsf = hyp[:5]
    t = (x1[:, None, :] - x2[None, :, :]) / hyp[5:5 + d]
    g1 = np.repeat(T(0.5) * (t * t).sum(-1), xdiv, axis=1)
    fd = f2[None, :] - f1[:, None]
    gf = T(0.5) * (fd / lsf) ** 2
    return a1 * np.exp(-g1) * nu * f1[:, None] - a1 * np.exp(-(g1 + gf)) * af * fd / (lsf * lsf), 2 * a1 * nu * f2


# ---- a layer on a GIVEN chain state (csrc/frozen_predict.hip; tests/frozen_predict_reference.py): c["chain"] = {Linv, LinvT, U,
# UT, a}, float64, is exact data -- no K_mm, no Cholesky, no inverse -- read the way the kernel reads it: A through the L^-T
# array, C through the U array, dA through U^T, dK through L^-1.  The shadow takes the factors' magnitudes and gives them no
# error of their own: it is the shadow of what THIS layer computes, absolute values through every sum and product.  What the
# layer INHERITS -- the error u sf of f from the layer below, the error of the upstream gradients from the layer above -- is
# not sent through those magnitudes again.  Under the workload's conditioning (cond(K_mm) of 1e8 .. 1e9: |L^-1||K| is 1e4 ..
# 1e5 |A|) that charges every inherited error this layer's cancellation a second time and the next layer's a third, and the
# composed figure admits anything.  The layer's outputs are smooth functions of what it inherits, so first order an inherited
# error moves them by the SIGNED derivative, formed in the reference's own format:
#   q = |A|^2, r = |C|^2   S(q) = 2 |A| S(A) (>= A^2: the product's own rounding), where S(A)^2 counts the error of A against S(A)
#                          although it multiplies |A| only.
#   f, forward             |d mean / d f| sf and |d raw / d f| sf with d mean / d f = a^T B, d raw / d f = d k_nn / d f - 2 A . B +
#                          2 C . U^T B, B = L^-1 dK / df.
#   upstream gradients     the layer's gradients are linear in (g_mean, g_var): |d g / d g_mean_j| and |d g / d g_var_j| from one
#                          run each on unit upstream gradients (a column depends on its own pair only), times the shadows
#                          handed down less the magnitudes.
#   f, backward            |d g / d f_j| sf_j by a central difference of the value statements (step 2^-20: its own error is
#                          1e-12 of the derivative in longdouble, and the derivative only scales a bound).
# c["defect"] plants one of frozen_predict_reference.FROZEN_DEFECTS in the values, never in the shadow.
def _chain_forward(c, T, values_only=False):
    M, ch, defect = c["M"], c["chain"], c.get("defect")
    cmn = _gram_operands(c)[1]
    Kmn, _, knn, Kabs = _gram(c["kind"], cmn, c["xdiv"], T)
    X, a, U = T(ch["LinvT"]).T, T(ch["a"]), T(ch["U"])
    A = X @ Kmn
    mean, C = A.T @ a, U.T @ A
    q, r = (A * A).sum(0), (C * C).sum(0)
    if defect == "last_row_out_of_q":
        q = (A[:-1] * A[:-1]).sum(0)
    if defect == "stale_pad_rows":                                          # rows M .. Mr-1 of the A panel keep what K left there
        stale = Kmn[:min(-M % 16, M)]
        q = q + (stale * stale).sum(0)
    varraw = (knn - q) + r
    st = dict(X=X, A=A, a=a, U=U, C=C, q=q, r=r, knn=knn, pos=knn - q > 0, varraw=varraw, mean=mean,
              var=np.maximum(varraw, T(c["min_var"])), kl=T(0.0), Ub=T(ch["UT"]).T, XTb=T(ch["Linv"]).T)
    if values_only:
        return st, None
    aX, aa, aU = np.abs(X), np.abs(a), np.abs(U)
    sA = aX @ Kabs
    sC = aU.T @ sA
    smean, sq, sr = sA.T @ aa, 2 * (np.abs(A) * sA).sum(0), 2 * (np.abs(C) * sC).sum(0)
    svar = knn + sq + sr
    if c.get("sf") is not None:
        dK, dknn = _gram_df2(cmn, c["xdiv"], T)
        B = X @ dK
        smean = smean + np.abs(B.T @ a) * T(c["sf"])
        svar = svar + np.abs(dknn - 2 * (A * B).sum(0) + 2 * (C * (U.T @ B)).sum(0)) * T(c["sf"])
    sst = dict(X=aX, A=sA, a=aa, U=aU, C=sC, q=sq, r=sr, knn=knn, pos=st["pos"], varraw=svar, mean=smean, var=svar, kl=T(0.0),
               Ub=np.abs(st["Ub"]), XTb=np.abs(st["XTb"]))
    return st, sst


def _chain_backward(c, st, sst, T):
    """(g_x, g_f) and their shadows: gv = g_var [raw > floor], dA = 2 U (C gv) + a g_mean - 2 A gv, dK = L^-T dA, the Gram
    backward of K_mn and k_nn.  The factors are constants: nothing else has a gradient."""
    kind, xdiv, defect = c["kind"], c["xdiv"], c.get("defect")
    cmn = _gram_operands(c)[1]
    above = st["varraw"] > T(c["min_var"])                                     # clamp_min passes gradient above the floor only

    def run(s, g, w, sh, case=cmn, div=xdiv):
        dA = s["Ub"] @ (2 * s["C"] * w[None, :]) + np.outer(s["a"], g)
        if sh or defect != "A_gv_dropped":
            dA = dA + (2 if sh else -2) * s["A"] * w[None, :]
        gknn = None if (defect == "dknn_df_dropped" and not sh) else w
        b = _gram_bwd(kind, case, div, s["XTb"] @ dA, gknn, None, T)
        pick = 2 if sh else 0
        return b["g_x2"][pick], (b["g_f2"][pick] if kind == 1 else None)

    gm, gv = T(c["g_mean"]), np.where(above, T(c["g_var"]), 0)
    gx, gf = run(st, gm, T(c["g_var"]) if defect == "floor_gate_ignored" else gv, False)
    sgx, sgf = run(sst, np.abs(gm), np.abs(gv), True)                          # this layer's own: f and the upstream pair exact
    cols = dict(cmn, x2=np.repeat(T(cmn["x2"]), xdiv, axis=0))                 # every column its own base row: no replica sum
    fold = lambda jx, e: (np.abs(jx) * e[:, None]).reshape(c["nbase"], xdiv, -1).sum(1)
    if c.get("s_g_mean") is not None:                                          # a layer of a model: the shadows handed down
        eg = np.maximum(T(c["s_g_mean"]) - np.abs(gm), 0)
        ew = np.where(above, np.maximum(T(c["s_g_var"]) - np.abs(T(c["g_var"])), 0), 0)
        one, zero = np.ones(c["Np"], gm.dtype), np.zeros(c["Np"], gm.dtype)
        for unit_g, unit_w, e in ((one, zero, eg), (zero, np.where(above, one, 0), ew)):
            jx, jf = run(st, unit_g, unit_w, False, cols, 1)
            sgx = sgx + fold(jx, e)
            if kind == 1:
                sgf = sgf + np.abs(jf) * e
    if c.get("sf") is not None:
        h, side = T(2.0 ** -20), []
        for sign in (1, -1):
            fh = T(c["f"]) + sign * h
            side.append(run(_chain_forward(dict(c, f=fh, sf=None, defect=None), T, values_only=True)[0], gm, gv, False, dict(cols, f2=fh), 1))
        sgx = sgx + fold((side[0][0] - side[1][0]) / (2 * h), T(c["sf"]))
        sgf = sgf + np.abs((side[0][1] - side[1][1]) / (2 * h)) * T(c["sf"])
    res = [dict(g_x=gx), dict(g_x=sgx)]
    if kind == 1:
        res[0]["g_f"], res[1]["g_f"] = gf, sgf
    return res


_layer_fwd_cache, _layer_ref_cache = {}, {}


def layer_ref(c, dtype=np.longdouble, shadow=False):
    """{output: value} of the layer ``c`` = layer_case(...) in ``dtype`` -- mean, var [N'], kl, g_m [M], g_LS [M x M, lower],
    g_hyp, g_x [nbase x d] (want_dx), g_f [N'], g_zf [M] (kind 1), and the two shares g_hyp_mn / g_hyp_mm, g_zf_mn / g_zf_mm
    of the PANEL and the CHAIN backward -- or, ``shadow``, the magnitude shadow S of each.  Cached per case and upstream."""
    assert dtype is not np.longdouble or HAVE_LONGDOUBLE
    key = (c["key"], np.dtype(dtype).name)
    if key not in _layer_ref_cache:
        T = lambda a: np.asarray(a, dtype)
        fkey = (c["key"][:10], np.dtype(dtype).name)                       # the forward does not depend on the upstream
        if fkey not in _layer_fwd_cache:
            _layer_fwd_cache[fkey] = _layer_forward(c, T)
        st, sst = _layer_fwd_cache[fkey]
        g, sg = _layer_backward(c, st, sst, T)
        fw = lambda s: {k: s[k] for k in ("mean", "var", "kl", "q", "knn", "varraw", "r")}
        _layer_ref_cache[key] = (dict(fw(st), **g), dict(fw(sst), **sg))
    return _layer_ref_cache[key][1 if shadow else 0]


def layer_oracle(c):
    """The same outputs by float64 autograd over oracle.layer_moments + kl_layer (triangular solves, no explicit inverse)."""
    from oracle import mfdgp_oracle as O
    kind, d, xdiv = c["kind"], c["d"], c["xdiv"]
    t = lambda a: torch.tensor(np.array(a), dtype=torch.float64)
    x, m, LS, hyp = t(c["x"]).requires_grad_(True), t(c["m"]).requires_grad_(True), t(c["L_S"]).requires_grad_(True), t(c["hyp"]).requires_grad_(True)
    f, zf = (t(c["f"]).requires_grad_(True), t(c["zf"]).requires_grad_(True)) if kind == 1 else (None, None)
    xr = x.repeat_interleave(xdiv, 0)
    Zx = t(c["Zx"])
    Xt = xr if kind == 0 else torch.cat([xr, f[:, None]], 1)
    Zt = Zx if kind == 0 else torch.cat([Zx, zf[:, None]], 1)
    hd = hyp_dict(kind, hyp, d)
    mean, var, _ = O.layer_moments(hd, Xt, Zt, m, LS, jitter=c["jitter"], training=(c["branch"] == 0), shortcut=False)
    var = var.clamp_min(c["min_var"])                                      # the oracle's own floor is 1e-10 <= min_var
    kl = O.kl_layer(hd, Zt, m, LS, jitter=c["jitter"])
    ((t(c["g_mean"]) * mean).sum() + (t(c["g_var"]) * var).sum() + c["g_kl"] * kl).backward()
    n = lambda v: v.detach().numpy()
    out = dict(mean=n(mean), var=n(var), kl=n(kl), g_m=n(m.grad), g_LS=np.tril(n(LS.grad)), g_hyp=n(hyp.grad), g_x=n(x.grad))
    if kind == 1:
        out["g_f"], out["g_zf"] = n(f.grad), n(zf.grad)
    return out


def layer_names(c):
    return ("mean", "var", "kl", "g_m", "g_LS", "g_hyp") + (("g_x",) if c["want_dx"] else ()) + (("g_f", "g_zf") if c["kind"] == 1 else ())


def layer_ratios(got, ref, S, names):
    """{output: (worst |got - ref| / (u S) over the components with S > 0, number of components with S = 0 that are not
    exactly zero -- NaN included)}."""
    out = {}
    for k in names:
        g, r, s = ld(got[k]).reshape(np.shape(ref[k])), ld(ref[k]), ld(S[k])
        err = np.abs(g - r)
        pos = s > 0
        with np.errstate(invalid="ignore"):
            ratio = np.where(pos, err / np.where(pos, ld(U) * s, 1), 0)
            ratio = np.where(np.isnan(ratio), np.inf, ratio)
        out[k] = (float(np.max(ratio, initial=0.0)), int(np.sum(~pos & ~(g == 0))))
    return out


def layer_gate(got, ref, S, names, C=None):
    """(violations, {group: worst ratio}, report) of the gate |got - ref| <= C_g u S, S = 0 => exactly zero."""
    C = LAYER_C if C is None else C
    rat = layer_ratios(got, ref, S, names)
    worst, bad = {}, []
    for k, (r, nz) in rat.items():
        g = layer_group(k)
        worst[g] = max(worst.get(g, 0.0), r)
        if not r <= C[g] or nz:
            bad.append((k, r, nz))
    report = "  ".join("%s %.2f u S = %.0f%% of the gate" % (g, w, 100 * w / C[g]) for g, w in worst.items())
    return bad, worst, report


# The cases the GPU conformance tests run and the CPU test proves the conditions and the constants on:
# (kind, d, M, nbase, xdiv, seed, clamp, floor, branch, want_dx).  M: 8 / 127 / 128 (kl_one, substitution Cholesky, Mp = 128),
# 129 (kl_part, blocked Cholesky, Mp = 256), 257 (Mp = 384: an odd row-block count), 400 (Mp = 512: the k-sliced dual syrk);
# N' = nbase xdiv: 12 (one partial block), 128 (exact), 129 (127 padding columns), 300 (several partial rows); clamp = 128
# columns at M = 8: every column of the first block clamped.
LAYER_CASES = [
    (0, 2, 8, 12, 1, 0, 0, False, 0, 1), (0, 2, 8, 300, 1, 0, 128, False, 0, 1), (0, 9, 8, 128, 1, 0, 0, True, 1, 0),
    (0, 2, 8, 129, 1, 1, 0, True, 0, 0), (0, 2, 127, 129, 1, 0, 0, False, 0, 1), (0, 9, 127, 12, 1, 0, 0, False, 1, 0),
    (0, 2, 127, 300, 1, 0, 10, True, 0, 0), (0, 2, 128, 128, 1, 0, 0, False, 0, 0), (0, 2, 128, 300, 1, 0, 5, True, 0, 1),
    (0, 9, 128, 12, 1, 0, 0, False, 1, 1), (0, 2, 129, 300, 1, 0, 0, False, 0, 1), (0, 9, 129, 129, 1, 0, 0, True, 1, 1),
    (0, 2, 129, 12, 1, 0, 4, False, 0, 0), (0, 2, 257, 128, 1, 0, 0, False, 0, 1), (0, 9, 257, 300, 1, 0, 20, False, 0, 0),
    (0, 2, 257, 129, 1, 0, 0, True, 1, 1), (0, 2, 400, 300, 1, 0, 30, False, 0, 1),
    (1, 2, 8, 4, 3, 0, 0, False, 0, 1), (1, 2, 8, 100, 3, 0, 43, False, 0, 1), (1, 9, 8, 16, 8, 0, 0, True, 1, 0),
    (1, 2, 8, 129, 1, 1, 0, True, 0, 0), (1, 2, 127, 43, 3, 0, 0, False, 0, 1), (1, 9, 127, 12, 1, 0, 0, False, 1, 0),
    (1, 2, 127, 100, 3, 0, 8, True, 0, 0), (1, 2, 128, 16, 8, 0, 0, False, 0, 0), (1, 2, 128, 100, 3, 0, 5, True, 0, 1),
    (1, 9, 128, 4, 3, 0, 0, False, 1, 1), (1, 2, 129, 300, 1, 0, 0, False, 0, 1), (1, 9, 129, 43, 3, 0, 0, True, 1, 1),
    (1, 2, 129, 4, 3, 0, 2, False, 0, 0), (1, 2, 257, 16, 8, 0, 0, False, 0, 1), (1, 9, 257, 100, 3, 0, 10, False, 0, 0),
    (1, 2, 257, 129, 1, 0, 0, True, 1, 1), (1, 2, 400, 100, 3, 0, 20, False, 0, 1),
]
LAYER_ACTIVITY_CASES = [(0, 2, 129, 640, 1, 0, 0, False, 0, 1), (1, 2, 129, 80, 8, 0, 0, False, 0, 1)]          # N' = 640: five blocks
LAYER_SPLIT_CASES = [(0, 2, 129, 300, 1, 0, 0, False, 0, 1), (1, 2, 129, 300, 1, 0, 0, False, 0, 1), (1, 2, 129, 43, 3, 1, 0, False, 0, 1)]
LAYER_SPLIT_ONE = (1, 2, 8, 4, 3, 0, 0, False, 0, 1)
LAYER_TUNING_CASES = [c for c in LAYER_CASES if c[2] in (257, 400) and c[1] == 2 and c[8] == 0]
LAYER_UPSTREAM_CASES = [(0, 2, 129, 300, 1, 0, 0, False, 0, 1), (1, 2, 8, 100, 3, 0, 43, False, 0, 1), (1, 2, 128, 100, 3, 0, 5, True, 0, 1)]
LAYER_ACTIVITY = {"first": [1, 0, 0, 0, 0], "one_column": [0, 0, 1, 0, 0], "scattered": [0, 1, 0, 1, 0]}


def activity_case(c, pattern):
    """``c`` (N' = 640) with whole 128-blocks of exactly zero upstream gradients: 'first' -- only the first block active;
    'one_column' -- nothing but g_mean of column 300; 'scattered' -- blocks 1 and 3."""
    mask = column_mask(LAYER_ACTIVITY[pattern], c["Np"])
    if pattern == "one_column":
        one = np.arange(c["Np"]) == 300
        return with_upstream(c, np.where(one, c["g_mean"], 0.0), None, 0.0, tag=pattern), mask
    return with_upstream(c, np.where(mask, c["g_mean"], 0.0), np.where(mask, c["g_var"], 0.0), c["g_kl"], tag=pattern), mask


def all_layer_cases():
    seen, out = set(), []
    for k in LAYER_CASES + LAYER_ACTIVITY_CASES + LAYER_SPLIT_CASES + [LAYER_SPLIT_ONE] + LAYER_UPSTREAM_CASES:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


# ---- direct callers of the layer entry points: pointers and the descriptor (tuning, jitter, min_var, branch, want_dx) pass
# through unchanged; outputs, saved, scratch and chain blocks are NaN before the call; every output has GUARD doubles behind it
GUARD = 8
WORKSPACE_TOO_SMALL = 2                 # MOBOCMF_WORKSPACE_TOO_SMALL


class LayerCall:
    """What a direct layer call leaves behind: ``out`` {name: float64 numpy}, ``rc``, ``info``, ``untouched`` (every guard double
    bitwise as it was), the device buffers a later call of the sequence needs."""


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def _out(n):
    return torch.full((n + GUARD,), NAN, dtype=torch.float64, device="cuda")


def _collect(r, bufs, lens):
    torch.cuda.synchronize()
    nan_bits = torch.full((GUARD,), NAN, dtype=torch.float64, device="cuda").view(torch.int64)
    r.untouched = all(bool(torch.equal(bufs[k][n:].view(torch.int64), nan_bits)) for k, n in lens.items())
    r.out = {k: bufs[k][:n].cpu().numpy() for k, n in lens.items()}
    r.bufs = bufs
    return r


def layer_desc(c, tune=None, params_const=0, **over):
    from mobocmf_amd import _lib
    d = _lib.LayerDesc(kind=c["kind"], d=c["d"], M=c["M"], xdiv=c["xdiv"], Np=c["Np"], branch=c["branch"], want_dx=c["want_dx"],
                       jitter=c["jitter"], min_var=c["min_var"], params_const=params_const, reserved=0)
    for k, v in over.items():
        setattr(d, k, v)
    if tune is not None:
        d.tuning = ctypes.pointer(tune)
    d._tune = tune                                                          # keeps it alive with the descriptor
    return d


def layer_inputs(c):
    return {k: _dev(c[k]) for k in ("x", "f", "Zx", "zf", "hyp", "m", "L_S")}


def _sizes(fn, desc):
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    rc = getattr(lib(), fn)(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(b))
    assert a.value % 8 == 0 and b.value % 8 == 0
    return rc, a.value, b.value


def _grad_lens(c, names):
    n = {"g_hyp": len(c["hyp"]), "g_m": c["M"], "g_LS": c["M"] * c["M"], "g_x": c["nbase"] * c["d"], "g_f": c["Np"], "g_zf": c["M"]}
    return {k: n[k] for k in names if (k != "g_x" or c["want_dx"]) and (k not in ("g_f", "g_zf") or c["kind"] == 1)}


def _shape_out(c, out):
    if "g_LS" in out:
        out["g_LS"] = out["g_LS"].reshape(c["M"], c["M"])
    if "g_x" in out:
        out["g_x"] = out["g_x"].reshape(c["nbase"], c["d"])
    if "kl" in out:
        out["kl"] = out["kl"][0]
    return out


def layer_forward_direct(c, tune=None, desc=None, saved_short=0, size_desc=None):
    """mobocmf_layer_forward with the sizes mobocmf_layer_workspace_bytes reports for the same descriptor (``size_desc``: for
    that one -- a descriptor the size query itself refuses can still be handed to the call)."""
    r = LayerCall()
    r.c, r.desc, r.inp = c, desc if desc is not None else layer_desc(c, tune), layer_inputs(c)
    r.size_rc = _sizes("mobocmf_layer_workspace_bytes", r.desc)[0]
    r.rc, r.sb, r.cb = _sizes("mobocmf_layer_workspace_bytes", r.desc if size_desc is None else size_desc)
    assert r.rc == 0
    r.saved, scratch = _nan_bytes(r.sb), _nan_bytes(r.cb)
    lens = {"mean": c["Np"], "var": c["Np"], "kl": 1}
    bufs = {k: _out(n) for k, n in lens.items()}
    info = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    i = r.inp
    r.rc = lib().mobocmf_layer_forward(ctypes.byref(r.desc), _p(i["x"]), _p(i["f"]), _p(i["Zx"]), _p(i["zf"]), _p(i["hyp"]), _p(i["m"]),
                                       _p(i["L_S"]), _p(bufs["mean"]), _p(bufs["var"]), _p(bufs["kl"]), _p(info), _p(r.saved),
                                       r.sb - saved_short, _p(scratch), r.cb, _stream())
    _collect(r, bufs, lens)
    r.info = int(info[0])
    _shape_out(c, r.out)
    return r


def layer_backward_direct(fw, c=None, null=()):
    """mobocmf_layer_backward over the forward ``fw`` with the upstream gradients of ``c`` (default: the forward's case);
    ``null``: names among g_mean / g_var passed as NULL."""
    c = fw.c if c is None else c
    r = LayerCall()
    lens = _grad_lens(c, ("g_hyp", "g_m", "g_LS", "g_x", "g_f", "g_zf"))
    bufs = {k: _out(n) for k, n in lens.items()}
    scratch = _nan_bytes(fw.cb)
    up = {k: None if k in null else _dev(c[k]) for k in ("g_mean", "g_var")}
    gkl = _dev(np.array([c["g_kl"]]))
    i = fw.inp
    r.rc = lib().mobocmf_layer_backward(ctypes.byref(fw.desc), _p(i["x"]), _p(i["f"]), _p(i["Zx"]), _p(i["zf"]), _p(i["hyp"]), _p(i["m"]),
                                        _p(i["L_S"]), _p(up["g_mean"]), _p(up["g_var"]), _p(gkl), _p(bufs.get("g_f")), _p(bufs.get("g_zf")),
                                        _p(bufs["g_hyp"]), _p(bufs["g_m"]), _p(bufs["g_LS"]), _p(bufs.get("g_x")), _p(fw.saved), fw.sb,
                                        _p(scratch), fw.cb, _stream())
    _collect(r, bufs, lens)
    _shape_out(c, r.out)
    return r


def _desc_table(descs):
    from mobocmf_amd import _lib
    return (ctypes.POINTER(_lib.LayerDesc) * len(descs))(*[ctypes.pointer(d) for d in descs])


def chain_forward_direct(cs, tune=None, descs=None):
    """mobocmf_layers_chain_forward of the layers ``cs`` (equal M) into NaN-filled chain blocks of the size and stride
    mobocmf_chain_block_bytes reports (the chain's descriptors: N' = xdiv = 1, as functional.ChainBatch.chain_desc)."""
    r = LayerCall()
    n = len(cs)
    r.cs, r.tune = cs, tune
    r.descs = descs if descs is not None else [layer_desc(c, tune, Np=1, xdiv=1, want_dx=0) for c in cs]
    r.rc, r.bb, r.st = _sizes("mobocmf_chain_block_bytes", r.descs[0])
    if r.rc:
        return r
    r.stride = (r.bb + 255) // 256 * 256
    r.blocks = _nan_bytes(n * r.stride)
    r.inp = [layer_inputs(c) for c in cs]
    kls = [_out(1) for _ in cs]
    infos = [torch.full((1,), -77, dtype=torch.int32, device="cuda") for _ in cs]
    T = lambda k: _tab([i[k] for i in r.inp])
    r.rc = lib().mobocmf_layers_chain_forward(n, _desc_table(r.descs), T("Zx"), T("zf"), T("hyp"), T("m"), T("L_S"), _tab(kls), _tab(infos),
                                              _p(r.blocks), r.stride, r.blocks.numel(), _stream())
    torch.cuda.synchronize()
    nan_bits = torch.full((GUARD,), NAN, dtype=torch.float64, device="cuda").view(torch.int64)
    r.untouched = all(bool(torch.equal(k[1:].view(torch.int64), nan_bits)) for k in kls)
    r.kl = [float(k[0]) for k in kls]
    r.info = [int(i[0]) for i in infos]
    return r


def chain_block(ch, z, state_only=False):
    return ch.blocks[z * ch.stride:z * ch.stride + (ch.st if state_only else ch.bb)]


def panel_forward_direct(ch, z, c, params_const=0, block=None):
    """mobocmf_layer_panel_forward of layer ``z`` of the chain call ``ch`` (``block``: that byte tensor instead of the layer's
    chain block -- the state alone under params_const)."""
    r = LayerCall()
    r.c, r.z, r.inp = c, z, ch.inp[z]
    r.desc = layer_desc(c, ch.tune, params_const)
    r.block = chain_block(ch, z) if block is None else block
    r.rc, r.sb, r.cb = _sizes("mobocmf_panel_workspace_bytes", r.desc)
    if r.rc:
        return r
    r.saved, scratch = _nan_bytes(r.sb), _nan_bytes(r.cb)
    r.x, r.f = _dev(c["x"]), _dev(c["f"])
    lens = {"mean": c["Np"], "var": c["Np"]}
    bufs = {k: _out(n) for k, n in lens.items()}
    i = r.inp
    r.rc = lib().mobocmf_layer_panel_forward(ctypes.byref(r.desc), _p(r.x), _p(r.f), _p(i["Zx"]), _p(i["zf"]), _p(i["hyp"]), _p(bufs["mean"]),
                                             _p(bufs["var"]), _p(r.block), r.block.numel(), _p(r.saved), r.sb, _p(scratch), r.cb, _stream())
    return _collect(r, bufs, lens)


def panel_backward_direct(pf, c=None):
    """mobocmf_layer_panel_backward over the panel forward ``pf``: g_f, g_x and the K_mn shares of g_hyp / g_zf."""
    c = pf.c if c is None else c
    r = LayerCall()
    lens = _grad_lens(c, ("g_hyp", "g_x", "g_f", "g_zf"))
    bufs = {k: _out(n) for k, n in lens.items()}
    scratch = _nan_bytes(pf.cb)
    gm, gv = _dev(c["g_mean"]), _dev(c["g_var"])
    i = pf.inp
    r.rc = lib().mobocmf_layer_panel_backward(ctypes.byref(pf.desc), _p(pf.x), _p(pf.f), _p(i["Zx"]), _p(i["zf"]), _p(i["hyp"]), _p(gm), _p(gv),
                                              _p(bufs.get("g_f")), _p(bufs.get("g_zf")), _p(bufs["g_hyp"]), _p(bufs.get("g_x")), _p(pf.block),
                                              pf.block.numel(), _p(pf.saved), pf.sb, _p(scratch), pf.cb, _stream())
    _collect(r, bufs, lens)
    _shape_out(c, r.out)
    return r


def chain_backward_direct(ch, g_kl, had_panel, shares=None):
    """mobocmf_layers_chain_backward.  ``shares``[z]: the LayerCall of layer z's panel backward, whose g_hyp / g_zf buffers are
    handed over (had_panel 2: accumulated into) -- None: fresh NaN buffers.  Returns one LayerCall per layer."""
    n = len(ch.cs)
    outs, lens, bufs = [], [], []
    for z, c in enumerate(ch.cs):
        l = _grad_lens(c, ("g_hyp", "g_m", "g_LS", "g_zf"))
        b = {k: _out(m) for k, m in l.items()}
        if shares is not None and shares[z] is not None:
            b["g_hyp"] = shares[z].bufs["g_hyp"]
            if "g_zf" in b:
                b["g_zf"] = shares[z].bufs["g_zf"]
        lens.append(l)
        bufs.append(b)
    gk = [_dev(np.array([g])) for g in g_kl]
    T = lambda k: _tab([i[k] for i in ch.inp])
    B = lambda k: _tab([b.get(k) for b in bufs])
    rc = lib().mobocmf_layers_chain_backward(n, _desc_table(ch.descs), T("Zx"), T("zf"), T("hyp"), _tab(gk), (ctypes.c_int32 * n)(*had_panel),
                                             B("g_zf"), B("g_hyp"), B("g_m"), B("g_LS"), _p(ch.blocks), ch.stride, ch.blocks.numel(), _stream())
    for z, c in enumerate(ch.cs):
        r = LayerCall()
        r.rc = rc
        _collect(r, bufs[z], lens[z])
        _shape_out(c, r.out)
        outs.append(r)
    return outs


# ------------------------------------------------------------------------------------ the one-launch steps: the whole model
# (tiny_step.hip, coop_step.hip; include/mobocmf_hip.h, mobocmf_tiny_model; DESIGN.md, "The model bound".)
#
# model_ref composes the layer statements above -- _layer_forward / _layer_backward, called on every layer of a model -- as
# oracle.model_forward / oracle.elbo do: softplus of the packed raw vector, Z~_l = [Z_x, m_{l-1}], f = mean + sqrt(var) eps with
# the S-fold replication between layer 0 and layer 1, layer l on the first rows[l] rows, the data term of the rows of level l
# (row weights, the mean over S), kl_scale sum KL, seeds at the top layer's columns; backwards the ELBO's gradients, the
# propagation (g_f -> g_mean, g_var of the layer below) and g_zf[l] -> g_m[l-1], the softplus and Interval derivatives.
#
# Its SHADOW composes the same way, and at every joint it hands over the shadow of the quantity, not its magnitude: S(f) =
# S(mean) + S(var) |eps| / (2 sqrt(var)) + |mean| + sqrt(var) |eps|, S(g_mean) = |data term| + |seed| + sum S(g_f), and so on.
# A first-order shadow with exact leaves does not see the error of f: layer l reads f as an input of K_mn and k_nn, so u S(f)
# reaches everything behind them through dK / df.  The shadow is EXTENDED by that term rather than the constants enlarged:
# the leaf sum |term| of K_mn gains |dK / df| S(f), k_nn gains |dk_nn / df| S(f) (_layer_forward, "sf"), and every addend
# |G| |dterm / dtheta| of the Gram backward gains |G| |d^2 term / dtheta df| S(f) (_gram_bwd, sf2).  With S(f) = 0 the model's
# shadow of a layer is layer_ref's.
MODEL_GROUPS = {"forward": ("out", "top_mean", "top_var"), "chain": ("g_m", "g_LS"), "gram": ("g_hyp", "g_x"), "noise": ("g_noise",)}
MODEL_NOISE_LO = 1e-4
# C_g per depth L and group, by the rule of LAYER_C: measured by tests/test_model_reference_cpu.py on every case of the GPU file
# as the larger worst err / (u S) of the float64 run of model_ref and of float64 autograd over the oracle, recorded a quarter
# above the measurement, times 4.  Measured (restatement / oracle, the case of the larger one):
#   L = 1  forward 6.21 / 24.64 (M16_L1_d1_N129: the oracle's x / ls - z / ls on a lattice of spacing 1 / 16), chain 8.44 / 8.85
#          (M32_L1_d8_544), gram 1.30 / 7.24 (M7_L1_d2, the input gradient), noise 0.93 / 0.56 (M1_L1_d1)
#   L = 2  forward 3.61 / 3.90 (M127_L2_d8_N144), chain 5.61 / 9.83 (M16_L2_d8_wide), gram 0.41 / 1.50 (M16_L2_d8_S3, the input
#          gradient), noise 0.75 / 0.75 (M32_L2_d8_S3)
#   L = 3  forward 2.12 / 3.13 (M16_L3_d8_S8), chain 7.06 / 6.95 (clamp_M20), gram 1.35 / 5.18 (M16_L3_d8_S8), noise 0.67 / 0.83
# The oracle's figures depend on the host CPU's vector kernels and BLAS (not on the thread count): another host gave 5.94 (L = 2
# forward), 21.67 (L = 2 chain), 7.53 (L = 1 gram), 1.29 (L = 3 noise) -- all at most 0.44 of C_g.
# At L = 1 the model adds the ELBO and one softplus derivative to a layer, and its figures sit BELOW LAYER_RATIO_MEASURED (17 /
# 165 / 125) because its cases are the one-launch kernels' sizes: the layer's worst ratios come from M = 128 .. 257 at d = 9 and
# from the KL differentiated alone, which no model case does.
MODEL_RATIO_MEASURED = {1: {"forward": 31.0, "chain": 11.1, "gram": 9.1, "noise": 1.16},
                        2: {"forward": 4.9, "chain": 12.3, "gram": 1.9, "noise": 0.95},
                        3: {"forward": 3.9, "chain": 8.8, "gram": 6.5, "noise": 1.05}}
MODEL_C = {L: {k: 4.0 * v for k, v in t.items()} for L, t in MODEL_RATIO_MEASURED.items()}


def model_group(name):
    base = name.rstrip("0123456789")
    return next(g for g, names in MODEL_GROUPS.items() if base in names)


_model_cases, _model_ref_cache = {}, {}


def _inv_softplus(h):
    return h + np.log(-np.expm1(-h))


def model_case(L, d, M, rows, S, seed=0, clamp=0, weights=False, seeds=None, predict=False, zx=None, floor=False):
    """One well-conditioned whole-model problem (cached, read-only): L layers sharing Z_x -- layer_case's jittered lattice (d <=
    3) or uniform points, and its lengthscale ranges, so that cond(K_mm + jitter I) <= LAYER_COND_MAX for every Z~_l = [Z_x,
    m_{l-1}] (asserted by the CPU test).  ``rows`` = (N, rows[1], ...), descending: the rows are in the kernels' order, row b
    has the level of the last layer whose prefix holds it -- rows[l] == rows[l+1] leaves level l without a row.  y of order one;
    explicit eps[l] (rows[l] S); noise Interval(MODEL_NOISE_LO, hi) on the layers with l + seed even, hi <= lo (raw is tau) on
    the others; kl_scale = 0.7.  ``clamp`` = k: the first k rows lie ON inducing rows -- x on Z_x[b % M], and eps chosen so
    that f = m_{l-1}[b % M] in the layers above -- under jitter = CLAMP_JITTER.  ``weights``: row_weight in [0.5, 2], every
    fourth row 0.  ``seeds``: "both" | "mean" | "var" -- seed_gmean / seed_gvar standard normal (the other one zeros),
    seed_scale = -0.75.  ``predict``: the eval branch at N test points: rows[l] = N, no row scored (fid = -1), kl_scale = 0,
    eps[l] = S fixed samples tiled over the points, and every third row's seeds zero.  ``zx`` = "uniform" (d <= 2): Z_x uniform
    in [0, 1]^d with lengthscales 0.4 .. 0.6 under jitter 1e-6 -- the workload's conditioning, cond(K_mm + jitter I) of 1e8 ..
    1e9, which only a reference on the GIVEN chain (frozen_predict_ref) can gate.  ``floor`` (prediction, d = 8): the last test
    point lies ON Z_x[7 % M], L_S of layer 0 is 1e-7 I and jitter 1e-12: that column of layer 0 sits on the variance floor."""
    rows = tuple(int(r) for r in rows)
    key = ("model", L, d, M, rows, S, seed, clamp, weights, seeds, predict) + ((zx, floor) if zx or floor else ())
    if key in _model_cases:
        return _model_cases[key]
    assert len(rows) == L and all(rows[l] >= rows[l + 1] >= 1 for l in range(L - 1)) and not (predict and clamp)
    rng = np.random.default_rng(7919 * L + 1009 * M + 31 * rows[0] + 7 * d + S + 131071 * seed)
    assert zx in (None, "uniform") and not (zx and d > 2) and not (floor and not (predict and d == 8))
    if zx:
        Zx = rng.random((M, d))
        ls = lambda: rng.uniform(0.4, 0.6, d)
    elif d <= 3:
        side = int(np.ceil(M ** (1.0 / d)))
        h = 1.0 / side
        grid = np.stack(np.meshgrid(*[np.arange(side)] * d, indexing="ij"), -1).reshape(-1, d)
        Zx = (grid[rng.permutation(len(grid))[:M]] + 0.5 + 0.15 * rng.uniform(-1, 1, (M, d))) * h
        ls = lambda: h * rng.uniform(0.55, 0.8, d)
    else:
        Zx = rng.random((M, d))
        ls = lambda: rng.uniform(0.25, 0.32, d)
    N = rows[0]
    hyp = [np.concatenate([[0.7 + rng.random()], ls()])]
    for l in range(1, L):
        hyp.append(np.concatenate([[0.6 + rng.random(), 0.5 + rng.random(), 0.5 + rng.random(), 0.05 + 0.1 * rng.random(),
                                    0.7 + rng.random()], ls(), ls()]))
    x = Zx[rng.integers(0, M, N)] + 0.6 * hyp[0][1:] * rng.standard_normal((N, d)) / np.sqrt(d)
    if clamp:
        assert clamp <= N
        x[:clamp] = Zx[np.arange(clamp) % M]
    fid = np.full(N, -1.0) if predict else np.array([sum(rows[l] > b for l in range(L)) - 1.0 for b in range(N)])
    y = np.sin(3 * x.sum(1)) + 0.3 * fid + 0.1 * rng.standard_normal(N)
    interval = [(l + seed) % 2 == 0 for l in range(L)]
    c = dict(L=L, d=d, M=M, rows=rows, S=S, N=N, branch=int(predict), predict=predict, clamp=clamp, key=key,
             jitter=CLAMP_JITTER if clamp else 1e-6, kl_scale=0.0 if predict else 0.7, x=x, y=y, fid=fid, Zx=Zx,
             raw=[_inv_softplus(h_) for h_ in hyp], m=[0.5 * rng.standard_normal(M) for _ in range(L)],
             L_S=[0.2 * np.eye(M) + 0.05 * np.tril(rng.standard_normal((M, M))) for _ in range(L)],
             noise_lo=[MODEL_NOISE_LO if i else 0.0 for i in interval], noise_hi=[0.3 + 0.2 * l if i else 0.0 for l, i in enumerate(interval)],
             raw_noise=[0.5 * rng.standard_normal() if i else 0.05 + 0.1 * rng.random() for i in interval],
             row_weight=None, seed_gmean=None, seed_gvar=None, seed_scale=0.0)
    if floor:
        c["x"] = np.concatenate([x[:-1], Zx[7 % M][None, :]])
        c["L_S"] = [1e-7 * np.eye(M)] + c["L_S"][1:]
        c["jitter"] = 1e-12
    if predict:
        c["samples"] = [None] + [rng.standard_normal(S) for _ in range(1, L)]
        c["eps"] = [None] + [np.tile(s, N) for s in c["samples"][1:]]
    else:
        c["eps"] = [None] + [rng.standard_normal(rows[l] * S) for l in range(1, L)]
    if weights:
        c["row_weight"] = np.where(np.arange(N) % 4 == 3, 0.0, rng.uniform(0.5, 2.0, N))
    if seeds:
        nt = rows[-1] * (S if L > 1 else 1)
        on = (np.arange(nt) // (S if L > 1 else 1)) % 3 != 1 if predict else np.ones(nt, bool)
        c["seed_gmean"] = np.where(on, rng.standard_normal(nt), 0.0) if seeds in ("both", "mean") else np.zeros(nt)
        c["seed_gvar"] = np.where(on, rng.standard_normal(nt), 0.0) if seeds in ("both", "var") else np.zeros(nt)
        c["seed_scale"] = -0.75
    for l in range(1, L if clamp else 0):                       # f = m_{l-1} on the clamped rows of the layers above
        _, st, _ = _model_forward(c, _f64, stop=l)[-1]
        k = min(clamp, rows[l])
        cols, fdiv = np.arange(k * S), S if l == 1 else 1
        e = c["eps"][l].copy()
        e[cols] = (c["m"][l - 1][(cols // S) % M] - st["mean"][cols // fdiv]) / np.sqrt(st["var"][cols // fdiv])
        c["eps"][l] = e
    for v in list(c.values()):
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _model_cases[key] = c
    return c


def _softplus(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def model_layer(mc, l, T, f=None, sf=None, chains=None):
    """Layer ``l`` of the model as a case of the layer statements (layer_case's fields) in ``T``'s number format.  ``chains``
    [l]: the layer's GIVEN chain state (_layer_forward, "chain") with the packed hyper-parameters "hyp" the kernel was handed --
    data like the factors, where the model's own are softplus(raw) in ``T``'s format."""
    nb, xdiv = mc["rows"][l], (mc["S"] if l else 1)
    c = dict(kind=int(l > 0), d=mc["d"], M=mc["M"], nbase=nb, xdiv=xdiv, Np=nb * xdiv, branch=mc["branch"], want_dx=int(mc["predict"]),
             jitter=mc["jitter"], min_var=1e-10, x=mc["x"][:nb], f=f, sf=sf, Zx=mc["Zx"], zf=T(mc["m"][l - 1]) if l else None,
             hyp=_softplus(T(mc["raw"][l])), m=mc["m"][l], L_S=mc["L_S"][l])
    if chains is not None:
        c.update(chain=chains[l], hyp=T(chains[l]["hyp"]), defect=mc.get("defect"))
    return c


def _model_forward(mc, T, stop=None, chains=None):
    """[(layer case, state, shadow state)] of the layers 0 .. stop - 1 (all): the propagation with its shadow; ``chains``: on
    the layers' GIVEN chain states (model_layer)."""
    L, S, rows = mc["L"], mc["S"], mc["rows"]
    out, f, sf = [], None, None
    for l in range(L if stop is None else stop):
        lc = model_layer(mc, l, T, f, sf, chains)
        st, sst = _layer_forward(lc, T)
        out.append((lc, st, sst))
        if l + 1 < L:
            idx = np.arange(rows[l + 1] * S) // (S if l == 0 else 1)
            mean, sd, e = st["mean"][idx], np.sqrt(st["var"][idx]), T(mc["eps"][l + 1])
            f = mean + sd * e
            svar = sst["var"][idx]
            if chains is not None:
                # a column ON the floor (frozen_predict_ref asserts every floor decision robust) holds the constant 1e-10 on both
                # sides: its variance carries no error into f, where S(var) / (2 sqrt(1e-10)) would admit anything
                svar = np.where(st["varraw"][idx] > lc["min_var"], svar, 0)
            sf = sst["mean"][idx] + svar * np.abs(e) / (2 * sd) + np.abs(mean) + sd * np.abs(e)
    return out


def _noise(mc, l, T):
    """(tau, d tau / d raw) of layer l."""
    lo, hi, raw = T(mc["noise_lo"][l]), T(mc["noise_hi"][l]), T(mc["raw_noise"][l])
    if not mc["noise_hi"][l] > mc["noise_lo"][l]:
        return raw, T(1.0)
    sg = 1 / (1 + np.exp(-raw))
    return lo + (hi - lo) * sg, (hi - lo) * sg * (1 - sg)


def model_layout(mc):
    """[(name, start, stop)] of the flat vector (mobocmf_tiny_flat_len): per layer [packed hyper-parameters | m | L_S], then
    raw_noise of every layer."""
    out, o, M = [], 0, mc["M"]
    for l in range(mc["L"]):
        for name, n in (("g_hyp%d" % l, len(mc["raw"][l])), ("g_m%d" % l, M), ("g_LS%d" % l, M * M)):
            out.append((name, o, o + n))
            o += n
    return out + [("g_noise", o, o + mc["L"])]


def model_split(mc, flat):
    return {k: (flat[a:b].reshape(mc["M"], mc["M"]) if k.startswith("g_LS") else flat[a:b]) for k, a, b in model_layout(mc)}


def model_names(mc, what):
    """The outputs a mode leaves: ``what`` = 'forward' | 'gradients' | 'input'."""
    fw = ("out", "top_mean", "top_var")
    return fw + {"forward": (), "input": ("g_x",), "gradients": tuple(k for k, _, _ in model_layout(mc))}[what]


def _model_run(mc, T, loss_only=False, chains=None):
    """(values, shadows, forward states) of the whole model in ``T``'s number format; ``loss_only``: the scalar the gradients
    are of, -ELBO + seed_scale (<seed_gmean, top mean> + <seed_gvar, top var>), from the forward alone.  ``chains``: on the
    layers' GIVEN chain states (model_layer) -- the parameters are constants, so of the gradients only g_x exists."""
    L, S, rows, N = mc["L"], mc["S"], mc["rows"], mc["N"]
    dt = T(0.0).dtype
    fw = _model_forward(mc, T, chains=chains)
    y, fid, ks = T(mc["y"]), mc["fid"], T(mc["kl_scale"])
    w = T(np.ones(N) if mc["row_weight"] is None else mc["row_weight"])
    half, log2pi = T(0.5), T(LOG_2PI)
    data = sdata = kl = skl = T(0.0)
    ups, gn, sgn = [], np.zeros(L, dt), np.zeros(L, dt)
    for l, (lc, st, sst) in enumerate(fw):
        div, nn = lc["xdiv"], lc["Np"]
        b = np.arange(nn) // div
        mask = fid[b] == float(l)
        tau, chain = _noise(mc, l, T)
        dlt, var = y[b] - st["mean"], st["var"]
        sq = dlt * dlt + var
        ssq = dlt * dlt + 2 * np.abs(dlt) * (np.abs(y[b]) + sst["mean"]) + var + sst["var"]
        wb = w[b] / div
        data = data + np.where(mask, -wb * half * (sq / tau + np.log(tau) + log2pi), 0).sum()
        sdata = sdata + np.where(mask, wb * half * (ssq / tau + np.abs(np.log(tau)) + log2pi), 0).sum()
        kl, skl = kl + st["kl"], skl + sst["kl"]
        # d(-ELBO) / d(mean, var, raw_noise) of the rows of level l
        gm, sgm = np.where(mask, -wb * dlt / tau, 0), np.where(mask, wb * (np.abs(y[b]) + sst["mean"]) / tau, 0)
        gv = np.where(mask, half * wb / tau, 0)
        gn[l] = np.where(mask, -wb * half * (sq / (tau * tau) - 1 / tau), 0).sum() * chain
        sgn[l] = np.where(mask, wb * half * (ssq / (tau * tau) + 1 / tau), 0).sum() * np.abs(chain)
        ups.append([gm, gv, sgm, gv.copy()])
    res = dict(out=np.array([data - ks * kl, ks * kl, -(data - ks * kl)], dt), top_mean=fw[-1][1]["mean"], top_var=fw[-1][1]["var"])
    sha = dict(out=np.array([sdata + ks * skl, ks * skl, sdata + ks * skl], dt), top_mean=fw[-1][2]["mean"], top_var=fw[-1][2]["var"])
    if mc["seed_gmean"] is not None:
        sc = T(mc["seed_scale"])
        for i, k in enumerate(("seed_gmean", "seed_gvar")):
            ups[-1][i] = ups[-1][i] + sc * T(mc[k])
            ups[-1][2 + i] = ups[-1][2 + i] + np.abs(sc * T(mc[k]))
    if loss_only:
        seed = 0 if mc["seed_gmean"] is None else sc * ((T(mc["seed_gmean"]) * res["top_mean"]).sum() + (T(mc["seed_gvar"]) * res["top_var"]).sum())
        return res["out"][2] + seed
    gx, sgx = np.zeros((N, mc["d"]), dt), np.zeros((N, mc["d"]), dt)
    flat, sflat = {}, {}
    zshare = (None, None)
    for l in range(L - 1, -1, -1):
        lc, st, sst = fw[l]
        gm, gv, sgm, sgv = ups[l]
        g, sg = _layer_backward(dict(lc, g_mean=gm, g_var=gv, g_kl=ks, s_g_mean=sgm, s_g_var=sgv), st, sst, T)
        if chains is None:
            sig = 1 / (1 + np.exp(-T(mc["raw"][l])))
            flat["g_hyp%d" % l], sflat["g_hyp%d" % l] = g["g_hyp"] * sig, sg["g_hyp"] * sig
            flat["g_m%d" % l], sflat["g_m%d" % l] = g["g_m"], sg["g_m"]
            if zshare[0] is not None:                                      # g_zf of the layer above: Z~_{l+1} = [Z_x, m_l]
                flat["g_m%d" % l], sflat["g_m%d" % l] = g["g_m"] + zshare[0], sg["g_m"] + zshare[1]
            flat["g_LS%d" % l], sflat["g_LS%d" % l] = g["g_LS"], sg["g_LS"]
        if mc["predict"]:
            gx[:rows[l]] += g["g_x"]
            sgx[:rows[l]] += sg["g_x"]
        if l:
            if chains is None:
                zshare = (g["g_zf"], sg["g_zf"])
                res["g_zf%d" % l], sha["g_zf%d" % l] = zshare
            ncn, fdiv = lc["Np"], S if l == 1 else 1                       # this layer's columns feed on the layer below
            k = ncn // fdiv
            _, stb, sstb = fw[l - 1]
            idx = np.arange(ncn) // fdiv
            sd, var, e = np.sqrt(stb["var"][idx]), stb["var"][idx], T(mc["eps"][l])
            fold = lambda a: a.reshape(k, fdiv).sum(1)
            ups[l - 1][0][:k] += fold(g["g_f"])
            ups[l - 1][1][:k] += fold(g["g_f"] * e * half / sd)
            ups[l - 1][2][:k] += fold(sg["g_f"])
            ups[l - 1][3][:k] += fold(sg["g_f"] * np.abs(e) * half / sd + np.abs(g["g_f"] * e) * sstb["var"][idx] / (4 * var * sd))
    flat["g_noise"], sflat["g_noise"] = gn, sgn
    for d_, s_ in ((res, flat), (sha, sflat)):
        d_.update(s_)
        if chains is None:
            d_["grad"] = np.concatenate([np.ravel(s_[k]) for k, _, _ in model_layout(mc)])
    if mc["predict"]:
        res["g_x"], sha["g_x"] = gx, sgx
    return res, sha, fw


def model_ref(mc, dtype=np.longdouble, shadow=False):
    """{output: value} of the model ``mc`` = model_case(...) in ``dtype`` -- out [3], top_mean, top_var [rows[L-1] S], the flat
    gradient 'grad' of d(-ELBO + seed term) / d(raw parameters) in mobocmf_tiny_flat_len's layout and its blocks g_hyp<l>, g_m<l>,
    g_LS<l> [M x M, lower], g_noise [L], g_zf<l> [M], the share of g_m<l-1> that Z~_l = [Z_x, m_{l-1}] sends down; prediction cases: g_x [N x d] -- or, ``shadow``, the composed shadow S of each.  Cached."""
    assert dtype is not np.longdouble or HAVE_LONGDOUBLE
    key = (mc["key"], np.dtype(dtype).name)
    if key not in _model_ref_cache:
        _model_ref_cache[key] = _model_run(mc, lambda a: np.asarray(a, dtype))[:2]
    return _model_ref_cache[key][1 if shadow else 0]


def model_oracle(mc):
    """The same outputs by float64 autograd over the oracle: oracle.elbo for the plain ELBO; with row weights or seeds its
    statements (model_forward, expected_log_prob, kl_layer) with the weights and the seed term; prediction cases through
    oracle.predict (eval_mode, the call inside predict_for_acquisition, whose per-point averages the per-column seeds cannot
    address) less the likelihood noise."""
    from oracle import mfdgp_oracle as O
    L, S, N, d, rows = mc["L"], mc["S"], mc["N"], mc["d"], mc["rows"]
    t = lambda a: torch.tensor(np.array(a), dtype=torch.float64)
    leaf = lambda a: t(a).requires_grad_(True)
    raw, m, LS, rn = [leaf(a) for a in mc["raw"]], [leaf(a) for a in mc["m"]], [leaf(a) for a in mc["L_S"]], [leaf(a) for a in mc["raw_noise"]]
    x = leaf(mc["x"])
    noise = [O.interval(r, lo, hi) if hi > lo else r for r, lo, hi in zip(rn, mc["noise_lo"], mc["noise_hi"])]
    state = {"Zx": t(mc["Zx"]), "noise": noise,
             "layers": [{"hyp": hyp_dict(int(l > 0), O.softplus(raw[l]), d), "m": m[l], "L_S": LS[l]} for l in range(L)]}
    nt = rows[-1] * (S if L > 1 else 1)
    seed = lambda mean, var: mc["seed_scale"] * ((t(mc["seed_gmean"]) * mean[:nt]).sum() + (t(mc["seed_gvar"]) * var[:nt]).sum())
    n = lambda v: v.detach().numpy()
    if mc["predict"]:
        state["samples"] = [None] + [t(s) for s in mc["samples"][1:]]
        Xt = x.repeat_interleave(S if L > 1 else 1, 0)
        mean, var = O.predict(state, Xt, L - 1, training=False, eval_mode=True, jitter=mc["jitter"])
        var = var - noise[L - 1].detach()
        out = dict(out=np.zeros(3), top_mean=n(mean), top_var=n(var))
        if mc["seed_gmean"] is not None:
            seed(mean, var).backward()
            out["g_x"] = n(x.grad)
        return out
    eps = [None] + [t(np.concatenate([mc["eps"][l], np.zeros((N - rows[l]) * S)])) for l in range(1, L)]
    y, fid = t(mc["y"]), t(mc["fid"])
    outs = O.model_forward(state, x, eps=eps, S=S, training=True, jitter=mc["jitter"], shortcut=False)
    if mc["row_weight"] is None and mc["seed_gmean"] is None:
        e, skl = O.elbo(state, x, y, fid, eps=eps, S=S, num_data=N / mc["kl_scale"], jitter=mc["jitter"], shortcut=False)
        loss = -e
    else:
        w = t(np.ones(N) if mc["row_weight"] is None else mc["row_weight"])
        data = 0.0
        for l, (mean, var) in enumerate(outs):
            div = S if l else 1
            mask = (fid == l).repeat_interleave(div)
            if int(mask.sum()):
                data = data + (w.repeat_interleave(div) * O.expected_log_prob(y.repeat_interleave(div), mean, var, noise[l]))[mask].sum() / div
        skl = mc["kl_scale"] * sum(O.kl_layer(state["layers"][l]["hyp"], O.inducing_inputs(state, l), m[l], LS[l], mc["jitter"]) for l in range(L))
        e = data - skl
        loss = -e
        if mc["seed_gmean"] is not None:
            loss = loss + seed(*outs[-1])
    loss.backward()
    z = lambda p: np.zeros(p.shape) if p.grad is None else n(p.grad)
    out = dict(out=np.array([float(e.detach()), float(skl.detach()), -float(e.detach())]), top_mean=n(outs[-1][0])[:nt], top_var=n(outs[-1][1])[:nt],
               g_noise=np.array([float(z(r)) for r in rn]))
    for l in range(L):
        out["g_hyp%d" % l], out["g_m%d" % l], out["g_LS%d" % l] = z(raw[l]), z(m[l]), np.tril(z(LS[l]))
    return out


def model_gate(got, ref, S, names, C):
    """(violations [(name, ratio, non-zeros where S = 0)], {group: worst ratio}, report) of the gate |got - ref| <= C_g u S per
    component with exact zeros where S = 0; ``C``: MODEL_C[L]."""
    rat = layer_ratios(got, ref, S, names)
    worst, bad = {}, []
    for k, (r, nz) in rat.items():
        g = model_group(k)
        worst[g] = max(worst.get(g, 0.0), r)
        if not r <= C[g] or nz:
            bad.append((k, r, nz))
    report = "  ".join("%s %.2f u S = %.0f%% of the gate" % (g, w_, 100 * w_ / C[g]) for g, w_ in worst.items())
    return bad, worst, report


# The cases the one-launch conformance tests run and the CPU test proves the conditions and the constants on: model_case's
# arguments by name.  tiny_step.hip (launch code at the end of the file): MR = 16 up to M = 16, else 32; 512 threads beyond
# M * (widest layer's columns) = 512; the panel pool in LDS while tiny_pool_in_lds() holds.  coop_step.hip (cgeom_of): Mp = M
# rounded up to 16; H inside the backward phase up to 8 column blocks of 16 (N' <= 128), else k-sliced, ks = ceil(N'p / 256)
# capped at 4.  Multi-layer cases at M >= 16 use d = 8 where they can: at d <= 2 a lattice point has 2 .. 8 near neighbours,
# the comparison inverse of |L| grows with M and the composed shadow of the lower layers' gradients with it.
def _mc(L, d, M, rows, S, **kw):
    return dict(L=L, d=d, M=M, rows=rows, S=S, **kw)


MODEL_TINY_CASES = {
    "M1_L1_d1": _mc(1, 1, 1, (3,), 1),                               # MR 16, 256 threads, pool in LDS
    "M7_L2_d2_S3": _mc(2, 2, 7, (12, 5), 3),                         # a prefix layer
    "M16_L3_d8_S8": _mc(3, 8, 16, (20, 9, 1), 8),                    # a top layer of one row; 16 * 72 columns: 512 threads
    "M16_L1_d2": _mc(1, 2, 16, (30,), 1),                            # 480 elements: 256 threads
    "M16_L2_d8_wide": _mc(2, 8, 16, (200, 10), 1),                   # 18 630 pool doubles: panels in `work`
    "M17_L2_d1": _mc(2, 1, 17, (9, 9), 1),                           # MR 32; level 0 has no row
    "M20_L3_d2_S3": _mc(3, 2, 20, (12, 4, 4), 3),                    # level 1 has no row
    "M32_L2_d8_S3": _mc(2, 8, 32, (40, 20), 3),                      # MR 32, 512 threads, panels in `work`
    "M32_L1_d8_512": _mc(1, 8, 32, (16,), 1),                        # exactly 512 elements: still 256 threads
    "M32_L1_d8_544": _mc(1, 8, 32, (17,), 1),                        # 544: 512 threads, pool in LDS
}
MODEL_COOP_CASES = {
    "M5_L3_d2": _mc(3, 2, 5, (12, 12, 5), 1),                        # all layers' m in one wavefront of the gradient assembly; N' = 12
    "M16_L1_d1_N129": _mc(1, 1, 16, (129,), 1),                      # nine column blocks, the last of one column: ks 1
    "M17_L2_d8_N130": _mc(2, 8, 17, (130, 40), 1),
    "M48_L2_d8_S8": _mc(2, 8, 48, (64, 20), 8),                      # layer 1: N' = 160
    "M64_L2_d2_N128": _mc(2, 2, 64, (128, 16), 1),                   # N' = 128: the widest layer that forms H in the backward phase
    "M65_L2_d8_N272": _mc(2, 8, 65, (272, 100), 1),                  # ks 2
    "M127_L2_d8_N144": _mc(2, 8, 127, (144, 144), 1),                # ks 1 in both layers; level 0 has no row
    "M128_L3_d8_S2": _mc(3, 8, 128, (130, 40, 12), 2),
    "M16_L2_d8_N1040": _mc(2, 8, 16, (1040, 30), 1),                 # ks capped at 4
    "M128_L1_d2_N129": _mc(1, 2, 128, (129,), 1),
}
MODEL_FEATURE_CASES = {
    "clamp": _mc(2, 2, 7, (12, 5), 3, clamp=3), "weights_seeds": _mc(2, 2, 7, (12, 5), 3, weights=True, seeds="both"),
    "seed_mean": _mc(2, 2, 7, (12, 5), 3, seeds="mean"), "seed_var": _mc(2, 2, 7, (12, 5), 3, seeds="var"),
    "clamp_M20": _mc(3, 8, 20, (24, 10, 3), 2, clamp=5, weights=True, seeds="both"),
}
MODEL_PREDICT_CASES = {
    "M7_L1_d2": _mc(1, 2, 7, (10,), 1, predict=True, seeds="both"), "M16_L2_d8_S3": _mc(2, 8, 16, (9, 9), 3, predict=True, seeds="both"),
    "M20_L3_d2_S8": _mc(3, 2, 20, (5, 5, 5), 8, predict=True, seeds="both"),
    "M65_L2_d8_S8": _mc(2, 8, 65, (20, 20), 8, predict=True, seeds="both"),          # coop only: N' = 160
}
MODEL_UPDATE_CASES = {"tiny": "M7_L2_d2_S3", "coop": "M17_L2_d8_N130"}
MODEL_GROUP_CASES = {"tiny": ("M7_L2_d2_S3", "M32_L2_d8_S3", "M16_L3_d8_S8"), "coop": ("M5_L3_d2", "M17_L2_d8_N130", "M64_L2_d2_N128")}


def all_model_cases():
    out = {}
    for table in (MODEL_TINY_CASES, MODEL_COOP_CASES, MODEL_FEATURE_CASES, MODEL_PREDICT_CASES):
        out.update(table)
    return out


def named_model_case(name):
    return model_case(**all_model_cases()[name])


def tiny_geometry(mcs):
    """(MR, threads, pool in LDS) of a mobocmf_tiny_elbo_step launch over ``mcs``, restated from tiny_step.hip: geom_of (pool_len),
    lds_bytes, LDS_BUDGET and the launch code of mobocmf_tiny_elbo_step."""
    HS, NVEC = 5 + 2 * 8, 11
    mmax = max(c["M"] for c in mcs)
    MR = 16 if mmax <= 16 else 32
    ms = MR * (MR + 1)
    lds = 8 * (12 * ms + 3 * MR * 9 + 2 * 3 * HS + 3 * 16 + 3 * 3 * MR + 2 * MR + 8 * (HS + 1) + 24 + 32 + 16)
    cols = lambda c: [r * (c["S"] if l else 1) for l, r in enumerate(c["rows"])]
    pool = max(sum(cols(c)) * (2 * c["M"] + NVEC) + 3 * max(c["M"], 8) * max(cols(c)) for c in mcs)
    cmax = max(max(cols(c)) for c in mcs)
    return MR, 512 if mmax * cmax > 512 else 256, lds + 8 * pool <= 160 * 1024 - 512


def coop_geometry(mc):
    """Per layer (hblk, ks) of mobocmf_coop_elbo_step, restated from cgeom_of (coop_step.hip)."""
    out = []
    for l, r in enumerate(mc["rows"]):
        ncp = (r * (mc["S"] if l else 1) + 15) // 16 * 16
        hblk = ncp // 16 <= 8
        out.append((hblk, ncp // 16 if hblk else min(4, max(1, (ncp + 255) // 256))))
    return out


# ---- direct callers of the one-launch steps: mobocmf_tiny_model records filled through the ctypes definitions of _lib, the
# table uploaded, the launch through the C ABI.  work, grad, out, top_mean / top_var are NaN before every launch and have GUARD
# doubles behind them; info is poisoned; sync_words are zeroed once, as the header prescribes, and the status word is read back.
STEP_GRADIENTS, STEP_UPDATE, STEP_FORWARD, STEP_INPUT_GRADIENTS, STEP_CHAIN_VALID = 0, 1, 2, 3, 16
INFO_POISON = -77
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
TRAIN_ALL = 0x3FF                         # raw[l][0..6], m, L_S, raw_noise


class OneLaunch:
    """A group of models set up for mobocmf_tiny_elbo_step (``coop`` False) or mobocmf_coop_elbo_step: ``state[i]`` {name: device
    tensor} -- inputs, parameters, Adam state, steps_done, rng words -- and ``outs[i]`` (work, grad, out, top_mean, top_var,
    info).  ``launch(mode)`` poisons the outputs, launches and collects: ``rc``, ``status`` (coop: the status word), ``wgs_used``,
    and per model ``res[i]`` {out, top_mean, top_var, grad, info} as numpy, ``guards[i]`` (every guard bitwise untouched),
    ``written[i]`` (names of the outputs that are no longer all poison)."""

    def __init__(self, mcs, coop, adam_seed=None, steps=0, trainable=None, over=None):
        from mobocmf_amd import _lib
        self.mcs, self.coop, self.n = list(mcs), coop, len(mcs)
        self.host = (_lib.TinyModel * self.n)()
        self.state, self.outs, self.lens = [], [], []
        L_ = lib()
        for i, mc in enumerate(self.mcs):
            rec, L, M, d, S, N = self.host[i], mc["L"], mc["M"], mc["d"], mc["S"], mc["N"]
            rec.L, rec.M, rec.d, rec.S, rec.N, rec.branch = L, M, d, S, N, mc["branch"]
            rec.kl_scale, rec.jitter, rec.seed_scale = mc["kl_scale"], mc["jitter"], mc["seed_scale"]
            t = {k: _dev(mc[k]) for k in ("x", "y", "fid", "Zx", "row_weight", "seed_gmean", "seed_gvar") if mc[k] is not None}
            for l in range(L):
                rec.rows[l] = mc["rows"][l]
                rec.trainable[l] = TRAIN_ALL if trainable is None else trainable[i][l]
                rec.noise_lo[l], rec.noise_hi[l] = mc["noise_lo"][l], mc["noise_hi"][l]
                off = 0
                for s, n in enumerate([1, d] if l == 0 else [1, 1, 1, 1, 1, d, d]):
                    t["raw%d_%d" % (l, s)] = _dev(mc["raw"][l][off:off + n])
                    rec.raw[l][s] = t["raw%d_%d" % (l, s)].data_ptr()
                    off += n
                t["m%d" % l], t["L_S%d" % l], t["raw_noise%d" % l] = _dev(mc["m"][l]), _dev(mc["L_S"][l]), _dev(np.array([mc["raw_noise"][l]]))
                rec.m[l], rec.L_S[l], rec.raw_noise[l] = (t[k % l].data_ptr() for k in ("m%d", "L_S%d", "raw_noise%d"))
                if l:
                    t["eps%d" % l] = _dev(mc["eps"][l])
                    t["rng%d" % l] = torch.tensor([12345 + l, 7, 3], dtype=torch.int64, device="cuda")      # eps replaces the draw
                    rec.eps[l], rec.rng[l] = t["eps%d" % l].data_ptr(), t["rng%d" % l].data_ptr()
            for k in ("x", "y", "fid", "Zx", "row_weight", "seed_gmean", "seed_gvar"):
                setattr(rec, k, t[k].data_ptr() if k in t else None)
            flat, wb = ctypes.c_int64(), ctypes.c_size_t()
            assert L_.mobocmf_tiny_flat_len(ctypes.byref(rec), ctypes.byref(flat)) == 0 and flat.value == model_layout(mc)[-1][2]
            assert getattr(L_, "mobocmf_coop_work_bytes" if coop else "mobocmf_tiny_work_bytes")(ctypes.byref(rec), ctypes.byref(wb)) == 0
            assert wb.value % 8 == 0
            if adam_seed is None:
                am, av = np.zeros(flat.value), np.zeros(flat.value)
            else:
                rng = np.random.default_rng(adam_seed + i)
                am, av = 0.01 * rng.standard_normal(flat.value), 1e-4 * rng.random(flat.value) + 1e-6
            t["adam_m"], t["adam_v"] = _dev(am), _dev(av)
            t["steps_done"] = torch.tensor([steps], dtype=torch.int64, device="cuda")
            rec.adam_m, rec.adam_v, rec.steps_done = t["adam_m"].data_ptr(), t["adam_v"].data_ptr(), t["steps_done"].data_ptr()
            nt = mc["rows"][-1] * (S if L > 1 else 1)
            lens = dict(work=wb.value // 8, grad=max(flat.value, N * d) if mc["predict"] else flat.value, out=3, top_mean=nt, top_var=nt)
            o = {k: _out(n) for k, n in lens.items()}
            o["info"] = torch.full((L + GUARD,), INFO_POISON, dtype=torch.int32, device="cuda")
            for k in o:
                setattr(rec, k, o[k].data_ptr())
            self.state.append(t)
            self.outs.append(o)
            self.lens.append(lens)
        if over is not None:
            over(self.host)
        self.table = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).cuda()
        self.sync = torch.zeros(16 * (self.n + 1), dtype=torch.int64, device="cuda") if coop else None
        torch.cuda.synchronize()

    def snapshot(self):
        torch.cuda.synchronize()
        return [{k: v.clone() for k, v in t.items()} for t in self.state]

    def changed(self, before):
        """Per model the names of the state tensors whose bytes differ from the snapshot ``before``."""
        torch.cuda.synchronize()
        bits = lambda v: v.view(torch.int64)
        return [sorted(k for k, v in t.items() if not torch.equal(bits(v), bits(before[i][k]))) for i, t in enumerate(self.state)]

    def launch(self, mode, wgs_per_model=0, keep=()):
        """``keep``: outputs NOT poisoned before this launch (MOBOCMF_STEP_CHAIN_VALID reads the `work` of the launch before)."""
        for o in self.outs:
            for k, v in o.items():
                if k not in keep:
                    v.fill_(INFO_POISON if k == "info" else NAN)
        torch.cuda.synchronize()
        host, table, a = ctypes.cast(self.host, ctypes.c_void_p), ctypes.c_void_p(self.table.data_ptr()), ADAM
        if self.coop:
            used = ctypes.c_int32(-1)
            self.rc = lib().mobocmf_coop_elbo_step(host, table, self.n, wgs_per_model, _p(self.sync), a["lr"], a["beta1"], a["beta2"], a["eps"],
                                                   mode, ctypes.byref(used), _stream())
            self.wgs_used = used.value
        else:
            self.rc = lib().mobocmf_tiny_elbo_step(host, table, self.n, a["lr"], a["beta1"], a["beta2"], a["eps"], mode, _stream())
        torch.cuda.synchronize()
        self.status = int(self.sync[16 * self.n + 1]) if self.coop else 0
        nan_bits = torch.full((GUARD,), NAN, dtype=torch.float64, device="cuda").view(torch.int64)
        self.res, self.guards, self.written = [], [], []
        for i, (mc, o, lens) in enumerate(zip(self.mcs, self.outs, self.lens)):
            lens = dict(lens)
            if mode & ~STEP_CHAIN_VALID == STEP_INPUT_GRADIENTS:
                lens["grad"] = mc["N"] * mc["d"]
            ok = all(bool(torch.equal(o[k][n:n + GUARD].view(torch.int64), nan_bits)) for k, n in lens.items())
            ok = ok and bool((o["info"][mc["L"]:] == INFO_POISON).all())
            if mode & ~STEP_CHAIN_VALID == STEP_INPUT_GRADIENTS:                  # nothing of grad beyond N d either
                ok = ok and bool(torch.isnan(o["grad"][lens["grad"]:]).all())
            self.guards.append(ok)
            self.written.append(sorted(k for k in lens if not bool(torch.isnan(o[k][:lens[k]]).all()))
                                + (["info"] if not bool((o["info"] == INFO_POISON).all()) else []))
            r = {k: o[k][:n].cpu().numpy() for k, n in lens.items() if k != "work"}
            r["info"] = o["info"][:mc["L"]].cpu().numpy()
            if "grad" in r and mode & ~STEP_CHAIN_VALID == STEP_INPUT_GRADIENTS:
                r["g_x"] = r.pop("grad").reshape(mc["N"], mc["d"])
            self.res.append(r)
        return self

    def params(self, i):
        """The flat vector of the parameters of model i, the layout of grad / adam_m / adam_v."""
        t, mc = self.state[i], self.mcs[i]
        parts = []
        for l in range(mc["L"]):
            parts += [t["raw%d_%d" % (l, s)] for s in range(2 if l == 0 else 7)] + [t["m%d" % l], t["L_S%d" % l].reshape(-1)]
        return torch.cat(parts + [t["raw_noise%d" % l] for l in range(mc["L"])]).cpu().numpy()


def tiny_direct(mcs, mode, **kw):
    """mobocmf_tiny_elbo_step over the models ``mcs`` in ``mode``; keywords: OneLaunch's.  Returns the OneLaunch."""
    return OneLaunch(mcs, False, **kw).launch(mode)


def coop_direct(mcs, mode, wgs_per_model=0, **kw):
    """mobocmf_coop_elbo_step likewise, with ``wgs_per_model`` workgroups per model (0: the library's choice)."""
    return OneLaunch(mcs, True, **kw).launch(mode, wgs_per_model)


def model_got(mc, r, what):
    """The outputs of ``r`` = OneLaunch.res[i] under model_names(mc, what)'s names."""
    out = {k: r[k] for k in ("out", "top_mean", "top_var")}
    if what == "gradients":
        out.update(model_split(mc, r["grad"]))
    elif what == "input":
        out["g_x"] = r["g_x"]
    return out
