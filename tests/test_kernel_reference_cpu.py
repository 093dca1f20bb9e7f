"""The references of the kernel conformance tests, checked on the CPU alone (tests/kernel_reference.py).

* Exactness proof: for every shape the GPU tests run, the int64 result equals the float64 CPU result bitwise and the sum of
  |a||b| behind any output -- an upper bound of every partial sum in every order -- is below 2^53.  So the GPU tests may ask
  for torch.equal under every tuning.
* The Gram constant c of the componentwise Gram bound is measured here, on the float64 CPU restatement against the
  longdouble reference, and compared with the constant recorded in kernel_reference.py.
* The longdouble ELBO reference against a plain float64 restatement.
* The product dispatch refuses, on the host, the sizes no kernel takes.
* The factorisation chain: float64 restatements of every algorithm of chol.hip (substitution-form Cholesky with the
  reciprocal-root multiply, the one-launch form's explicit-inverse panels, the three inverses) stay within HALF of the
  a-priori bounds of kernel_reference.py on every case the GPU tests run; the explicit-inverse panels exceed the classical
  bound (why that form has its own); tri_inverse_hp against mpmath; and slightly wrong references trip each checker.
"""
import numpy as np
import pytest
import torch

from oracle import mfdgp_oracle as O
from tests import kernel_reference as R

LIMIT = 2 ** 53


def test_extended_precision_is_available():
    assert R.HAVE_LONGDOUBLE or __import__("mpmath")
    A, B = np.random.default_rng(0).standard_normal((5, 7)), np.random.default_rng(1).standard_normal((7, 3))
    assert np.abs(np.asarray(R.matmul_hp(A, B), np.float64) - A @ B).max() < 1e-14


def test_derived_magnitude_bounds():
    """Entries in [-4, 4], Kd <= 4096, Mr <= 1280: |sum| <= 2^18 for the plain product and every epilogue, column sums of
    squares <= 2^47, the weighted syrk (three factors) <= 2^18 at Kd = 2176 -- all far below 2^53."""
    assert 4 * 4 * 4096 == 2 ** 16
    assert 4 * (4 * 4 * 4096) + 2 * 4 * 4 + 4 * 4 * 4 <= 2 ** 18 + 2 ** 8        # |2 C| of the dA epilogue
    assert (2 ** 16) ** 2 * 1280 <= 2 ** 47
    assert 4 * 4 * 4 * 2176 <= 2 ** 18
    assert max(max(s) for s in R.gemm_shapes()) <= 1280 and max(R.SYRK_KD) <= 4096 and max(R.EPI_MR) <= 1280


@pytest.mark.parametrize("shape", R.gemm_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_exact_gemm_inputs_are_exact(shape):
    Mr, Nc, Kd = shape
    for tri in R.TRI_FLAGS:
        if not R.tri_ok(tri, Mr, Nc, Kd):
            continue
        A, B = R.gemm_operands(Mr, Nc, Kd, tri)
        Ci = R.imatmul(A, B)
        assert np.array_equal(R.fmatmul(A, B), Ci)
        assert R.exactness_margin(A, B) <= 2 ** 18 < LIMIT
        Cf = A.astype(np.float64) @ B.astype(np.float64)
        assert np.array_equal(Cf, Ci.astype(np.float64))
        assert np.array_equal(Ci.astype(np.float64).astype(np.int64), Ci)
    # the scaled variant: row scales on A, column scales on B -- the product is the integer product times both
    A, B = R.gemm_operands(Mr, Nc, Kd, 0)
    rs, cs = R.tile_scales(Mr, 64, 5), R.tile_scales(Nc, 64, 6)
    Cf = (A.astype(np.float64) * rs[:, None]) @ (B.astype(np.float64) * cs[None, :])
    assert np.array_equal(Cf, R.fmatmul(A, B).astype(np.float64) * rs[:, None] * cs[None, :]) and np.isfinite(Cf).all()


def test_tile_scales_separate_neighbouring_tiles():
    s = R.tile_scales(1152, 128, 3)
    e = np.log2(s)
    assert np.array_equal(e, np.round(e)) and np.abs(e).max() <= 100
    blocks = e[::128]
    assert np.all(np.abs(np.diff(blocks)) >= 150) and all(np.all(e[i:i + 128] == e[i]) for i in range(0, 1152, 128))


@pytest.mark.parametrize("Mr", R.EPI_MR)
def test_exact_epilogue_inputs_are_exact(Mr):
    for Nc in sorted(set(R.EPI_NC_TILED + R.EPI_NC_PANEL)):
        for tri in (0, 1, 2):
            for scaled in (None, "rows", "cols"):
                c = R.epilogue_case(Mr, Nc, tri, scaled=scaled)
                x = R.epilogue_inputs(c)
                assert R.exactness_margin(c["A"], c["B"]) <= 2 ** 18
                if scaled is None:
                    assert np.array_equal(R.imatmul(c["A"], c["B"]), R.fmatmul(c["A"], c["B"]))
                for epi in (1, 2):
                    if (epi, scaled) in ((1, "rows"), (2, "cols")):
                        continue            # that scaling would be summed over by this epilogue's partial rows
                    ref, ri = R.epilogue_ref(c, epi), R.epilogue_ref_int(c, epi)
                    assert max(int(np.abs(v).max()) for v in ri.values()) < LIMIT
                    AB = x["A"] @ x["B"]                                      # float64 BLAS, any order
                    if epi == 1:
                        C = R.EPI_ALPHA * AB
                        assert np.array_equal(C, ref["C"])
                        assert np.array_equal((C * C).sum(0), ref["colsq"]) and int(ri["colsq4"].max()) <= 4 * 2 ** 47
                        assert np.array_equal(x["avec"] @ C, ref["coldot"])
                    else:
                        C = R.EPI_ALPHA * x["bscale"][None, :] * AB + x["avec"][:, None] * x["gmu"][None, :] \
                            - 2.0 * x["Aaux"] * x["cgv"][None, :]
                        assert np.array_equal(C, ref["C"])
                        assert np.array_equal(x["Aaux"] @ x["gmu"], ref["rowdot"])
                    assert all(np.isfinite(v).all() for v in ref.values())


@pytest.mark.parametrize("Mr", R.SYRK_MR)
def test_exact_syrk_inputs_are_exact(Mr):
    for Kd in R.SYRK_KD:
        for pat, scaled in [("all", False), ("all", True)] + [(p, False) for p in ("none", "first", "last")]:
            c = R.syrk_case(Mr, Kd, kact=R.ACTIVITY[pat](Kd // 128), scaled=scaled)
            Aw = c["A"] * c["w"][None, :]
            assert R.exactness_margin(Aw, c["A"].T) <= 2 ** 18
            if pat == "all" and not scaled:
                assert np.array_equal(R.imatmul(Aw, c["A"].T), R.fmatmul(Aw, c["A"].T))
            Af = c["A"].astype(np.float64) * c["rs"][:, None]
            H = (Af * c["w"].astype(np.float64)[None, :]) @ Af.T
            ref = R.syrk_ref(c)
            assert np.array_equal(H, ref) and np.array_equal(ref, ref.T) and np.isfinite(ref).all()
            if pat == "none":
                assert not ref.any()


def test_unused_block_poison_marks_whole_blocks_only():
    a = np.tril(np.ones((384, 384)))
    p = R.unused_block_poison(a, lower=True)
    assert np.isnan(p[0, 128]) and np.isnan(p[127, 383]) and np.isnan(p[255, 256]) and p[0, 127] == 0 and p[200, 255] == 0
    assert np.isnan(p).sum() == 3 * 128 * 128 and np.array_equal(np.nan_to_num(p), a)
    q = R.unused_block_poison(a.T.copy(), lower=False)
    assert np.array_equal(np.isnan(q), np.isnan(p).T)


# ---------------------------------------------------------------------------------------------------------- Gram constant
def _oracle_gram(kind, c, xdiv):
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    d = c["x1"].shape[1]
    h = t(c["hyp"])
    x2 = t(c["x2"]).repeat_interleave(xdiv, 0)
    if kind == 0:
        return O.gram({"alpha": h[0], "ls": h[1:]}, t(c["x1"]), x2).numpy()
    hyp = {"a1": h[0], "af": h[1], "nu": h[2], "a2": h[3], "lsf": h[4], "ls1": h[5:5 + d], "ls2": h[5 + d:]}
    X1 = torch.cat([t(c["x1"]), t(c["f1"])[:, None]], 1)
    X2 = torch.cat([x2, t(c["f2"])[:, None]], 1)
    return O.gram(hyp, X1, X2).numpy()


def test_gram_constant_is_the_measured_one():
    """Worst err / ((2 + |arg|) 2^-53 sum|term|) of the float64 CPU restatement over the Gram cases of the GPU test; the
    recorded GRAM_RATIO_MEASURED must cover it and not be stale (within a factor of two), and GRAM_C is four times it."""
    worst = {}
    for kind in (0, 1):
        for d in R.GRAM_D:
            for xdiv in (1, 3):
                c = R.gram_case(kind, d, 33, 129, xdiv)
                K, W, _ = R.gram_hp(kind, c, xdiv)
                bad, ratio = R.gram_violations(_oracle_gram(kind, c, xdiv), K, W, c=np.inf)
                assert bad == 0                     # only the absolute condition of the underflowing elements can count here
                worst[(kind, d)] = max(worst.get((kind, d), 0.0), ratio)
                assert float(np.abs(K).max()) > 0.1              # entries of order one beside the underflowing ones
                if kind == 0 and d == 32:
                    assert float((W / np.abs(K)).max()) > 1000     # |arg| in the thousands
    w = max(worst.values())
    print("gram ratios", {k: round(v, 2) for k, v in worst.items()}, "worst", w)
    assert w <= R.GRAM_RATIO_MEASURED <= 2.0 * w, worst
    assert R.GRAM_C == 4.0 * R.GRAM_RATIO_MEASURED


# ---------------------------------------------------------------------------------------------------------- Gram backward
def _autograd_gram_bwd(kind, c, xdiv, G, gknn, active):
    """float64 torch autograd of sum G . gram + sum gknn . gram_diag over the oracle: {output: gradient} as numpy."""
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    d = c["x1"].shape[1]
    Np = c["x2"].shape[0] * xdiv
    Gm = np.asarray(G, np.float64)
    if active is not None:
        Gm = np.where(R.column_mask(active, Np)[None, :], Gm, 0.0)
    h = t(c["hyp"]).requires_grad_(True)
    x2 = t(c["x2"]).requires_grad_(True)
    xr = x2.repeat_interleave(xdiv, 0)
    if kind == 0:
        hyp = {"alpha": h[0], "ls": h[1:]}
        X1, X2, leaves = t(c["x1"]), xr, (h, x2)
    else:
        hyp = {"a1": h[0], "af": h[1], "nu": h[2], "a2": h[3], "lsf": h[4], "ls1": h[5:5 + d], "ls2": h[5 + d:]}
        f1, f2 = t(c["f1"]).requires_grad_(True), t(c["f2"]).requires_grad_(True)
        X1, X2, leaves = torch.cat([t(c["x1"]), f1[:, None]], 1), torch.cat([xr, f2[:, None]], 1), (h, x2, f1, f2)
    L = (t(Gm) * O.gram(hyp, X1, X2)).sum()
    if gknn is not None:
        L = L + (t(gknn) * O.gram_diag(hyp, X2)).sum()
    g = torch.autograd.grad(L, leaves)
    out = {"hyp": g[0].numpy(), "g_x2": g[1].numpy()}
    if kind == 1:
        out["g_f1"], out["g_f2"] = g[2].numpy(), g[3].numpy()
    return out


def _gram_bwd_cpu_cases():
    """(kind, d, xdiv, with gknn, activity) at 33 x 129 base rows: both kinds, every d, xdiv 1 and 3, with and without gknn,
    and one activity mask per (kind, d) -- 387 columns are four blocks, the last a partial one."""
    for kind in (0, 1):
        for d in R.GRAM_D:
            for xdiv in (1, 3):
                for with_knn in (False, True):
                    yield kind, d, xdiv, with_knn, None
            yield kind, d, 3, True, [1, 0, 0, 1]


def _apart(c, seed):
    """``c`` with the columns gram_case put next to rows of x1 (|x - z| ~ 1e-3) moved to fresh uniform points.  The oracle
    forms x / ls - z / ls: an absolute rounding of 2 u |x| / ls, which is 2 u |x| / |x - z| RELATIVE to the d/dx and d/dls addends
    G K (x - z) / ls^2 -- with |x - z| down to 1e-4 in one coordinate that alone is 1e-12 .. 1e-11 of A (measured: up to 5.3e-12 A
    at d = 32), the oracle's own error and no statement about the reference.  The formulas are compared where the oracle is
    accurate; the constant and the cancellation are measured on gram_case as it is."""
    c = dict(c, x2=c["x2"].copy())
    k = min(c["x1"].shape[0], c["x2"].shape[0], 5)
    c["x2"][:k] = np.random.default_rng(4242 + seed).random((k, c["x2"].shape[1]))
    return c


@pytest.fixture(scope="module")
def gram_bwd_cpu():
    """Per case of _gram_bwd_cpu_cases: (reference, numpy float64 restatement) on gram_case, (reference, autograd) on the same
    case with the near-coincident columns moved apart; computed once."""
    res = {}
    for kind, d, xdiv, with_knn, act in _gram_bwd_cpu_cases():
        c = R.gram_case(kind, d, 33, 129, xdiv)
        G, gk = R.gram_bwd_inputs(33, 129 * xdiv, seed=d + xdiv, active=act)
        gk = gk if with_knn else None
        ca = _apart(c, d)
        res[(kind, d, xdiv, with_knn, None if act is None else tuple(act))] = (
            R.gram_bwd_hp(kind, c, xdiv, G, gk, act), R.gram_bwd_f64(kind, c, xdiv, G, gk, act),
            R.gram_bwd_hp(kind, ca, xdiv, G, gk, act), _autograd_gram_bwd(kind, ca, xdiv, G, gk, act))
    return res


def test_gram_backward_reference_matches_autograd(gram_bwd_cpu):
    """The longdouble reference equals float64 autograd of the oracle's gram (+ gram_diag) to 1e-12 A per component, every
    output of every case; an inactive block of G may hold NaN."""
    for key, (_, _, ref, auto) in gram_bwd_cpu.items():
        assert set(ref) == set(auto) == ({"hyp", "g_x2"} if key[0] == 0 else set(R.GRAM_BWD_OUTPUTS)), key
        for k, (v, W, A) in ref.items():
            err = np.abs(R.ld(auto[k]).reshape(v.shape) - v)
            assert bool(np.all(err <= R.ld(1e-12) * A)), (key, k, float(np.max(err / np.maximum(A, R.ld(1e-300)))))
            assert bool(np.all(W >= 2 * A)) and bool(np.all(A >= np.abs(v) * (1 - 1e-15)))
    c = R.gram_case(1, 3, 33, 129, 3)
    G, gk = R.gram_bwd_inputs(33, 387, seed=6, active=[1, 0, 0, 1])
    Gn = G.copy()
    Gn[:, 128:384] = np.nan
    a, b = R.gram_bwd_hp(1, c, 3, G, gk, [1, 0, 0, 1]), R.gram_bwd_hp(1, c, 3, Gn, gk, [1, 0, 0, 1])
    assert all(np.array_equal(a[k][i], b[k][i]) for k in a for i in range(3))
    assert not a["g_f2"][2][128:384].any() and a["g_f2"][2][:128].all()


def test_gram_backward_constant_is_the_measured_one(gram_bwd_cpu):
    """Worst err / (2^-53 W) of the float64 restatement (kernel_reference.gram_bwd_f64: direct differences, as the device
    forms them) over the cases above: GRAM_BWD_RATIO_MEASURED covers it and is not stale (within a factor of two);
    GRAM_BWD_C is four times it."""
    worst = {}
    for key, (ref, f64, _, _) in gram_bwd_cpu.items():
        bad, ratio, _ = R.gram_bwd_violations({k: v[0] for k, v in f64.items()}, ref, {k: 0 for k in ref}, c=np.inf)
        assert bad == 0, key
        worst[key[:2]] = max(worst.get(key[:2], 0.0), ratio)
    w = max(worst.values())
    print("gram backward ratios", {k: round(v, 2) for k, v in worst.items()}, "worst", w)
    assert w <= R.GRAM_BWD_RATIO_MEASURED <= 2.0 * w, worst
    assert R.GRAM_BWD_C == 4.0 * R.GRAM_BWD_RATIO_MEASURED


def test_gram_backward_bound_bites_where_the_layer_tolerance_does_not(gram_bwd_cpu):
    """Some component of each kind cancels by more than a factor 100 (A / |ref|): a bound on 2^-53 A there is orders of
    magnitude below 1e-7 of the value's norm."""
    for kind in (0, 1):
        canc = max(float(np.max(np.where(np.abs(v) > 0, A / np.where(np.abs(v) > 0, np.abs(v), 1), 0)))
                   for key, (ref, _, _, _) in gram_bwd_cpu.items() if key[0] == kind for v, W, A in ref.values())
        print(f"kind {kind}: worst cancellation {canc:.3g}")
        assert canc > 100


def test_gram_backward_depth_follows_the_launch():
    """gram_bwd_depth on the geometry the size query reports: the three reduction forms and the formula per output."""
    assert [R.sum_form(*a) for a in ((15, 10), (16, 10), (63, 10), (64, 4096), (64, 4097), (1024, 3))] == [0, 2, 2, 1, 2, 1]
    assert [R.sum_depth(*a) for a in ((15, 10), (16, 10), (63, 10), (64, 4096), (1024, 3), (257, 3))] == [15, 6, 18, 10, 13, 11]
    nbytes, geo = R.gram_bwd_geometry(1, 3, 33, 257, 8, True)
    assert geo == (3, 8, 8) and nbytes % 256 == 0
    D = R.gram_bwd_depth(1, 3, 33, 257, 8, geo)
    assert D == {"hyp": 8 + 8 + 8 + 6 + (6 + 2), "g_f1": 8 + 9 + 6 + 3, "g_f2": 8 + 3 + 6 + 8, "g_x2": 8 + 8 + 2 + 6 + 8}
    _, geo = R.gram_bwd_geometry(0, 2, 512, 8192, 1, True)
    assert geo == (64, 16, 32) and R.gram_bwd_depth(0, 2, 512, 8192, 1, geo) == {"hyp": 1 + 32 + 8 + 6 + 13, "g_x2": 1 + 32 + 2 + 6 + 6}


# ---------------------------------------------------------------------------------------------------------- ELBO reference
def test_elbo_reference_matches_a_float64_restatement():
    rng = np.random.default_rng(4)
    B = 37
    y, fid = rng.standard_normal(B), rng.integers(0, 3, B).astype(np.float64)
    layers = []
    for l, (div, rows, lo, hi) in enumerate([(1, B, 1e-4, 2.0), (3, 20, 0.0, 0.0), (8, 0, 1e-4, 1.0)]):
        layers.append(dict(mean=rng.standard_normal(B * div), var=rng.random(B * div) + 0.1, raw=0.3 + 0.1 * l, lo=lo, hi=hi,
                           div=div, rows=rows))
    kls = [0.5, 1.25]
    ref = R.elbo_hp(layers, y, fid, kls, 0.37, 1.0, None)
    data = 0.0
    for l, lay in enumerate(layers):
        tau = lay["lo"] + (lay["hi"] - lay["lo"]) / (1 + np.exp(-lay["raw"])) if lay["hi"] > lay["lo"] else lay["raw"]
        for i in range(lay["rows"] * lay["div"]):
            b = i // lay["div"]
            if fid[b] == l:
                data += -0.5 * (((y[b] - lay["mean"][i]) ** 2 + lay["var"][i]) / tau + np.log(tau) + np.log(2 * np.pi)) / lay["div"]
    assert abs(float(ref["out3"][0]) - (data - 0.37 * 1.75)) < 1e-12 * abs(data)
    assert float(ref["out3"][1]) == pytest.approx(0.37 * 1.75, rel=1e-15) and ref["out3"][2] == -ref["out3"][0]
    assert np.isnan(np.asarray(ref["g_mean"][1], np.float64)[20 * 3:]).all() and not np.isnan(np.asarray(ref["g_mean"][1], np.float64)[:60]).any()
    assert np.isnan(np.asarray(ref["g_mean"][2], np.float64)).all() and float(ref["g_kl"]) == pytest.approx(-0.37)
    # g_raw against a central difference of the data term in the raw parameter
    h = 1e-6
    def total(raw0):
        ls = [dict(l) for l in layers]
        ls[0]["raw"] = raw0
        return float(R.elbo_hp(ls, y, fid, kls, 0.37, 1.0, None)["out3"][0])
    fd = (total(layers[0]["raw"] + h) - total(layers[0]["raw"] - h)) / (2 * h)
    assert float(ref["g_raw"][0]) == pytest.approx(fd, rel=1e-6)


@pytest.mark.parametrize("shape,trans_b,tune_kw", R.GEMM_DECLINED,
                         ids=[f"{'x'.join(map(str, s))}-t{t}{'-forced' if kw else ''}" for s, t, kw in R.GEMM_DECLINED])
def test_gemm_declined_shapes_are_refused_on_the_host(shape, trans_b, tune_kw):
    """A size no product kernel takes under the given tuning is refused by the dispatch itself, before anything is launched:
    MOBOCMF_BAD_ARG without a device (the k-slicing heuristic once divided by a tile count of zero at these shapes)."""
    import ctypes

    from mobocmf_amd import _lib
    Mr, Nc, Kd = shape
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # never dereferenced on the host
    tune = R.make_tuning(**tune_kw)
    rc = _lib.load().mobocmf_gemm_f64(0, trans_b, Mr, Nc, Kd, p, Kd, p, Kd if trans_b else Nc, p, Nc, ctypes.c_double(1.0), 0,
                                      ctypes.byref(tune), None)
    assert rc == R.BAD_ARG


# ------------------------------------------------------------------------------------------------ factorisation chain
# float64 restatements of the algorithms of chol.hip, run through the checkers the GPU tests use.  Each must stay at or below
# HALF of its bound on every (family, n) the GPU tests run: where one did not, the case would change, never the constant.
def _chol_recip(K, drop=None):
    """Unblocked right-looking Cholesky with the reciprocal-root multiply (l_ij = s_ij r_j, l_jj = s_jj r_j, r_j = 1 / sqrt(s_jj):
    two roundings, inside the 2 u allowed for rsqrt_nr).  drop = (i0, i1, j): the update of rows i0:i1 by column j is left out."""
    S = np.array(K, np.float64)
    n = S.shape[0]
    for j in range(n):
        r = 1.0 / np.sqrt(S[j, j])
        S[j:, j] *= r
        l = S[j + 1:, j].copy()
        if drop is not None and drop[2] == j:
            l[max(drop[0] - j - 1, 0):max(drop[1] - j - 1, 0)] = 0.0
            S[j + 1:, j + 1:] -= np.outer(l, S[j + 1:, j])
        else:
            S[j + 1:, j + 1:] -= np.outer(l, l)
    return np.tril(S)


def _inv_recip(L):
    """Inverse of a small lower triangle by substitution with a reciprocal diagonal, row i from the rows above."""
    m = L.shape[0]
    X = np.zeros((m, m))
    for i in range(m):
        r = 1.0 / L[i, i]
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) * r
        X[i, i] = r
    return X


def _block_explicit(A, m):
    """One diagonal block by panels of width m formed as PRODUCTS with the explicit inverse of the pivot block (m = 16 inside
    a 64-block: potrf_coop_kernel part (A); the pivot tile itself by _chol_recip / _inv_recip as chol_inv_tile16 does), and the
    block's inverse assembled as X_sc = -X_ss sum_t L_st X_tc.  Returns (L, X)."""
    S = np.array(A, np.float64)
    n = S.shape[0]
    X = np.zeros((n, n))
    for s0 in range(0, n, m):
        s1 = min(s0 + m, n)
        Lss = _chol_recip(S[s0:s1, s0:s1])
        Xss = _inv_recip(Lss)
        S[s0:s1, s0:s1] = Lss
        S[s1:, s0:s1] = S[s1:, s0:s1] @ Xss.T
        S[s1:, s1:] -= S[s1:, s0:s1] @ S[s1:, s0:s1].T
        X[s0:s1, s0:s1] = Xss
        if s0:
            X[s0:s1, :s0] = -(Xss @ (S[s0:s1, :s0] @ X[:s0, :s0]))
    return np.tril(S), X


def _chol_explicit(K):
    """Blocked Cholesky as the one-launch form runs it: 64-column steps, the diagonal block by _block_explicit(16), EVERY
    block below it as a product with the block's computed inverse, the trailing update as one product per step.  Returns
    (L, X) with X holding the explicit inverses on its diagonal 64-blocks (zero elsewhere)."""
    S = np.array(K, np.float64)
    n = S.shape[0]
    X = np.zeros((n, n))
    for j0 in range(0, n, 64):
        j1 = min(j0 + 64, n)
        LJ, XJ = _block_explicit(S[j0:j1, j0:j1], 16)
        S[j0:j1, j0:j1] = LJ
        X[j0:j1, j0:j1] = XJ
        S[j1:, j0:j1] = S[j1:, j0:j1] @ XJ.T
        S[j1:, j1:] -= S[j1:, j0:j1] @ S[j1:, j0:j1].T
    return np.tril(S), X


def _trtri(L, route):
    """launch_trtri_z restated: 64-block inverses by substitution, level 0 [[D0, 0], [-D1 (L10 D0), D1]] per 128-block, then
    recursive doubling X21 = -X22 (L21 X11) ('doubling': power-of-two block counts) or block row by block row ('rows').
    The matrix is padded to a multiple of 128 with the identity, as the device pads it."""
    n = L.shape[0]
    Mp = (n + 127) // 128 * 128
    Lp = np.eye(Mp)
    Lp[:n, :n] = np.tril(L)
    X = np.zeros((Mp, Mp))
    for o in range(0, Mp, 128):
        D0, D1 = _inv_recip(Lp[o:o + 64, o:o + 64]), _inv_recip(Lp[o + 64:o + 128, o + 64:o + 128])
        X[o:o + 64, o:o + 64], X[o + 64:o + 128, o + 64:o + 128] = D0, D1
        X[o + 64:o + 128, o:o + 64] = -(D1 @ (Lp[o + 64:o + 128, o:o + 64] @ D0))
    nb = Mp // 128
    if route == "doubling":
        assert nb & (nb - 1) == 0
        sz = 128
        while sz < Mp:
            for o in range(0, Mp, 2 * sz):
                T = Lp[o + sz:o + 2 * sz, o:o + sz] @ X[o:o + sz, o:o + sz]
                X[o + sz:o + 2 * sz, o:o + sz] = -(X[o + sz:o + 2 * sz, o + sz:o + 2 * sz] @ T)
            sz *= 2
    else:
        for i in range(1, nb):
            o = 128 * i
            T = Lp[o:o + 128, :o] @ X[:o, :o]
            X[o:o + 128, :o] = -(X[o:o + 128, o:o + 128] @ T)
    return X[:n, :n]


def _trtri_right_looking(L, Xd):
    """The one-launch form's own inverse (potrf_coop_kernel, the inverse workgroups) restated: right-looking in 64-blocks,
    S_ic = sum_{t < i} L_it X_tc accumulated in X's own storage as the block rows complete, X_jc = -X_jj S_jc, X_jj = the
    explicit inverse of the diagonal block (the diagonal 64-blocks of ``Xd``)."""
    n = L.shape[0]
    X = np.zeros((n, n))
    for j0 in range(0, n, 64):
        j1 = min(j0 + 64, n)
        Xjj = Xd[j0:j1, j0:j1]
        X[j0:j1, :j0] = 0.0 - Xjj @ X[j0:j1, :j0]
        X[j0:j1, j0:j1] = Xjj
        X[j1:, :j1] += L[j1:, j0:j1] @ X[j0:j1, :j1]
    return X


def _cases():
    return [(f, n) for n in R.FACTOR_ORDERS + (R.FACTOR_ORDER_COOP_CAPS,) for f in R.factor_families(n)]


def test_factor_cases_have_the_stated_conditioning():
    for f, n in _cases():
        K, y = R.factor_case(f, n)
        assert K.shape == (n, n) and y.shape == (n,) and np.array_equal(K, K.T) and np.isfinite(K).all()
        if f == "rbf" and n >= 15:
            w = np.linalg.eigvalsh(K)
            assert 1e6 <= w[-1] / w[0] <= 1e9, (n, w[-1] / w[0])
            assert K.min() > 0
        if f == "signed":
            w = np.linalg.eigvalsh(K)
            assert w[-1] / w[0] < 100 and np.array_equal(K, np.round(K)) and (n < 3 or K.min() < 0 < K.max())
            assert np.abs(K).max() < 2 ** 20
        if f == "rbf_scaled":
            K0, y0 = R.factor_case("rbf", n)
            D = R.tile_scales(n, 64, 17 * n)
            assert np.array_equal(K, D[:, None] * K0 * D[None, :]) and np.array_equal(y, D * y0)       # (exact scalings)
            assert np.array_equal(K / D[:, None] / D[None, :], K0)
            assert 2.0 ** -201 < np.abs(K[K != 0]).min() and np.abs(K).max() < 2.0 ** 201


def test_tri_inverse_hp_matches_an_mpmath_inverse():
    import mpmath
    n = 40
    L = np.linalg.cholesky(R.factor_case("rbf", 40)[0])
    X = R.tri_inverse_hp(L)
    mpmath.mp.dps = 50
    Xm = mpmath.inverse(mpmath.matrix(L.tolist()))
    aX = np.abs(np.asarray(X, np.float64))
    Rb = aX @ np.abs(L) @ aX
    for i in range(n):
        for j in range(n):
            ref = Xm[i, j]
            if j > i:
                assert X[i, j] == 0 and abs(ref) < mpmath.mpf(10) ** -30
                continue
            # the reference's own error, n 2^-64 |X||L||X| when longdouble carries it; compared at 50 digits
            err = abs(mpmath.mpf(float(X[i, j])) + mpmath.mpf(float(X[i, j] - np.longdouble(float(X[i, j])))) - ref)
            assert err <= (n + 2) * 2.0 ** -64 * Rb[i, j] * (1 if R.HAVE_LONGDOUBLE else 2 ** 11), (i, j)


_worst = {}


@pytest.mark.parametrize("family,n", _cases(), ids=lambda v: str(v))
def test_factor_restatements_stay_within_half_of_each_bound(family, n):
    """Worst fractions of the bound over all cases (printed per case; this machine, numpy float64 against longdouble):
    substitution-form Cholesky 0.39 of (k + 8) u |L||L^T| (rbf, n = 192, at k = 1; 2.2 .. 3.9 u R on the rbf families, up to
    16.5 u R at k in the hundreds on ``signed``), explicit-inverse Cholesky 0.39 of its own bound (41 .. 1053 u R on the rbf
    families from n = 63 on: far outside the classical bound; 3 .. 5.4 u R on ``signed``, where it keeps the classical one too),
    inverse by recursive doubling / block rows / the one-launch form's right-looking sweep 0.2 .. 4.63 in units of
    u |X||L||X| (4.63 at n = 640) against n + 8, at most 0.035 of the bound, a = L^-1 y at most 2.1 of n + 2, mll at most 2.8 of n + 8 (both worst where n + . is >= 130).  The
    two routes of the inverse agree to the printed digits: their products differ in shape, not in the terms they sum."""
    K, y = R.factor_case(family, n)
    L = _chol_recip(K)
    ok, ru, frac = R.chol_check(L, K)
    assert ok and frac <= 0.5, (ru, frac)
    _worst["sub"] = max(_worst.get("sub", 0), frac)
    Le, Xe = _chol_explicit(K)
    ok, rue, frace = R.chol_check(Le, K, Xe)
    assert ok and frace <= 0.5, (rue, frace)
    _worst["exp"] = max(_worst.get("exp", 0), frace)
    Xhp = R.tri_inverse_hp(L)
    nb = (n + 127) // 128
    routes = ("doubling", "rows") if nb & (nb - 1) == 0 else ("rows",)
    ri = {}
    for route in routes:
        X = _trtri(L, route)
        ok, ri[route] = R.trinv_check(X, L, Xhp)
        assert ok and ri[route] <= 0.5 * (n + R.TRINV_CX), (route, ri[route])
        _worst["inv"] = max(_worst.get("inv", 0), ri[route])
        _worst["invfrac"] = max(_worst.get("invfrac", 0), ri[route] / (n + R.TRINV_CX))
    if R.one_launch_runs(n, 0):
        ok, ri["one launch"] = R.trinv_check(_trtri_right_looking(Le, Xe), Le)
        assert ok and ri["one launch"] <= 0.5 * (n + R.TRINV_CX), ri
        _worst["inv"] = max(_worst["inv"], ri["one launch"])
    a = X @ y
    ok, ra = R.solve_check(a, X, y)
    assert ok and ra <= 0.5 * (n + 2), ra
    mll = float(-0.5 * (a * a).sum() - np.log(np.diag(L)).sum() - 0.5 * n * np.log(2 * np.pi))
    ok, rm = R.mll_check(mll, L, a)
    assert ok and rm <= 0.5 * (n + R.MLL_CLOG), rm
    print("n=%d %s: chol %.2f uR (%.3f of bound), explicit %.2f uR (%.3f of its bound), inverse %s uR, a %.2f, mll %.2f; worst so far %s"
          % (n, family, ru, frac, rue, frace, {k: round(v, 2) for k, v in ri.items()}, ra, rm,
             {k: round(v, 3) for k, v in _worst.items()}))


@pytest.mark.parametrize("family", ("rbf", "signed"))
@pytest.mark.parametrize("n", R.PREDICT_N)
def test_predict_restatement_stays_within_half_of_its_bound(family, n):
    K, y = R.factor_case(family, n)
    L = _chol_recip(K)
    X = _trtri(L, "rows")
    a = X @ y
    for nt in R.PREDICT_NT:
        Kts, kss = R.cross_kernel(family, n, nt)
        A = X @ Kts
        okm, rm, okv, rv = R.predict_check(a @ A, kss - (A * A).sum(0), X, a, Kts, kss)
        assert okm and okv and max(rm, rv) <= 0.5 * (2 * n + 4), (nt, rm, rv)


def test_explicit_inverse_panels_exceed_the_classical_bound():
    """Why the one-launch form carries a bound of its own: the restatement of its panels -- products with the computed
    inverse of the diagonal block -- misses the classical (k + 8) u |L||L^T| on the workload's own conditioning, while the
    substitution form on the same matrix keeps it and the explicit form keeps ITS bound."""
    K, _ = R.factor_case("rbf", 257)
    Le, Xe = _chol_explicit(K)
    ok, ru, frac = R.chol_check(Le, K)
    print("explicit-inverse panels against the classical bound: %.1f u R, %.2f of the bound" % (ru, frac))
    assert not ok and frac > 1.0
    assert R.chol_check(Le, K, Xe)[0] and R.chol_check(_chol_recip(K), K)[0]


# ---- the bounds bite: a reference that is deliberately, slightly wrong trips the assertion
@pytest.mark.parametrize("family", R.FACTOR_FAMILIES)
def test_mutation_one_sign_in_a_tile_of_the_factor(family):
    K, _ = R.factor_case(family, 129)
    L = _chol_recip(K)
    assert R.chol_check(L, K)[0]
    for (i, j) in ((40, 5), (128, 70), (127, 127)):
        Lm = L.copy()
        Lm[i, j] = -Lm[i, j]
        assert not R.chol_check(Lm, K)[0], (i, j)
    Le, Xe = _chol_explicit(K)
    Le[100, 66] = -Le[100, 66]
    assert not R.chol_check(Le, K, Xe)[0]


@pytest.mark.parametrize("family", R.FACTOR_FAMILIES)
def test_mutation_one_dropped_trailing_update(family):
    """Column 63's update of the last 64-block's rows alone is left out (one of 128 terms of those entries)."""
    K, _ = R.factor_case(family, 193)
    assert R.chol_check(_chol_recip(K), K)[0]
    with np.errstate(invalid="ignore"):
        Lm = _chol_recip(K, drop=(128, 192, 63))
    # (at the rbf families' conditioning the missing term makes a later pivot negative; ``signed`` stays finite, so there it
    # is the bound that notices)
    assert family != "signed" or np.isfinite(Lm).all()
    assert not R.chol_check(Lm, K)[0]


@pytest.mark.parametrize("family", R.FACTOR_FAMILIES)
def test_mutation_one_row_of_the_inverse_off_by_1e12(family):
    K, y = R.factor_case(family, 129)
    L = _chol_recip(K)
    X = _trtri(L, "rows")
    Xhp = R.tri_inverse_hp(L)
    assert R.trinv_check(X, L, Xhp)[0]
    for row in (0, 70, 128):
        Xm = X.copy()
        Xm[row] *= 1 + 1e-12
        assert not R.trinv_check(Xm, L, Xhp)[0], row
    a = X @ y
    am = a.copy()
    am[77] *= 1 + 1e-9
    assert R.solve_check(a, X, y)[0] and not R.solve_check(am, X, y)[0]
    mll = float(-0.5 * (a * a).sum() - np.log(np.diag(L)).sum() - 0.5 * 129 * np.log(2 * np.pi))
    assert R.mll_check(mll, L, a)[0] and not R.mll_check(mll * (1 + 1e-11), L, a)[0]
