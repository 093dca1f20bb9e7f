"""The references of the kernel conformance tests, checked on the CPU alone (tests/kernel_reference.py).

* Exactness proof: for every shape the GPU tests run, the int64 result equals the float64 CPU result bitwise and the sum of
  |a||b| behind any output -- an upper bound of every partial sum in every order -- is below 2^53.  So the GPU tests may ask
  for torch.equal under every tuning.
* The Gram constant c of the componentwise Gram bound is measured here, on the float64 CPU restatement against the
  longdouble reference, and compared with the constant recorded in kernel_reference.py.
* The longdouble ELBO reference against a plain float64 restatement.
* The product dispatch refuses, on the host, the sizes no kernel takes.
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
