"""The three product entry points on EXACT inputs: bitwise equal to the CPU reference under every tuning.

Operands are integers in [-4, 4] (times powers of two along dimensions the output does not sum over), so every partial sum
is exactly representable and the float64 result is independent of summation order, FMA use, k-slicing, slab reduction and
tile shape (proved on the references alone in tests/test_kernel_reference_cpu.py).  torch.equal is therefore the assertion:
a wrong k-slice, pairing partner or partial row cannot hide below a tolerance, and with the scaled variant a wrong tile
cannot hide behind a louder one.  Every output and every slack region (columns width..ld, the doubles in front of an offset
base) starts as NaN: slack that is still NaN shows no stray write, a finite exact output shows no stray read.
"""
import itertools

import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = lambda a: np.asarray(a, np.float64)
LAYOUTS = ((0, 0), (2, 2))            # (columns of slack per row, doubles in front of the base): contiguous | ld > width, 16-byte base


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def _gemm_case(shape, tune_kw, scaled=False, poison_unused=False, flags=None, trans_bs=(0, 1)):
    Mr, Nc, Kd = shape
    tune = R.make_tuning(**tune_kw)
    rs = R.tile_scales(Mr, 64, 5) if scaled else np.ones(Mr)
    cs = R.tile_scales(Nc, 64, 6) if scaled else np.ones(Nc)
    C0 = F64(R.exact_ints((Mr, Nc), 9)) * rs[:, None] * cs[None, :]
    ran = 0
    for tri in R.TRI_FLAGS:
        if not R.tri_ok(tri, Mr, Nc, Kd) or (poison_unused and tri == 0):
            continue
        Ai, Bi = R.gemm_operands(Mr, Nc, Kd, tri)
        prod = dev(F64(R.fmatmul(Ai, Bi)) * rs[:, None] * cs[None, :])
        Af, Bf = F64(Ai) * rs[:, None], F64(Bi) * cs[None, :]
        if poison_unused:             # NaN where the contract says nothing is read: whole 128-blocks beyond the diagonal
            if tri & 3:
                Af = R.unused_block_poison(Af, lower=bool(tri & 1))
            if tri & 12:
                Bf = R.unused_block_poison(Bf, lower=bool(tri & 4))
        c0 = dev(C0)
        for (pad, off), trans_b in itertools.product(LAYOUTS, trans_bs):
            A = R.Strided(Mr, Kd, pad, off, fill=Af)
            B = R.Strided(Nc, Kd, pad, off, fill=Bf.T) if trans_b else R.Strided(Kd, Nc, pad, off, fill=Bf)
            C = R.Strided(Mr, Nc, pad, off)
            for alpha, acc in (flags or itertools.product((1.0, -0.5), (0, 1))):
                C.poison()
                if acc:
                    C.set(C0)
                R.gemm(A, B, C, Mr, Nc, Kd, tri=tri, trans_b=trans_b, alpha=alpha, accumulate=acc, tune=tune)
                want = alpha * prod + (c0 if acc else 0.0)
                what = f"tri={tri} trans_b={trans_b} alpha={alpha} acc={acc} pad={pad} off={off} {tune_kw}"
                assert torch.equal(C.view, want), what + ": %d elements differ" % int((C.view != want).sum())
                assert C.slack_untouched(), what + ": stray write"
                ran += 1
    assert ran > 0


_FAMILY_CASES = [(fam, s, kw) for fam, cases in R.GEMM_FAMILIES.items() for s, kw in cases]


@pytest.mark.parametrize("family,shape,tune_kw", _FAMILY_CASES,
                         ids=[f"{f}-{'x'.join(map(str, s))}{'-forced' if kw.get('small_gemm_max') else ''}" for f, s, kw in _FAMILY_CASES])
def test_gemm_families_are_exact(family, shape, tune_kw):
    """Every family at its smallest shapes and on both sides of the default thresholds (384 | 448..1024 | 1152), crossed with
    the chain's tri flags (where the operand is square), trans_b, alpha, accumulate, and two layouts."""
    _gemm_case(shape, tune_kw)


@pytest.mark.parametrize("shape,tune_kw", [((384, 384, 384), {}), ((640, 640, 640), dict(mid_gemm_waves=32)),
                                           ((640, 640, 640), dict(mid_gemm_waves=4)), ((1152, 128, 128), R.TILED),
                                           ((256, 256, 256), dict(R.TILED, small_panel_max=16))],
                         ids=["small", "mid32", "mid4", "tiled", "tiled_square"])
def test_gemm_scaled_tiles_are_exact(shape, tune_kw):
    """Rows of A and columns of B times 2^e, e constant on 64-blocks and >= 2^160 apart between neighbours: a quiet tile that
    is wrong is a failure here, where a max-norm would not see it."""
    _gemm_case(shape, tune_kw, scaled=True, flags=[(1.0, 0), (-0.5, 1)])


@pytest.mark.parametrize("shape,tune_kw", [((384, 384, 384), {}), ((16, 16, 16), {}), ((512, 512, 512), dict(mid_gemm_waves=32)),
                                           ((640, 640, 640), dict(mid_gemm_waves=8)), ((640, 640, 640), dict(mid_gemm_waves=4)),
                                           ((256, 256, 256), dict(R.TILED, small_panel_max=16)),
                                           ((1152, 128, 128), R.TILED)],
                         ids=["small", "small16", "mid32", "mid8", "mid4", "tiled_square", "tiled"])
def test_triangular_operand_contract(shape, tune_kw):
    """include/mobocmf_hip.h at mobocmf_gemm_f64: the unused triangle holds zeros; 128 x 128 blocks wholly inside it are never
    read.  Those blocks hold NaN here, the rest of the unused triangle zeros, and every family must return the exact product."""
    _gemm_case(shape, tune_kw, poison_unused=True, flags=[(1.0, 0)])


@pytest.mark.parametrize("shape,tune_kw", R.GEMM_PANEL, ids=["x".join(map(str, s)) for s, _ in R.GEMM_PANEL])
def test_gemm_panel_widths_below_a_tile_are_exact(shape, tune_kw):
    """Nc < 128 under the plain entry point: only the whole-block panel kernel takes it (A B form; dense and triangular A).
    (512, 48, 512) with the default tuning is the shape at which the k-slicing heuristic of the dispatch counted zero tiles."""
    _gemm_case(shape, tune_kw, trans_bs=(0,))
    _gemm_case(shape, tune_kw, scaled=True, flags=[(-0.5, 1)], trans_bs=(0,))


@pytest.mark.parametrize("shape,trans_b,tune_kw", R.GEMM_DECLINED,
                         ids=[f"{'x'.join(map(str, s))}-t{t}{'-forced' if kw else ''}" for s, t, kw in R.GEMM_DECLINED])
def test_gemm_declined_shapes_return_bad_arg(shape, trans_b, tune_kw):
    """include/mobocmf_hip.h at mobocmf_gemm_f64: a size no kernel takes under the given tuning is MOBOCMF_BAD_ARG, and
    nothing is written."""
    Mr, Nc, Kd = shape
    A = R.Strided(Mr, Kd, fill=np.ones((Mr, Kd)))
    B = R.Strided(Nc, Kd, fill=np.ones((Nc, Kd))) if trans_b else R.Strided(Kd, Nc, fill=np.ones((Kd, Nc)))
    C = R.Strided(Mr, Nc, 2, 2)
    rc = R.gemm(A, B, C, Mr, Nc, Kd, trans_b=trans_b, tune=R.make_tuning(**tune_kw), check=False)
    torch.cuda.synchronize()
    assert rc == R.BAD_ARG, rc
    assert bool(torch.isnan(C.back).all())


# ------------------------------------------------------------------------------------------------------------- epilogues
def _activity(pat, Nc):
    # one word per STARTED 128 columns (the panel kernel takes widths that are no multiple of 128: the last word governs the rest)
    return None if pat is None else torch.tensor(R.ACTIVITY[pat](-(-Nc // 128)), dtype=torch.int32, device=DEV)


def _epilogue_case(Mr, Nc, tri, tune_kw, panel, scaled_for=None, poison_unused=False, pats=(None, "all", "none", "first", "last"),
                   epis=(0, 1, 2), sos=(0, 1), layouts=LAYOUTS):
    tune = R.make_tuning(**tune_kw)
    nan = lambda *s: torch.full(s, R.NAN, dtype=torch.float64, device=DEV)
    for epi in epis:
        scaled = None if scaled_for is None else scaled_for[epi]
        c = R.epilogue_case(Mr, Nc, tri, scaled=scaled)
        x, ref = R.epilogue_inputs(c), {k: dev(v) for k, v in R.epilogue_ref(c, epi).items()}
        Af = R.unused_block_poison(x["A"], lower=(tri == 1)) if poison_unused else x["A"]
        avec, bscale, gmu, cgv = dev(x["avec"]), dev(x["bscale"]), dev(x["gmu"]), dev(x["cgv"])
        for (pad, off), so, pat in itertools.product(layouts, sos, pats):
            A, B = R.Strided(Mr, Mr, pad, off, fill=Af), R.Strided(Mr, Nc, pad, off, fill=x["B"])
            C = R.Strided(Mr, Nc, pad, off)
            act = _activity(pat, Nc)
            live = torch.ones(Nc, dtype=torch.bool, device=DEV) if act is None else act.bool().repeat_interleave(128)[:Nc]
            what = f"epi={epi} tri={tri} Mr={Mr} Nc={Nc} so={so} act={pat} pad={pad} off={off} {tune_kw}"
            kw = {}
            if epi == 1:
                rows = R.colstat_rows(tri, Mr, Nc, Mr, tune)
                assert rows == 2 * (Mr // 128) if panel or tune_kw.get("tile_rows") == 128 else rows == 2 * (Mr // 64), what
                kw = dict(colsq=nan(rows, Nc), coldot=nan(rows, Nc), avec=avec)
            if epi == 2:
                parts = Nc // 16 if panel else 2 * (Nc // 128)
                Aaux = R.Strided(Mr, Nc, pad, off, fill=x["Aaux"])
                kw = dict(avec=avec, bscale=bscale, gmu=gmu, cgv=cgv, Aaux=Aaux, rowdot=nan(parts + 1, Mr))
            R.gemm_epilogue(A, B, C, Mr, Nc, Mr, tri, epi, alpha=R.EPI_ALPHA, stream_out=so, colact=act, tune=tune, **kw)
            got = C.view
            assert torch.equal(got[:, live], ref["C"][:, live]), what + ": C"
            assert bool(torch.isnan(got[:, ~live]).all()) and C.slack_untouched(), what + ": a skipped block or slack was written"
            if epi == 1:
                for name in ("colsq", "coldot"):
                    part = kw[name]
                    assert torch.equal(part[:, live].sum(0), ref[name][live]), what + ": " + name
                    assert bool(torch.isnan(part[:, ~live]).all()), what + ": partials of a skipped block written"
            if epi == 2:
                rd = kw["rowdot"]
                assert bool(torch.isnan(rd[-1]).all()) and not bool(torch.isnan(rd[:-1]).any()), what + ": row-dot partial rows"
                lv = live.cpu().numpy().astype(np.int64)            # skipped blocks contribute exact zeros
                want = dev(F64(c["Aaux"] @ (c["gmu"] * lv)) * c["rs"])
                assert torch.equal(rd[:-1].sum(0), want), what + ": row dots"


_TILED_KNOBS = [(rows, pair) for rows in (64, 128) for pair in (1, 2)]


@pytest.mark.parametrize("tri", [1, 2], ids=["lowerA", "upperA"])
@pytest.mark.parametrize("Mr", R.EPI_MR)
def test_epilogues_tiled_kernel_exact(Mr, tri):
    """Epilogues 0 / 1 / 2 on the tiled kernel (small_panel_max = 16): tile heights 64 / 128, pairing never / always (Mr = 384,
    640: an odd number of row blocks, the pairing has a leftover block), stream_out, the column-activity patterns; the partial
    rows are summed here -- with exact inputs those sums are exact whatever their number."""
    for (rows, pair), Nc in itertools.product(_TILED_KNOBS, R.EPI_NC_TILED):
        _epilogue_case(Mr, Nc, tri, dict(small_panel_max=16, tile_rows=rows, pair_mode=pair), panel=False,
                       layouts=LAYOUTS if Nc == 128 else LAYOUTS[1:])


@pytest.mark.parametrize("tri", [1, 2], ids=["lowerA", "upperA"])
@pytest.mark.parametrize("Mr", [m for m in R.EPI_MR if m <= 512])
def test_epilogues_panel_kernel_exact(Mr, tri):
    """The same on the whole-block panel kernel (defaults; Mr = Kd <= 512), also at widths that are no multiple of 128."""
    for Nc in R.EPI_NC_PANEL:
        _epilogue_case(Mr, Nc, tri, {}, panel=True, layouts=LAYOUTS if Nc <= 48 else LAYOUTS[1:])


@pytest.mark.parametrize("panel", [True, False], ids=["panel", "tiled"])
def test_epilogues_scaled_and_contract(panel):
    """Scaled variant (column scales for the plain store and the column statistics, row scales for the dA epilogue and its
    row dots; 128-blocks >= 2^160 apart) with NaN in the 128-blocks of A that lie wholly in the unused triangle."""
    kws = [{}] if panel else [dict(small_panel_max=16, tile_rows=r, pair_mode=p) for r, p in _TILED_KNOBS]
    for kw, tri in itertools.product(kws, (1, 2)):
        _epilogue_case(384, 384, tri, kw, panel=panel, scaled_for={0: "cols", 1: "cols", 2: "rows"}, poison_unused=True,
                       pats=(None, "first"), sos=(0,), layouts=LAYOUTS[1:])


# ---------------------------------------------------------------------------------------------------------- weighted syrk
def _syrk_case(Mr, Kd, tune_kw, pat=None, scaled=False, pad=2, off=2):
    tune = R.make_tuning(**tune_kw)
    nb = Kd // 128
    c = R.syrk_case(Mr, Kd, kact=None if pat is None else R.ACTIVITY[pat](nb), scaled=scaled)
    A = R.Strided(Mr, Kd, pad, off, fill=F64(c["A"]) * c["rs"][:, None])
    H = torch.full((Mr, Mr), R.NAN, dtype=torch.float64, device=DEV)
    act = None if pat is None else torch.tensor(R.ACTIVITY[pat](nb), dtype=torch.int32, device=DEV)
    R.syrk(A, dev(F64(c["w"])), H, Mr, Kd, kact=act, tune=tune)
    want = dev(R.syrk_ref(c))
    what = f"Mr={Mr} Kd={Kd} act={pat} scaled={scaled} {tune_kw}"
    assert torch.equal(H, want), what + ": %d elements differ" % int((H != want).sum())
    assert torch.equal(H, H.T), what
    return H


@pytest.mark.parametrize("path", ["default", "tiled"])
@pytest.mark.parametrize("Mr", R.SYRK_MR)
def test_weighted_syrk_exact(Mr, path):
    """H = A diag(w) A^T bitwise equal to the reference (hence symmetric): the small-operand path (defaults, Mr and Kd <= 384)
    and the k-sliced tiled path (forced by small_gemm_max = 16), every workgroup budget, activity patterns with w zero on
    the inactive blocks."""
    for Kd, wgs in itertools.product(R.SYRK_KD, (0, 16, 4096)):
        kw = dict(syrk_workgroups=wgs, **({} if path == "default" else dict(small_gemm_max=16)))
        for pat in (None, "all", "none", "first", "last"):
            if pat in ("first", "last") and Kd == 128:
                continue
            _syrk_case(Mr, Kd, kw, pat=pat, pad=0 if pat is None else 2, off=0 if pat is None else 2)


@pytest.mark.parametrize("kw", [{}, dict(small_gemm_max=16), dict(small_gemm_max=16, syrk_workgroups=4096)],
                         ids=["small", "tiled", "tiled4096"])
def test_weighted_syrk_scaled_tiles(kw):
    """Rows of A times 2^e per 128-block: the tiles of H are 2^160 apart or more."""
    for Kd in (256, 2176):
        _syrk_case(384, Kd, kw, scaled=True)


# --------------------------------------------------------------------------------------------------------- knob invariance
def test_knob_invariance_gemm():
    """One shape, every legal combination of the kernel-selection knobs of mobocmf_gemm_f64: bitwise equal to each other."""
    Mr = Nc = Kd = 384
    Ai, Bi = R.gemm_operands(Mr, Nc, Kd, 1)      # dense B: the whole-block panel kernel takes it when the others are off
    A, B = R.Strided(Mr, Kd, 2, 2, fill=F64(Ai)), R.Strided(Kd, Nc, 2, 2, fill=F64(Bi))
    first = None
    for sg, sp, mg, mw in itertools.product((16, 384), (16, 512), (0, 1024), (4, 8, 32)):
        C = R.Strided(Mr, Nc, 2, 2)
        R.gemm(A, B, C, Mr, Nc, Kd, tri=1, tune=R.make_tuning(small_gemm_max=sg, small_panel_max=sp, mid_gemm_max=mg, mid_gemm_waves=mw))
        first = C.view.clone() if first is None else first
        assert torch.equal(C.view, first), (sg, sp, mg, mw)
    assert torch.equal(first, dev(F64(R.fmatmul(Ai, Bi))))


def test_knob_invariance_epilogue():
    Mr, Nc = 384, 384
    outs = {}
    for epi in (1, 2):
        c = R.epilogue_case(Mr, Nc, 1)
        x = R.epilogue_inputs(c)
        for sp, rows, pair in itertools.product((16, 512), (0, 64, 128), (0, 1, 2)):
            tune = R.make_tuning(small_panel_max=sp, tile_rows=rows, pair_mode=pair)
            A, B, C = R.Strided(Mr, Mr, fill=x["A"]), R.Strided(Mr, Nc, fill=x["B"]), R.Strided(Mr, Nc)
            if epi == 1:
                n = R.colstat_rows(1, Mr, Nc, Mr, tune)
                p1, p2 = torch.zeros(n, Nc, dtype=torch.float64, device=DEV), torch.zeros(n, Nc, dtype=torch.float64, device=DEV)
                R.gemm_epilogue(A, B, C, Mr, Nc, Mr, 1, 1, alpha=R.EPI_ALPHA, colsq=p1, coldot=p2, avec=dev(x["avec"]), tune=tune)
                res = (C.view.clone(), p1.sum(0), p2.sum(0))
            else:
                rd = torch.zeros(Nc // 16, Mr, dtype=torch.float64, device=DEV)
                R.gemm_epilogue(A, B, C, Mr, Nc, Mr, 1, 2, alpha=R.EPI_ALPHA, avec=dev(x["avec"]), bscale=dev(x["bscale"]),
                                gmu=dev(x["gmu"]), cgv=dev(x["cgv"]), Aaux=R.Strided(Mr, Nc, fill=x["Aaux"]), rowdot=rd, tune=tune)
                res = (C.view.clone(), rd.sum(0))
            ref = outs.setdefault(epi, res)
            assert all(torch.equal(a, b) for a, b in zip(res, ref)), (epi, sp, rows, pair)


def test_knob_invariance_syrk():
    first = None
    for sg, wgs in itertools.product((16, 384), (0, 16, 64, 512, 4096)):
        H = _syrk_case(384, 1024, dict(small_gemm_max=sg, syrk_workgroups=wgs), pat="last")
        first = H if first is None else first
        assert torch.equal(H, first), (sg, wgs)
