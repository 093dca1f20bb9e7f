"""The frozen-chain predict kernels (csrc/frozen_predict.hip: mobocmf_frozen_predict on 16-column panels, M <= 512, and
mobocmf_frozen_predict_split on 8-column panels, M <= 1024) against a longdouble restatement ON THE GIVEN CHAIN STATE.

The kernels are handed every layer's L^-1, L^-T, U, U^T and a as DATA.  A reference that forms its own factors carries
cond(K_mm) u on both sides, and the composed shadow of the whole model (kernel_reference.model_ref) grows with M through the
comparison inverse of |L|: at 128 < M <= 1024 its gate admits anything.  Conditioned on the factors the kernel actually reads
-- as mes_reference.exact_predict_ref treats mobocmf_exact_predict -- both problems go: per column

    K = k(Z~, [x, f])   A = L^-1 K   C = U^T A   mean = a^T A   var = max(k_nn - |A|^2 + |C|^2, 1e-10)   f' = mean + sqrt(var) eps
    gv = g_var [raw > 1e-10]   dA = 2 U (C gv) + a g_mean - 2 A gv   dK = L^-T dA   the Gram backward w.r.t. x and f (d k_nn / d f
    included), the propagation backward,

are four products with an M x M constant per layer.  The statements and their shadow are kernel_reference's own (_chain_forward
/ _chain_backward behind _layer_forward / _layer_backward, the Gram statements _gram / _gram_bwd, and the model's composition
_model_forward / _model_run with ``chains``): absolute values through every sum and product, the shadow of f carried into the
next layer, and ZERO shadow on the factors and on the packed hyper-parameters, which are data.  What a layer inherits -- the
error of f from below, of the upstream gradients from above -- reaches its outputs through the layer's SIGNED derivatives
instead of through the magnitudes a second time, and S(|A|^2) is 2 |A| S(A) (kernel_reference, above _chain_forward: the
over-counts removed, and why).  The gate is |got - ref| <= C_g u S per component, exact zeros where S = 0, in two groups:
'forward' (top_mean, top_var) and 'gram' (g_x).

C_g is not fitted to the device: tests/test_frozen_predict_reference_cpu.py measures the float64 run of the same restatement
against the longdouble one on every case below, on chains formed on the host, and FROZEN_C = 4 x the recorded figure (the rule
of LAYER_C / MODEL_C: reciprocal lengthscales, fusing, another summation order)."""
import ctypes

import numpy as np

from tests import kernel_reference as R

FROZEN_GROUPS = {"forward": ("top_mean", "top_var"), "gram": ("g_x",)}
# Measured by tests/test_frozen_predict_reference_cpu.py over every case below (worst err / (u S) of the float64 run, chains
# formed on the host), recorded a quarter above the measurement:
#   forward 2.39 (M16_L2_d8_S2_T9; 0.4 .. 1.9 on the other well-conditioned cases, 0.10 on the uniform-Z_x family)
#   gram    1.95 (floor_M130_L1_d8_T3; 1.70 at M = 1, 0.3 .. 0.75 on the other one-layer cases)
# What the gate can see is S / |value| (printed per case by that test).  The moments: medians of 1 .. 80 on the lattice and d = 8
# cases up to M = 1024, 6e3 .. 7e3 at cond 6e4 (M200_L1_d4), 4e8 .. 1e9 on the uniform-Z_x family -- cond(K_mm) itself.  g_x: 1 ..
# 90 at L = 1 and 1e1 .. 5e2 at L >= 2 up to M = 257, 1e4 at M = 512, 3e4 at M = 1024 on the well-conditioned chains; 8e6 at cond
# 6e4 and 1e16 at cond 1e8: the backward passes the rounding of A through |U|, |U^T| and |L^-T| in turn, each taking the
# cancellation of its product once more, and that IS the worst case of these four products in float64.  On the uniform-Z_x
# family the gate on g_x is therefore a bound on magnitudes only (the float64 run sits below 1e-2 of it); what holds g_x there
# are the exact zeros, the repeated bits, the equality with the single-model launch -- and the same code path gated at the
# sizes where S is tight.
FROZEN_RATIO_MEASURED = {"forward": 3.0, "gram": 2.45}
FROZEN_C = {k: 4.0 * v for k, v in FROZEN_RATIO_MEASURED.items()}
FROZEN_NAMES = {"forward": ("top_mean", "top_var"), "input": ("top_mean", "top_var", "g_x")}
# what the CPU test plants in the float64 run, one at a time; the gate must report each on at least one case
FROZEN_DEFECTS = ("last_row_out_of_q", "eps_replica_shifted", "A_gv_dropped", "dknn_df_dropped", "floor_gate_ignored",
                  "UT_entry_off", "stale_pad_rows")
MAX_XDIV = 48                             # MOBOCMF_MAX_XDIV
FORWARD, INPUT_GRADIENTS = R.STEP_FORWARD, R.STEP_INPUT_GRADIENTS
# chains of the CPU test: longdouble Cholesky, tri_inverse_hp and matmul_hp up to this M, the same statements in float64
# beyond it (the row loops in longdouble take minutes at M = 512 .. 1024).  Which factors the reference is handed does not
# enter what is measured: they are exact data on both sides.
HOST_CHAIN_HP_MAX_M = 257


def _fc(L, d, M, T, S=1, **kw):
    return dict(L=L, d=d, M=M, rows=(T,) * L, S=S, predict=True, seeds="both", **kw)


# The smallest cases on each side of a switch in the kernel (frozen_geometry restates the switches; the GPU file asserts them).
FROZEN_PANEL_CASES = {
    "M1_L1_d1_T1": _fc(1, 1, 1, 1),                                   # the smallest problem
    "M16_L2_d8_S2_T9": _fc(2, 8, 16, 9, 2),                           # eight base rows per workgroup; a second workgroup with one row
    "M17_L2_d3_S3_T6": _fc(2, 3, 17, 6, 3),                           # Mr = 32; five rows x 3 = 15 columns, one dead column in the block
    "M200_L1_d4_T33": _fc(1, 4, 200, 33),                             # L = 1: sixteen rows per workgroup, the last workgroup with one
    "M129_L2_d2_S5_T7_uniform": _fc(2, 2, 129, 7, 5, zx="uniform"),   # nine row tiles: the reversed second round holds one; pad rows 129 .. 143
    "M130_L3_d2_S17_T3": _fc(3, 2, 130, 3, 17),                       # S > 16: one base row per workgroup, two column blocks per layer >= 1
    "M257_L2_d8_S16_T2": _fc(2, 8, 257, 2, 16),                       # seventeen tiles: three rounds; exactly one block
    "M512_L2_d8_S48_T2": _fc(2, 8, 512, 2, MAX_XDIV),                 # the LDS limit; three column blocks
    "floor_M130_L1_d8_T3": _fc(1, 8, 130, 3, floor=True),             # the top layer's last column on the variance floor
}
FROZEN_SPLIT_CASES = {
    "M16_L1_d2_T9": _fc(1, 2, 16, 9),                                 # eight base rows per workgroup plus one
    "M65_L3_d8_S8_T2": _fc(3, 8, 65, 2, 8),                           # one full part
    "M129_L2_d2_S11_T3_uniform": _fc(2, 2, 129, 3, 11, zx="uniform"),  # parts of 8 + 3
    "M1024_L2_d8_S9_T2": _fc(2, 8, 1024, 2, 9),                       # the 136 KB LDS limit; parts of 8 + 1
    "floor_M130_L1_d8_T3": _fc(1, 8, 130, 3, floor=True),             # the top layer's last column on the floor
    "floor_M130_L2_d8_S9_T3": _fc(2, 8, 130, 3, 9, floor=True),       # layer 0's last column on the floor, formed by both parts
}
# one launch of several models: (M, L, S) differ, d = 2 and T = 6 and x are shared (x: the first model's)
FROZEN_GROUP_CASES = (_fc(2, 2, 17, 6, 3), _fc(1, 2, 129, 6), _fc(3, 2, 257, 6, 2))


def frozen_case(kw, x=None):
    """model_case(**kw) with seed_scale = 1 (the kernels take the seeds as they are); ``x``: with those test points instead
    of its own (the models of one launch share x)."""
    mc = R.model_case(**kw)
    mc = dict(mc, seed_scale=1.0, key=mc["key"] + ("frozen",))
    if x is None:
        return mc
    assert x.shape == mc["x"].shape
    return dict(mc, x=x, key=mc["key"] + ("shared x",))


def frozen_group_cases():
    first = frozen_case(FROZEN_GROUP_CASES[0])
    return [first] + [frozen_case(kw, first["x"]) for kw in FROZEN_GROUP_CASES[1:]]


def all_frozen_cases():
    """{name: case} of everything the GPU file runs."""
    out = {n: frozen_case(kw) for n, kw in list(FROZEN_PANEL_CASES.items()) + list(FROZEN_SPLIT_CASES.items())}
    out.update({"group_M%d_L%d" % (mc["M"], mc["L"]): mc for mc in frozen_group_cases()})
    return out


def frozen_geometry(mc, split):
    """The launch geometry restated from csrc/frozen_predict.hip.  16-column form: base rows per workgroup (frozen_rows_per_wg),
    workgroups, base rows of the last one, 16-row tiles of M, rounds of tile_of_wave over the 8 wavefronts, tiles of the last
    round, column blocks of a workgroup's widest layer and the dead columns of its last block.  Split form: rows per workgroup
    (8 at L = 1, else 1), parts (ceil(S / 8)), replicas of the last part, workgroups, tiles, dynamic LDS bytes."""
    L, M, T, S = mc["L"], mc["M"], mc["rows"][0], (mc["S"] if mc["L"] > 1 else 1)
    tiles = -(-M // 16)
    if split:
        parts = 1 if L == 1 else -(-S // 8)
        return dict(rows=8 if L == 1 else 1, parts=parts, last_part=S - 8 * (parts - 1), wgs=-(-T // 8) if L == 1 else T * parts,
                    tiles=tiles, lds=17 * 16 * tiles * 8)
    rb = 16 if L == 1 else (1 if S >= 16 else 16 // S)
    wgs = -(-T // rb)
    cols = min(rb, T) * S
    return dict(rows=rb, wgs=wgs, last_rows=T - rb * (wgs - 1), tiles=tiles, rounds=-(-tiles // 8), last_round=tiles - 8 * ((tiles - 1) // 8),
                blocks=-(-cols // 16), dead=-cols % 16, lds=33 * 16 * tiles * 8)


def host_layers(mc):
    """The layers of ``mc`` as the chain forward and the kernels are handed them: float64, hyp = softplus(raw) rounded."""
    return [R.model_layer(mc, l, R._f64) for l in range(mc["L"])]


def host_chains(mc):
    """Every layer's chain state formed on the host and rounded to float64: {Linv, LinvT, U, UT, a, hyp}.  Up to
    HOST_CHAIN_HP_MAX_M in longdouble (the column Cholesky, tri_inverse_hp, matmul_hp), beyond it the same statements in
    float64."""
    out = []
    hp = mc["M"] <= HOST_CHAIN_HP_MAX_M and R.HAVE_LONGDOUBLE
    T = R.ld if hp else R._f64
    for lc in host_layers(mc):
        M = lc["M"]
        Kmm = R._gram(lc["kind"], R._gram_operands(lc)[0], 1, T)[0] + T(lc["jitter"]) * np.eye(M, dtype=T(0.0).dtype)
        L = R._chol_columns(Kmm)
        Linv = R.tri_inverse_hp(L) if hp else R._tri_inverse(L)
        mm = R.matmul_hp if hp else (lambda a, b: a @ b)
        Linv = R._f64(Linv)
        U, a = R._f64(mm(Linv, np.tril(lc["L_S"]))), R._f64(mm(Linv, lc["m"][:, None]))[:, 0]
        out.append(dict(Linv=Linv, LinvT=Linv.T.copy(), U=U, UT=U.T.copy(), a=a, hyp=lc["hyp"]))
    return out


def chain_state_views(block, M):
    """Named float64 host copies {Linv, LinvT, U, UT, a} [M x M, M] of one layer's CHAIN state, read back from the device byte
    tensor ``block`` and carved in the order common.h documents (FCS_*): [L | L^-1 | L^-T | U | U^T | L_S | a | m], each Mp x
    Mp with Mp = M rounded up to 128, then the Mp-vectors.  "padded": the same five at their full Mp extent."""
    Mp = -(-M // 128) * 128
    mm = Mp * Mp
    assert block.numel() >= (6 * mm + 2 * Mp) * 8
    w = block[:(6 * mm + 2 * Mp) * 8].view(R.torch.float64).cpu().numpy()
    full = {k: w[i * mm:(i + 1) * mm].reshape(Mp, Mp) for k, i in (("Linv", 1), ("LinvT", 2), ("U", 3), ("UT", 4))}
    full["a"] = w[6 * mm:6 * mm + Mp]
    out = {k: (v[:M, :M] if v.ndim == 2 else v[:M]).copy() for k, v in full.items()}
    out["padded"] = full
    return out


_ref_cache = {}


def frozen_predict_ref(mc, chains, shadow=False, dtype=np.longdouble):
    """{top_mean, top_var [T S; T at L = 1], g_x [T x d]} of the case ``mc`` on the GIVEN ``chains`` (one dict per layer:
    chain_state_views' or host_chains' fields and "hyp") in ``dtype`` -- or, ``shadow``, the composed componentwise shadow S of
    each.  The longdouble run asserts that every column's floor decision in every layer is robust: |raw - 1e-10| exceeds the
    column's own gate FROZEN_C['forward'] u S(raw) -- a condition on the inputs.  Cached per case and chain object."""
    assert dtype is not np.longdouble or R.HAVE_LONGDOUBLE
    key = (mc["key"], mc.get("defect"), id(chains), np.dtype(dtype).name)
    if key not in _ref_cache:
        res, sha, fw = R._model_run(mc, lambda a: np.asarray(a, dtype), chains=chains)
        if dtype is np.longdouble:
            for l, (lc, st, sst) in enumerate(fw):
                margin = np.abs(st["varraw"] - R.ld(lc["min_var"]))
                assert np.all(margin > FROZEN_C["forward"] * R.ld(R.U) * sst["varraw"]), (mc["key"], l)
        pick = lambda r: {k: r[k] for k in FROZEN_NAMES["input"]}
        _ref_cache[key] = (pick(res), pick(sha), chains)                   # (the chains stay alive with their id)
    return _ref_cache[key][1 if shadow else 0]


def floored_columns(mc, chains):
    """Per layer the columns on the variance floor (from the longdouble run)."""
    fw = R._model_forward(mc, R.ld, chains=chains)
    return [np.flatnonzero(st["varraw"] <= R.ld(lc["min_var"])) for lc, st, _ in fw]


def frozen_gate(got, ref, S, names):
    """(violations [(name, ratio, non-zeros where S = 0)], {group: worst ratio}, report) of |got - ref| <= FROZEN_C u S."""
    rat = R.layer_ratios(got, ref, S, names)
    worst, bad = {}, []
    for k, (r, nz) in rat.items():
        g = next(g_ for g_, ns in FROZEN_GROUPS.items() if k in ns)
        worst[g] = max(worst.get(g, 0.0), r)
        if not r <= FROZEN_C[g] or nz:
            bad.append((k, r, nz))
    report = "  ".join("%s %.2f u S = %.0f%% of the gate" % (g, w, 100 * w / FROZEN_C[g]) for g, w in worst.items())
    return bad, worst, report


def with_defect(mc, chains, defect):
    """(case, chains) of the float64 run with one of FROZEN_DEFECTS planted.  Two of them are changes of the run's inputs:
    'eps_replica_shifted' -- in the second 16-column block of a base row (replicas 16 ..; S > 16) layer 1 draws the NEXT
    replica's sample; 'UT_entry_off' -- one entry of the U^T array (not of U) of the top layer is scaled by 1 + 2^-30.  The
    others are read by _layer_forward / _layer_backward."""
    assert defect in FROZEN_DEFECTS
    mc = dict(mc, key=mc["key"] + ("defect", defect))
    if defect == "eps_replica_shifted":
        S, N = mc["S"], mc["rows"][1] if mc["L"] > 1 else 0
        if mc["L"] == 1 or S <= 16:
            return mc, chains
        s = np.arange(S)
        e = mc["samples"][1][np.where(s >= 16, (s + 1) % S, s)]
        return dict(mc, eps=[None, np.tile(e, N)] + list(mc["eps"][2:])), chains
    if defect == "UT_entry_off":
        top = dict(chains[-1])
        UT = top["UT"].copy()
        i = mc["M"] // 2
        UT[i // 2, i] *= 1 + 2.0 ** -30                                    # (U^T is upper triangular: row <= column)
        top["UT"] = UT
        return mc, list(chains[:-1]) + [top]
    return dict(mc, defect=defect), chains


# ---- the direct caller: descriptors through the ctypes definition of _lib, the table uploaded as bytes, NaN-filled outputs
# with GUARD doubles behind each, the chains from mobocmf_layers_chain_forward (branch = 1) into its NaN-prefilled blocks
class FrozenLaunch:
    """The models ``mcs`` (they share T, d and x) set up for mobocmf_frozen_predict (``split`` False) or
    mobocmf_frozen_predict_split: ``chain_calls[i]`` (kernel_reference.chain_forward_direct of the model's layers),
    ``chains[i]`` (per layer chain_state_views and "hyp"), the outputs, `work` of exactly the bytes the size query reports."""

    def __init__(self, mcs, split):
        from mobocmf_amd import _lib
        torch = R.torch
        self.mcs, self.split, self.n = list(mcs), split, len(mcs)
        self.entry = "mobocmf_frozen_predict_split" if split else "mobocmf_frozen_predict"
        self.host = (_lib.FrozenPredictModel * self.n)()
        self.T, self.d = mcs[0]["rows"][0], mcs[0]["d"]
        self.x = R._dev(mcs[0]["x"])
        self.chain_calls, self.chains, self.keep, self.outs, self.lens = [], [], [], [], []
        for i, mc in enumerate(self.mcs):
            assert mc["rows"][0] == self.T and mc["d"] == self.d and np.array_equal(mc["x"], mcs[0]["x"])
            L, M, S = mc["L"], mc["M"], (mc["S"] if mc["L"] > 1 else 1)
            layers = host_layers(mc)
            ch = R.chain_forward_direct(layers)
            assert ch.rc == 0 and ch.info == [0] * L and ch.untouched, (ch.rc, ch.info)
            self.chain_calls.append(ch)
            self.chains.append([dict(chain_state_views(R.chain_block(ch, l, True), M), hyp=layers[l]["hyp"]) for l in range(L)])
            rec = self.host[i]
            rec.L, rec.M, rec.d, rec.S, rec.T = L, M, self.d, S, self.T
            t = {"gm": R._dev(mc["seed_gmean"]), "gv": R._dev(mc["seed_gvar"])}
            for l in range(_lib.TINY_MAX_LAYERS):
                on = l < L
                rec.kind[l] = int(on and l > 0)
                rec.chain[l] = R.chain_block(ch, l).data_ptr() if on else None
                rec.Zx[l], rec.hyp[l] = (ch.inp[l]["Zx"].data_ptr(), ch.inp[l]["hyp"].data_ptr()) if on else (None, None)
                if on and l:
                    t["samples%d" % l] = R._dev(mc["samples"][l])
                rec.zf[l] = ch.inp[l]["zf"].data_ptr() if on and l else None
                rec.samples[l] = t["samples%d" % l].data_ptr() if on and l else None
            nt = self.T * S
            wb = ctypes.c_size_t(7)
            assert getattr(R.lib(), self.entry + "_work_bytes")(ctypes.byref(rec), INPUT_GRADIENTS, ctypes.byref(wb)) == 0
            assert wb.value == (8 * -(-S // 8) * self.T * self.d if split and L > 1 else 0)
            lens = dict(top_mean=nt, top_var=nt, grad=self.T * self.d, work=wb.value // 8)
            o = {k: R._out(n) for k, n in lens.items()}
            rec.x, rec.top_mean, rec.top_var, rec.grad = self.x.data_ptr(), o["top_mean"].data_ptr(), o["top_var"].data_ptr(), o["grad"].data_ptr()
            rec.seed_gmean, rec.seed_gvar = t["gm"].data_ptr(), t["gv"].data_ptr()
            rec.work = o["work"].data_ptr() if wb.value else None
            self.keep.append(t)
            self.outs.append(o)
            self.lens.append(lens)
        self.table = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()

    def poison(self):
        for o in self.outs:
            for v in o.values():
                v.fill_(R.NAN)

    def run(self, mode):
        """Poisons every output and `work`, launches, synchronises.  ``res[i]`` {top_mean, top_var, g_x} as numpy (NaN where
        nothing was written), ``guards[i]``: every guard double -- behind `work` too -- still NaN; ``grad_untouched[i]``."""
        torch = R.torch
        self.poison()
        torch.cuda.synchronize()
        self.rc = getattr(R.lib(), self.entry)(ctypes.cast(self.host, ctypes.c_void_p), R._p(self.table), self.n, mode, R._stream())
        torch.cuda.synchronize()
        self.res, self.guards, self.grad_untouched = [], [], []
        for mc, o, lens in zip(self.mcs, self.outs, self.lens):
            self.guards.append(all(bool(torch.isnan(o[k][n:]).all()) for k, n in lens.items()))
            self.grad_untouched.append(bool(torch.isnan(o["grad"]).all()) and bool(torch.isnan(o["work"]).all()))
            self.res.append(dict(top_mean=o["top_mean"][:lens["top_mean"]].cpu().numpy(), top_var=o["top_var"][:lens["top_var"]].cpu().numpy(),
                                 g_x=o["grad"][:lens["grad"]].cpu().numpy().reshape(self.T, self.d)))
        return self
