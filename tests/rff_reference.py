"""The random-Fourier-feature sample kernels (csrc/rff.hip: mobocmf_rff_eval, mobocmf_rff_eval_chains; csrc/rff_opt.hip:
mobocmf_rff_chains_value_grad, mobocmf_rff_refine) against a longdouble restatement ON THE GIVEN DRAWS.

The kernels are handed W1, b1, theta, Wf, W2, b2 and three scales per layer as DATA: they carry zero shadow, no model is
fitted, and a case is a seeded numpy draw packed into one ``params`` buffer (a NaN word in front of every operand and behind
the last: a read one past an operand shows as NaN) with a ``layers`` table of the form functional.rff_eval_chains takes.  The
builder is this module's own -- layers of one chain and chains of one launch may have different F, which RFFChainSample.pack
does not allow.  Per layer (the header of rff.hip; the forward-mode recursion of rff_opt.hip)

    kind 0   f = s0 sum_j theta_j cos(a_j),                                           a_j = b1_j + W1_j . x
    kind 1   f = sum_j theta_j s0 f' cos(a_j) + theta_{F+j} s1 cos(a_j + Wf_j f') + theta_{2F+j} s2 cos(b2_j + W2_j . x)
             D = d f / d f' = sum_j theta_j s0 cos(a_j) - theta_{F+j} s1 Wf_j sin(a_j + Wf_j f')
             g = px + D g',   px = the partial derivative w.r.t. x at fixed f'

and the componentwise shadow S of each under kernel_reference's rules: absolute values through every sum and product; an
argument's shadow |b| + sum_k |w_k x_k| (+ |Wf f'|) reaches cos and sin through the signed derivative, S(cos a) = |sin a| S(a) +
|cos a| (one rounding of the function itself); the shadow of f' from the layer below reaches f, D and px through |D|, |dD / df'|
and |dpx / df'| -- not through the magnitudes a second time -- and S(g) = S(px) + S(D) |g'| + |D| S(g').  The gate is
|got - ref| <= RFF_C u S per component, exact zeros where S = 0, in the groups 'value' and 'grad'.

The refinement is gated through its ONE-STEP model (rff_refine_step_ref): outer = inner = 1, backtracks = restore = 0 and a
given step0 / rho0, where what mobocmf_rff_refine writes is a closed form as long as every decision on the way is robust.

RFF_C is not fitted to the device: tests/test_rff_reference_cpu.py measures a float64 restatement in the kernels' summation
orders (``order``: 'eval' -- one thread per point, the features in order; 'vg' / 'refine' -- lane-strided partial sums, the
xor butterfly, the wavefronts' sums in order) against the longdouble one on every case below."""
import ctypes

import numpy as np

from tests import kernel_reference as R

RFF_T, RFF_FC = 256, 64                   # rff.hip: grid points per workgroup, features per LDS chunk
RO_WAVE, RO_VG_WAVES = 64, 4              # rff_opt.hip: lanes, points per workgroup of the value-and-gradient kernel
MAX_LAYERS, MAX_CON = 3, 32               # MOBOCMF_RFF_MAX_LAYERS, MOBOCMF_REFINE_MAX_CON
ARMIJO = 1e-4                             # the library's default, left as it is
RFF_GROUPS = ("value", "grad")
# Measured by tests/test_rff_reference_cpu.py (worst err / (u S) of the float64 run in the kernels' summation orders over every
# case below, the kind 1 layers on a given fprev and the one-step model's merit gradient, fs and slack_min included), recorded
# a quarter above the measurement:
#   value  1.11 (kind 1 at F = 1 on a given fprev, EVAL1 F1_d3, 257 points; 0.94 at F = 1 in the refinement's order, 0.54 at
#          F = 1 in a wavefront's; 0.13 .. 0.35 on the eval cases at F >= 63, 0.03 .. 0.14 in the lane-strided orders)
#   grad   0.47 (value_grad d2_F1_n5_L2; 0.43 and 0.26 on the other F = 1 cases, 0.03 .. 0.25 at F >= 63; the merit gradient of
#          the one-step model 0.01 .. 0.26)
# A single feature has nothing to average over: its few roundings are the whole error and the whole shadow, which is why the
# F = 1 cases set both figures.  What the gate can see is the median S / |value| (printed per case by that test): 2 .. 35 at
# F = 1; 60 .. 900 for values and 160 .. 1400 for gradients at F >= 63 and lengthscale 1/3 (the F terms do cancel: |f| ~ sqrt(F)
# of sum |term|, and the argument's shadow |b| + sum |w x| of 5 .. 50 multiplies every term); 1.4e4 .. 2.8e4 at |W . x| ~ 1e3;
# 6e6 on the cancelling theta -- there the gate bounds the error by 6e6 u |f| = 7e-10 |f|, which IS the accuracy float64 has for
# such a sum, where the normwise 1e-11 max |f| of the older tests admits anything at a component 1e-6 of the largest.
RFF_RATIO_MEASURED = {"value": 1.39, "grad": 0.59}
RFF_C = {k: 4.0 * v for k, v in RFF_RATIO_MEASURED.items()}
# what the CPU test plants in the float64 run, one at a time; the gate must report each on at least one case
RFF_DEFECTS = ("last_chunk_dropped", "theta1_shifted", "b2_as_b1", "s0_twice", "D_dropped", "wf_dropped_from_D",
               "wave_value_dropped", "wave_grad_dropped", "merit_sign_flipped")


# ------------------------------------------------------------------------------------------------------------------ cases
def _pack(ops):
    """(params, layers): every operand of ``ops`` [chain][layer] in one float64 buffer, a NaN word in front of each and one at
    the end; the table functional.rff_eval_chains takes."""
    parts, layers, pos = [], [], 0
    for chain in ops:
        tab = []
        for op in chain:
            e = dict(kind=op["kind"], F=op["F"], s0=op["s0"], s1=op["s1"], s2=op["s2"])
            for name in ("W1", "b1", "theta") + (("Wf", "W2", "b2") if op["kind"] else ()):
                a = np.ascontiguousarray(op[name], np.float64).reshape(-1)
                parts += [np.array([np.nan]), a]
                e[name] = pos + 1
                pos += 1 + a.size
            tab.append(e)
        layers.append(tab)
    parts.append(np.array([np.nan]))
    return np.concatenate(parts), layers


def rff_case(name, d, chains, n, seed, wscale=3.0, cancel=False):
    """A launch of len(chains) chain samples at n points of [0, 1]^d: ``chains[k]`` = the F of every layer of chain k.  Rows of
    W1, W2 are standard normal times ``wscale`` (the reciprocal lengthscale), phases uniform in [0, 2 pi), theta standard
    normal, Wf 1.5 x standard normal, the scales sqrt(2 amplitude / F).  ``cancel``: theta of chain 0's layer 0 is a draw of
    scale 1e3 corrected (least squares on the n < F points) so that f = 1e-6 sum |theta cos| at every point -- posterior
    weights under a small noise look like that."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    ops = []
    for Fs in chains:
        assert 1 <= len(Fs) <= MAX_LAYERS
        chain = []
        for l, F in enumerate(Fs):
            amp = lambda: np.sqrt(2.0 * (0.5 + rng.random()) / F)
            op = dict(kind=int(l > 0), F=F, W1=wscale * rng.standard_normal((F, d)), b1=rng.uniform(0, 2 * np.pi, F),
                      theta=rng.standard_normal(3 * F if l else F), s0=amp(), s1=0.0, s2=0.0)
            if l:
                op.update(Wf=1.5 * rng.standard_normal(F), W2=wscale * rng.standard_normal((F, d)),
                          b2=rng.uniform(0, 2 * np.pi, F), s1=amp(), s2=amp())
            chain.append(op)
        ops.append(chain)
    if cancel:
        op = ops[0][0]
        assert n < op["F"]
        Phi = np.cos(x @ op["W1"].T + op["b1"][None, :])
        th = 1e3 * op["theta"]
        target = 1e-6 * (np.abs(th)[None, :] * np.abs(Phi)).sum(1) * np.where(np.arange(n) % 2, -1.0, 1.0)
        op["theta"] = th - np.linalg.lstsq(Phi, Phi @ th - target, rcond=None)[0]
    params, layers = _pack(ops)
    for a in [x, params] + [v for ch in ops for op in ch for v in op.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return dict(name=name, d=d, n=n, K=len(chains), chains=tuple(tuple(c) for c in chains), x=x, ops=ops, params=params,
                layers=layers)


MIXED = ((65,), (64, 1, 129), (63, 65))                     # depths 1, 3, 2; the layers of a chain differ in F
# the smallest shapes on each side of each switch (rff_geometry restates the switches; the GPU file asserts the sides)
EVAL_CASES = {
    "d1_F1_n1_L1": dict(d=1, chains=((1,),), n=1),
    "d2_F63_n255_L2": dict(d=2, chains=((63, 63),), n=255),
    "d3_F64_n256_L3": dict(d=3, chains=((64, 64, 64),), n=256),
    "d8_F65_n257_L2": dict(d=8, chains=((65, 65),), n=257),
    "d9_F129_n257_L1": dict(d=9, chains=((129,),), n=257),
    "d32_F64_n1_L3": dict(d=32, chains=((64, 64, 64),), n=1),
    "d32_F65_n256_L2": dict(d=32, chains=((65, 65),), n=256),
    "d2_F129_n257_L3": dict(d=2, chains=((129, 129, 129),), n=257),
    "mixed_d3_K3_n257": dict(d=3, chains=MIXED, n=257),
    "short_d2_F65_n257_L2": dict(d=2, chains=((65, 65),), n=257, wscale=1e3),
    "cancel_d3_F65_n5_L1": dict(d=3, chains=((65,),), n=5, cancel=True),
}
# kind 1 through mobocmf_rff_eval with a GIVEN fprev: (case of EVAL_CASES, chain, layer) at F = 1, 63, 64, 65, 129
EVAL1_CASES = {"F1_d3": ("mixed_d3_K3_n257", 1, 1), "F63_d2": ("d2_F63_n255_L2", 0, 1), "F64_d3": ("d3_F64_n256_L3", 0, 2),
               "F65_d32": ("d32_F65_n256_L2", 0, 1), "F129_d2": ("d2_F129_n257_L3", 0, 1)}
VG_CASES = {
    "d1_F1_n1_L1": dict(d=1, chains=((1,),), n=1),
    "d2_F1_n5_L2": dict(d=2, chains=((1, 1),), n=5),
    "d2_F63_n3_L2": dict(d=2, chains=((63, 63),), n=3),
    "d3_F64_n4_L2": dict(d=3, chains=((64, 64),), n=4),
    "d8_F65_n5_L2": dict(d=8, chains=((65, 65),), n=5),
    "d9_F65_n5_L3": dict(d=9, chains=((65, 65, 65),), n=5),
    "d32_F63_n3_L2": dict(d=32, chains=((63, 63),), n=3),
    "mixed_d3_K3_n5": dict(d=3, chains=MIXED, n=5),
    "short_d2_F65_n5_L2": dict(d=2, chains=((65, 65),), n=5, wscale=1e3),
    "cancel_d3_F65_n5_L1": dict(d=3, chains=((65,),), n=5, cancel=True),
}
_cases = {}


def _seed(group, name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(group + name))


def eval_case(name):
    if ("eval", name) not in _cases:
        _cases["eval", name] = rff_case("eval " + name, seed=_seed("eval", name), **EVAL_CASES[name])
    return _cases["eval", name]


def vg_case(name):
    if ("vg", name) not in _cases:
        _cases["vg", name] = rff_case("vg " + name, seed=_seed("vg", name), **VG_CASES[name])
    return _cases["vg", name]


def eval1_case(name):
    """(case, chain, layer, fprev [n]): the layer evaluated by itself on a standard normal fprev, which is data."""
    cname, k, l = EVAL1_CASES[name]
    c = eval_case(cname)
    return c, k, l, np.random.default_rng(_seed("eval1", name)).standard_normal(c["n"])


def single_chain(case, k):
    """Chain k of the launch by itself: the same params buffer and offsets."""
    return dict(case, name=case["name"] + " chain %d" % k, K=1, chains=(case["chains"][k],), ops=[case["ops"][k]],
                layers=[case["layers"][k]])


# ---- the one-step refinement cases.  P = 2 problems share the chains (problem 0 with every slack >= 0 at every start, problem
# 1 with the slacks of the even constraints < 0), R = 3 starts in [0.25, 0.75]^d; C constraints cycle over the chains 1 .. K - 1
# with their own thresholds.  step0 is small against the curvature (wscale^2, times rho0 sum |grad c|^2 in the merit): the Armijo
# test passes with room, f decreases, and no component leaves (0, 1) -- unless ``clamp``: there start 0 of problem 0 has one
# component at 1e-9 whose gradient component is positive, and the step takes it below 0.
REFINE_CASES = {
    "d1_F1_L1_C0": dict(d=1, chains=((1,),), C=0, step0=1e-2),
    "d2_F511_L1_C1": dict(d=2, chains=((511,), (511,)), C=1, step0=1e-2),
    "d8_F512_L3_C2": dict(d=8, chains=((512, 512, 512),) * 3, C=2, step0=2e-4),
    "d3_F513_L3_C32": dict(d=3, chains=((513, 64, 513), (65, 513), (513,)), C=32, step0=2e-4),
    "d9_F255_L1_C1": dict(d=9, chains=((255,), (255,)), C=1, step0=1e-3),
    "d32_F256_L3_C2": dict(d=32, chains=((256, 256, 256),) * 3, C=2, step0=5e-5),
    "d9_F257_L3_C32": dict(d=9, chains=((257, 257, 257), (257,), (64, 257)), C=32, step0=1e-4),
    "d8_F512_L1_C0_clamped": dict(d=8, chains=((512,),), C=0, step0=1e-2, clamp=True),
}
REFINE_R = 3


def refine_case(name):
    if ("refine", name) in _cases:
        return _cases["refine", name]
    kw = dict(REFINE_CASES[name])
    C, step0, clamp = kw.pop("C"), kw.pop("step0"), kw.pop("clamp", False)
    seed = _seed("refine", name)
    c = rff_case("refine " + name, n=1, seed=seed, **kw)
    rng = np.random.default_rng(seed + 1)
    d, K = c["d"], c["K"]
    P = 2 if C else 1
    x0 = rng.uniform(0.25, 0.75, (P, REFINE_R, d))
    cons = [1 + i % (K - 1) for i in range(C)]
    if clamp:
        # the component: the first whose gradient component is positive with that component at 1e-9
        for k in range(d):
            t = x0[0, 0].copy()
            t[k] = 1e-9
            g = rff_chain_ref(c, t[None, :], dtype=np.float64, chains=(0,))["grad"][0, 0]
            if g[k] * step0 > 1e-6:
                x0[0, 0] = t
                c["clamped"] = (0, 0, k)
                break
        assert "clamped" in c, name
    thr = []
    if C:
        # thresholds from the constraints' float64 values at every start of both problems: 0.3 below the smallest (a slack
        # >= 0.3 everywhere) or 0.3 above the largest (<= -0.3 everywhere)
        v = rff_chain_ref(c, x0.reshape(-1, d), dtype=np.float64)["value"]
        lo, hi = v.min(1) - 0.3, v.max(1) + 0.3
        thr = [[lo[ci] - 0.01 * i for i, ci in enumerate(cons)],
               [(hi[ci] + 0.01 * i) if i % 2 == 0 else (lo[ci] - 0.01 * i) for i, ci in enumerate(cons)]]
    c.update(P=P, R=REFINE_R, C=C, x0=x0, step0=step0, rho0=1.0, obj=[0] * P, cons=[cons] * P, thr=thr,
             nw=8 if d <= 8 else 4)
    x0.setflags(write=False)
    _cases["refine", name] = c
    return c


def rff_geometry(case):
    """The switches of the kernels restated.  All: the DB instantiation and its dead columns.  eval / chains: LDS chunks and the
    size of the last one per chain and layer, workgroups (per chain) and the live rows of the last.  value_grad: workgroups,
    points in the last one, lanes without a feature per chain and layer.  refine: NW, features per thread and idle wavefronts
    per chain and layer."""
    d, n = case["d"], case["n"]
    DB = 2 if d <= 2 else (8 if d <= 8 else 32)
    nw = 8 if d <= 8 else 4
    per = lambda f: [[f(F) for F in Fs] for Fs in case["chains"]]
    return dict(DB=DB, dead=DB - d,
                chunks=per(lambda F: -(-F // RFF_FC)), last_chunk=per(lambda F: F - RFF_FC * ((F - 1) // RFF_FC)),
                wgs=-(-n // RFF_T), last_rows=n - RFF_T * ((n - 1) // RFF_T),
                vg_wgs=-(-n // RO_VG_WAVES), vg_last_points=n - RO_VG_WAVES * ((n - 1) // RO_VG_WAVES),
                vg_idle_lanes=per(lambda F: max(0, RO_WAVE - F)),
                NW=nw, per_thread=per(lambda F: -(-F // (RO_WAVE * nw))), idle_waves=per(lambda F: max(0, nw - -(-F // RO_WAVE))))


# -------------------------------------------------------------------------------------------------------------- the statement
def _partials(terms, order, nw, last_chunk_dropped=False):
    """terms [n x F ...] -> the threads' partial sums [n x T ...]: T = 1 for 'plain' (numpy's sum) and 'eval' (the features in
    order), T = 64 nw for 'vg' / 'refine' (thread t adds the features t, t + T, ... in order)."""
    F = terms.shape[1]
    if order == "plain":
        return terms.sum(1, keepdims=True)
    if order == "eval":
        if last_chunk_dropped:
            terms = terms[:, :RFF_FC * ((F - 1) // RFF_FC)]
            if terms.shape[1] == 0:
                return np.zeros_like(terms.sum(1, keepdims=True))
        return np.cumsum(terms, axis=1)[:, -1:]
    T = RO_WAVE * nw
    rounds = -(-F // T)
    pad = np.zeros((terms.shape[0], rounds * T - F) + terms.shape[2:], terms.dtype)
    t = np.concatenate([terms, pad], 1).reshape((terms.shape[0], rounds, T) + terms.shape[2:])
    acc = t[:, 0]
    for r in range(1, rounds):
        acc = acc + t[:, r]
    return acc


def _across(part, order, nw, drop_wave=None):
    """[n x T ...] -> [n ...]: ro_sum -- the xor butterfly inside each wavefront, then the wavefronts in the order 0, 1, ...
    (``drop_wave``: that wavefront's share left out, a planted defect)."""
    if order in ("plain", "eval"):
        return part[:, 0]
    v = part.reshape((part.shape[0], nw, RO_WAVE) + part.shape[2:])
    lanes = np.arange(RO_WAVE)
    off = RO_WAVE // 2
    while off:
        v = v + v[:, :, lanes ^ off]
        off //= 2
    t = v[:, 0, 0]
    for w in range(1, nw):
        if w != drop_wave:
            t = t + v[:, w, 0]
    return t


def _layer_run(op, x, fp, sfp, pg, g, sg, T, order, nw, defect):
    """One layer in the number format ``T`` converts to.  fp / sfp: the value of the layer below and its shadow [n]; pg: the
    threads' shares of the gradient below [n x T x d], g / sg: that gradient and its shadow [n x d].  Returns (value, D, the
    threads' shares of the gradient, the gradient, S(value), S(D), S(gradient))."""
    F, kind = op["F"], op["kind"]
    W1, b1, th = T(op["W1"]), T(op["b1"]), T(op["theta"])
    s0 = T(op["s0"])
    ab = np.abs
    drop_v = 1 if defect == "wave_value_dropped" else None
    part = lambda t: _partials(t, order, nw, defect == "last_chunk_dropped")
    tot = lambda t: _across(part(t), order, nw, drop_v)

    def arg(W, b):
        a, sa = b[None, :] + 0 * x[:, :1], ab(b)[None, :] + 0 * x[:, :1]
        for k in range(x.shape[1]):
            t = W[None, :, k] * x[:, k:k + 1]
            a, sa = a + t, sa + ab(t)
        return a, sa

    a1, sa1 = arg(W1, b1)
    c1, s1_ = np.cos(a1), np.sin(a1)
    Sc1, Ss1 = ab(s1_) * sa1 + ab(c1), ab(c1) * sa1 + ab(s1_)
    aW1 = ab(W1)[None, :, :]
    if kind == 0:
        val = s0 * tot(th[None, :] * c1)
        if defect == "s0_twice":
            val = s0 * val
        px = s0 * part(-(th[None, :] * s1_)[:, :, None] * W1[None, :, :])
        S_val = ab(s0) * (ab(th)[None, :] * Sc1).sum(1)
        S_g = ab(s0) * ((ab(th)[None, :] * Ss1)[:, :, None] * aW1).sum(1)
        return val, None, px, _across(px, order, nw), S_val, None, S_g
    Wf, W2 = T(op["Wf"]), T(op["W2"])
    b2 = b1 if defect == "b2_as_b1" else T(op["b2"])
    t0, t2 = th[None, :F], th[None, 2 * F:] * T(op["s2"])
    t1 = (np.concatenate([th[F + 1:2 * F], th[2 * F:2 * F + 1]]) if defect == "theta1_shifted" else th[F:2 * F])[None, :] * T(op["s1"])
    wf = Wf[None, :]
    s0fp = (s0 * fp)[:, None]
    af, saf = a1 + wf * fp[:, None], sa1 + ab(wf * fp[:, None])
    a2, sa2 = arg(W2, b2)
    cf, sf, c2, s2_ = np.cos(af), np.sin(af), np.cos(a2), np.sin(a2)
    Scf, Ssf = ab(sf) * saf + ab(cf), ab(cf) * saf + ab(sf)
    Sc2, Ss2 = ab(s2_) * sa2 + ab(c2), ab(c2) * sa2 + ab(s2_)
    val = tot(t0 * s0fp * c1 + t1 * cf + t2 * c2)
    D = tot(t0 * s0 * c1 - (0 if defect == "wf_dropped_from_D" else t1 * wf * sf))
    cx1, cx2 = -(t0 * s0fp * s1_ + t1 * sf), -(t2 * s2_)
    px = part(cx1[:, :, None] * W1[None, :, :] + cx2[:, :, None] * W2[None, :, :])
    Dg = 1 if defect == "D_dropped" else D[:, None, None]
    npg = px + Dg * pg
    # the shadows: this layer's own roundings, then what it inherits through its signed derivatives w.r.t. fp
    dD = (-t1 * wf * wf * cf).sum(1)
    dpx = (-(t0 * s0 * s1_ + t1 * wf * cf)[:, :, None] * W1[None, :, :]).sum(1)
    S_val = (ab(t0 * s0fp) * Sc1 + ab(t1) * Scf + ab(t2) * Sc2).sum(1) + ab(D) * sfp
    S_D = (ab(t0 * s0) * Sc1 + ab(t1 * wf) * Ssf).sum(1) + ab(dD) * sfp
    S_px = ((ab(t0 * s0fp) * Ss1 + ab(t1) * Ssf)[:, :, None] * aW1 + (ab(t2) * Ss2)[:, :, None] * ab(W2)[None, :, :]).sum(1) \
        + ab(dpx) * sfp[:, None]
    S_g = S_px + S_D[:, None] * ab(g) + ab(D)[:, None] * sg
    return val, D, npg, _across(npg, order, nw), S_val, S_D, S_g


def _chain_run(case, k, x, T, order, nw, defect):
    """Per layer of chain k at the rows of x: dict(value, D, grad, S_value, S_D, S_grad); the last entry also holds "pg", the
    threads' shares of the top gradient [n x T x d]."""
    x = T(x)
    out, fp, sfp, pg, g, sg = [], None, None, 0, None, None
    for op in case["ops"][k]:
        val, D, pg, g, S_val, S_D, sg = _layer_run(op, x, fp, sfp, pg, g, sg, T, order, nw, defect)
        fp, sfp = val, S_val
        out.append(dict(value=val, D=D, grad=g, S_value=S_val, S_D=S_D, S_grad=sg))
    out[-1]["pg"] = pg
    return out


_ref_cache = {}


def rff_chain_ref(case, x=None, shadow=False, dtype=np.longdouble, order="plain", nw=1, defect=None, chains=None):
    """{value [K x n], grad [K x n x d], layers [chain][layer] -> dict(value, D, grad, S_value, S_D, S_grad)} of the chains
    (all; or the indices ``chains``) of ``case`` at the rows of ``x`` (the case's own) in ``dtype`` -- or, ``shadow``, the
    componentwise shadow S of value and grad.  ``order`` / ``nw``: the summation order (module docstring); ``defect``: one of
    RFF_DEFECTS planted in the values, never in the shadow.  Cached."""
    assert dtype is not np.longdouble or R.HAVE_LONGDOUBLE
    x = case["x"] if x is None else np.ascontiguousarray(x, np.float64)
    ks = tuple(range(case["K"])) if chains is None else tuple(chains)
    key = (case["name"], x.tobytes(), np.dtype(dtype).name, order, nw, defect, ks)
    if key not in _ref_cache:
        T = lambda a: np.asarray(a, dtype)
        lay = [_chain_run(case, k, x, T, order, nw, defect) for k in ks]
        stack = lambda f: np.stack([c[-1][f] for c in lay])
        _ref_cache[key] = (dict(value=stack("value"), grad=stack("grad"), layers=lay),
                           dict(value=stack("S_value"), grad=stack("S_grad")))
        if len(_ref_cache) > 400:
            _ref_cache.pop(next(iter(_ref_cache)))
    return _ref_cache[key][1 if shadow else 0]


def rff_layer1_ref(case, k, l, fprev, shadow=False, dtype=np.longdouble, order="plain", defect=None):
    """Layer l >= 1 of chain k by itself at the case's points on the GIVEN fprev (zero shadow): {value [n]} or its shadow."""
    T = lambda a: np.asarray(a, dtype)
    n, d = case["n"], case["d"]
    z = T(np.zeros((n, d)))
    val, _, _, _, S_val, _, _ = _layer_run(case["ops"][k][l], T(case["x"]), T(fprev), T(np.zeros(n)), 0, z, z, T, order, 1, defect)
    return dict(value=S_val if shadow else val)


def rff_gate(got, ref, S, names=RFF_GROUPS):
    """(violations [(name, ratio, non-zeros where S = 0)], {group: worst ratio}, report) of |got - ref| <= RFF_C u S."""
    rat = R.layer_ratios(got, ref, S, names)
    worst = {k: r for k, (r, _) in rat.items()}
    bad = [(k, r, nz) for k, (r, nz) in rat.items() if not r <= RFF_C[k] or nz]
    report = "  ".join("%s %.2f u S = %.0f%% of the gate" % (g, w, 100 * w / RFF_C[g]) for g, w in worst.items())
    return bad, worst, report


def seen(ref, S, name):
    """The median S / |value| of an output: what the gate can see."""
    v = np.abs(R.ld(ref[name])).reshape(-1)
    s = R.ld(S[name]).reshape(-1)
    ok = v > 0
    return float(np.median(s[ok] / v[ok])) if ok.any() else float("inf")


# ------------------------------------------------------------------------------------- the one-step model of the refinement
def _clamp(v):
    return np.minimum(np.maximum(v, 0), 1)


def _merit_at(case, p, x, dtype, order="plain", nw=1, defect=None, flip=False):
    """Problem p at the rows of x [n x d]: dict(f, S_f, s [C x n], S_s, neg [C x n], M, S_M, g [n x d], S_g, gf) -- the
    objective, the slacks c_i - thr_i, the merit f + rho0 / 2 sum_{s_i < 0} s_i^2 (every multiplier is zero in the first
    round) and its gradient grad f + sum_{s_i < 0} rho0 s_i grad c_i, summed over the threads AFTER the combination as the
    kernel does.  Shadows: S(s) = S(c) + |s|, S(M) = S(f) + sum rho0 (|s| S(s) + s^2 / 2), S(g) = S(grad f) + sum rho0 (S(s)
    |grad c| + |s| S(grad c))."""
    T = lambda a: np.asarray(a, dtype)
    cons, thr, rho = case["cons"][p], (case["thr"][p] if case["C"] else []), T(case["rho0"])
    ks = sorted({case["obj"][p]} | set(cons))
    kw = dict(dtype=dtype, order=order, nw=nw, defect=defect, chains=ks)
    ref, S = rff_chain_ref(case, x, **kw), rff_chain_ref(case, x, shadow=True, **kw)
    at = {k: i for i, k in enumerate(ks)}
    o = at[case["obj"][p]]
    f, S_f = ref["value"][o], S["value"][o]
    mg, M, S_M, S_g = ref["layers"][o][-1]["pg"], f, S_f, S["grad"][o]
    s, S_s = [], []
    for ci, t in zip(cons, thr):
        i = at[ci]
        si = ref["value"][i] - T(t)
        Ss = S["value"][i] + np.abs(si)
        neg = si < 0
        coef = np.where(neg, (-rho if flip else rho) * si, 0)
        M = M + np.where(neg, (rho * si) * (rho * si) / (2 * rho), 0)
        S_M = S_M + np.where(neg, rho * (np.abs(si) * Ss + si * si / 2), 0)
        mg = mg + coef[:, None, None] * ref["layers"][i][-1]["pg"]
        S_g = S_g + np.where(neg, rho, 0)[:, None] * (Ss[:, None] * np.abs(ref["grad"][i]) + np.abs(si)[:, None] * S["grad"][i])
        s.append(si)
        S_s.append(Ss)
    g = _across(mg, order, nw, 1 if defect == "wave_grad_dropped" else None)
    n = x.shape[0]
    return dict(f=f, S_f=S_f, s=np.array(s, dtype).reshape(len(cons), n), S_s=np.array(S_s, dtype).reshape(len(cons), n), M=M,
                S_M=S_M, g=g, S_g=S_g, gf=ref["grad"][o])


def rff_refine_step_ref(case):
    """The closed form of what mobocmf_rff_refine writes for outer = inner = 1, backtracks = restore = 0, per problem p:
    dict(feasible, xs [R x d], xs_bound, clamped [R x d]).  With every slack >= 0 at both points (or C = 0): xs = clamp(x0 -
    step0 grad f), fs = f(xs); with a slack < 0 at both: xs = clamp(x0 - step0 (grad f + sum_{s_i < 0} rho0 s_i grad c_i)), fs NaN,
    slack_min the smallest slack at xs.  Asserted in longdouble, for every start: every decision of the kernel on the way clears
    its own gate -- the sign of each slack at both points, the projected gradient's descent gl . dx < 0, ft < f0 (feasible),
    Mt <= M + armijo gd (infeasible: the accepted step is what is written), every unclamped component strictly inside (0, 1) and
    the clamped one strictly below 0 before the clamp.  xs_bound: step0 RFF_C['grad'] u S(g) plus the two roundings of the update."""
    assert R.HAVE_LONGDOUBLE
    key = ("step", case["name"])
    if key in _ref_cache:
        return _ref_cache[key]
    u, Cv, Cg = R.ld(R.U), RFF_C["value"], RFF_C["grad"]
    step = R.ld(case["step0"])
    out = []
    for p in range(case["P"]):
        tag = (case["name"], p)
        x = R.ld(_clamp(case["x0"][p]))
        a = _merit_at(case, p, np.asarray(x, np.float64), np.longdouble)
        assert np.all(np.abs(a["s"]) > Cv * u * a["S_s"]), tag
        feasible = bool(np.all(a["s"] >= 0))
        raw = x - step * a["g"]
        bound = step * Cg * u * a["S_g"] + u * (step * np.abs(a["g"]) + np.abs(raw))
        clamped = raw < 0
        assert np.all(np.where(clamped, raw + bound < 0, (raw - bound > 0) & (raw + bound < 1))), tag
        want = np.zeros(x.shape, bool)
        if case.get("clamped") is not None and case["clamped"][0] == p:
            want[case["clamped"][1], case["clamped"][2]] = True
        assert np.array_equal(clamped, want), tag
        xs = np.where(clamped, 0, raw)
        bound = np.where(clamped, 0, bound)
        dx = xs - x
        gd = (a["g"] * dx).sum(1)
        S_gd = (Cg * u * a["S_g"] * np.abs(dx) + np.abs(a["g"]) * (bound + u * np.abs(dx))).sum(1) + u * (np.abs(a["g"] * dx)).sum(1) * 8
        assert np.all(gd + S_gd < 0), tag
        # the trial point: the kernel's own lies within ``bound`` of xs, which moves every value by at most |gradient| . bound
        b = _merit_at(case, p, np.asarray(xs, np.float64), np.longdouble)
        xr = R.ld(np.asarray(xs, np.float64))
        move = lambda grad: (np.abs(grad) * (bound + np.abs(xs - xr))).sum(-1)
        ks = [case["obj"][p]] + list(case["cons"][p])
        gt = rff_chain_ref(case, np.asarray(xs, np.float64), chains=sorted(set(ks)))
        at = {k: i for i, k in enumerate(sorted(set(ks)))}
        mv_s = np.array([move(gt["grad"][at[ci]]) for ci in case["cons"][p]], np.longdouble).reshape(b["s"].shape)
        assert np.all(np.abs(b["s"]) > Cv * u * b["S_s"] + mv_s), tag
        assert np.array_equal(b["s"] < 0, a["s"] < 0) or (not feasible and np.all((b["s"] < 0).any(0))), tag
        if feasible:
            assert np.all(b["s"] >= 0), tag
            assert np.all(a["f"] - b["f"] > Cv * u * (a["S_f"] + b["S_f"]) + move(b["gf"])), tag
        else:
            assert np.all((a["s"] < 0).any(0)) and np.all((b["s"] < 0).any(0)), tag
        arm = R.ld(ARMIJO)
        room = a["M"] + arm * gd - b["M"]
        assert np.all(room > Cv * u * (a["S_M"] + b["S_M"]) + arm * S_gd + move(b["g"])), tag
        out.append(dict(feasible=feasible, xs=xs, xs_bound=bound, clamped=clamped))
    _ref_cache[key] = out
    return out


def rff_refine_step_f64(case, defect=None):
    """mobocmf_rff_refine for the one-step options restated in float64 in the kernel's order, decision by decision (the eight
    or four wavefronts' partial sums, the merit gradient combined per thread and summed once): {xs [P x R x d], fs, slack_min
    [P x R]}.  ``defect``: one of RFF_DEFECTS."""
    P, Rn, d, nw = case["P"], case["R"], case["d"], case["nw"]
    xs, fs, sm = np.full((P, Rn, d), np.nan), np.full((P, Rn), np.nan), np.full((P, Rn), np.nan)
    flip = defect == "merit_sign_flipped"
    ev = lambda p, x: _merit_at(case, p, x, np.float64, "refine", nw, defect, flip)
    smin = lambda e: e["s"].min(0) if case["C"] else np.full(e["f"].shape, np.inf)
    for p in range(P):
        x = _clamp(case["x0"][p])
        a = ev(p, x)
        xt = _clamp(x - case["step0"] * a["g"])
        dx = xt - x
        gd = (a["g"] * dx).sum(1)
        b = ev(p, xt)
        fa, fb = np.all(a["s"] >= 0, axis=0), np.all(b["s"] >= 0, axis=0)
        for r in range(Rn):
            best = None
            if fa[r]:
                best = (x[r], a["f"][r], smin(a)[r])
            if gd[r] < 0:
                if fb[r] and (best is None or b["f"][r] < best[1]):
                    best = (xt[r], b["f"][r], smin(b)[r])
                accepted = b["M"][r] <= a["M"][r] + ARMIJO * gd[r]
            else:
                accepted = False
            xl, sl = (xt[r], smin(b)[r]) if accepted else (x[r], smin(a)[r])
            xs[p, r], fs[p, r], sm[p, r] = (best[0], best[1], best[2]) if best else (xl, np.nan, sl)
    return dict(xs=xs, fs=fs, slack_min=sm)


def rff_refine_gate(case, got):
    """(violations, {'xs': worst |xs - ref| / xs_bound, 'value': worst err / (u S) of fs / slack_min}, report) of a one-step
    launch's {xs, fs, slack_min}.  xs against the model inside xs_bound, exact zeros on the clamped
    component; fs and slack_min inside the 'value' gate of the reference evaluated AT THE GOT xs, which is given data."""
    model = rff_refine_step_ref(case)
    u, Cv = R.ld(R.U), RFF_C["value"]
    bad, worst = [], dict(xs=0.0, value=0.0)
    for p, m in enumerate(model):
        xs = np.asarray(got["xs"][p], np.float64)
        err = np.abs(R.ld(xs) - m["xs"])
        if not np.all(xs[m["clamped"]] == 0.0):
            bad.append(("clamped", p, xs[m["clamped"]].tolist()))
        free = ~m["clamped"]
        with np.errstate(invalid="ignore"):
            r = float(np.max(np.where(np.isnan(err[free]), np.inf, err[free] / m["xs_bound"][free]), initial=0.0))
        worst["xs"] = max(worst["xs"], r)
        if not r <= 1:
            bad.append(("xs", p, r))
        if not np.all(np.isfinite(xs)):
            continue
        e = _merit_at(case, p, xs, np.longdouble)
        fs, sm = R.ld(got["fs"][p]), R.ld(got["slack_min"][p])
        rv = 0.0
        if m["feasible"]:
            rv = float(np.max(np.abs(fs - e["f"]) / (u * e["S_f"])))
        elif not np.all(np.isnan(got["fs"][p])):
            bad.append(("fs not NaN", p, np.asarray(got["fs"][p]).tolist()))
        if case["C"]:
            rv = max(rv, float(np.max(np.abs(sm - e["s"].min(0)) / (u * e["S_s"].max(0)))))
        elif not np.all(np.isposinf(np.asarray(got["slack_min"][p], np.float64))):
            bad.append(("slack_min", p, np.asarray(got["slack_min"][p]).tolist()))
        rv = np.inf if np.isnan(rv) else rv
        worst["value"] = max(worst["value"], rv)
        if not rv <= Cv:
            bad.append(("value", p, rv))
    report = "xs %.0f%% of its bound  value %.2f u S = %.0f%% of the gate" % (100 * worst["xs"], worst["value"], 100 * worst["value"] / Cv)
    return bad, worst, report


# ------------------------------------------------------------ the direct callers: NaN-filled outputs with GUARD doubles behind
class RffLaunch:
    """``case`` on the device: x, params, the descriptor table of the chains ``chains`` (all).  Every method poisons its
    outputs, launches, synchronises and returns a dict of numpy results with "rc" and "guards" (every guard double still
    NaN)."""

    def __init__(self, case, chains=None):
        from mobocmf_amd import functional
        self.case, self.d = case, case["d"]
        self.ks = list(range(case["K"])) if chains is None else list(chains)
        self.x, self.params = R._dev(case["x"]), R._dev(case["params"])
        self.plen = case["params"].size
        self.desc = functional._rff_chain_table("rff_reference", [case["layers"][k] for k in self.ks], self.d, self.plen,
                                                self.params.device)
        R.torch.cuda.synchronize()

    def _collect(self, rc, bufs, shapes):
        R.torch.cuda.synchronize()
        out = dict(rc=rc, guards=all(bool(R.torch.isnan(bufs[k][int(np.prod(s)):]).all()) for k, s in shapes.items()))
        out.update({k: bufs[k][:int(np.prod(s))].cpu().numpy().reshape(s) for k, s in shapes.items()})
        return out

    def eval_chains(self):
        K, n = len(self.ks), self.case["n"]
        b = dict(value=R._out(K * n))
        rc = R.lib().mobocmf_rff_eval_chains(K, self.d, n, R._p(self.x), R._p(self.params), self.plen, R._p(self.desc),
                                             R._p(b["value"]), R._stream())
        return self._collect(rc, b, dict(value=(K, n)))

    def eval_layer1(self, k, l, fprev):
        """Layer l >= 1 of chain k through mobocmf_rff_eval (kind 1) on the given fprev."""
        n, e = self.case["n"], self.case["layers"][k][l]
        at = lambda name: ctypes.c_void_p(self.params.data_ptr() + 8 * e[name])
        fp = R._dev(fprev)
        b = dict(value=R._out(n))
        rc = R.lib().mobocmf_rff_eval(1, self.d, e["F"], n, R._p(self.x), R._p(fp), at("W1"), at("b1"), at("Wf"), at("W2"), at("b2"),
                                      at("theta"), e["s0"], e["s1"], e["s2"], R._p(b["value"]), R._stream())
        return self._collect(rc, b, dict(value=(n,)))

    def value_grad(self):
        K, n = len(self.ks), self.case["n"]
        b = dict(value=R._out(K * n), grad=R._out(K * n * self.d))
        rc = R.lib().mobocmf_rff_chains_value_grad(K, self.d, n, R._p(self.x), R._p(self.params), self.plen, R._p(self.desc),
                                                   R._p(b["value"]), R._p(b["grad"]), R._stream())
        return self._collect(rc, b, dict(value=(K, n), grad=(K, n, self.d)))

    def refine_step(self, only=None):
        """The one-step options on every start of every problem, or on the single start ``only`` = (p, r)."""
        from mobocmf_amd import functional
        c, d, torch = self.case, self.d, R.torch
        ps = range(c["P"]) if only is None else [only[0]]
        x0 = c["x0"] if only is None else c["x0"][only[0]:only[0] + 1, only[1]:only[1] + 1]
        P, Rn = x0.shape[:2]
        cnt = [len(c["cons"][p]) for p in ps]
        off = [sum(cnt[:i]) for i in range(P)]
        con = [ci for p in ps for ci in c["cons"][p]]
        thr = [t for p in ps for t in (c["thr"][p] if c["C"] else [])]
        i32 = lambda v: (ctypes.c_int32 * max(1, len(v)))(*v)
        con_d = torch.tensor(con, dtype=torch.int32).cuda() if con else None
        thr_d, x0_d = (R._dev(np.array(thr)) if con else None), R._dev(x0)
        opt = functional.rff_refine_options(outer=1, inner=1, backtracks=0, restore=0, step0=c["step0"], rho0=c["rho0"])
        b = dict(xs=R._out(P * Rn * d), fs=R._out(P * Rn), slack_min=R._out(P * Rn), x_best=R._out(P * d), f_best=R._out(P))
        ints = torch.full((2 * P + R.GUARD,), -7, dtype=torch.int32, device="cuda")
        rc = R.lib().mobocmf_rff_refine(P, Rn, d, len(self.ks), i32([c["obj"][p] for p in ps]), i32(off), i32(cnt), len(con),
                                        R._p(con_d), R._p(thr_d), R._p(x0_d), R._p(self.params), self.plen, R._p(self.desc),
                                        ctypes.byref(opt), R._p(b["xs"]), R._p(b["fs"]), R._p(b["slack_min"]), R._p(b["x_best"]),
                                        R._p(b["f_best"]), ctypes.c_void_p(ints.data_ptr()), ctypes.c_void_p(ints.data_ptr() + 4 * P),
                                        R._stream())
        out = self._collect(rc, b, dict(xs=(P, Rn, d), fs=(P, Rn), slack_min=(P, Rn), x_best=(P, d), f_best=(P,)))
        out["guards"] = out["guards"] and bool((ints[2 * P:] == -7).all())
        out["start_best"], out["status"] = ints[:P].cpu().numpy(), ints[P:2 * P].cpu().numpy()
        return out
