"""numpy restatement of mobocmf_nsga_survive / mobocmf_nsga_vary as include/mobocmf_hip.h states them (written from the header,
not from csrc/pareto_evolve.hip), with Philox4x32-10 and the draw addressing, and the generation loop of
util/pareto_evolve.py around an ``evaluate(X) -> (F (k, n), viol (n,) >= 0 or None)`` callback."""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
DEFAULTS = {"eta_c": 15.0, "p_c": 0.9, "eta_m": 20.0, "p_m": 0.0}


def philox4x32_10(c, k):
    """Ten rounds of Philox4x32 (Salmon et al. 2011) on counters ``c`` (4 arrays of 32-bit values held in uint64) and key
    ``k`` (2 ints)."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _MASK for v in c)
    k0, k1 = int(k[0]) & 0xFFFFFFFF, int(k[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_uniform(seed, call, idx):
    """(0, 1) with 53 random bits: counter (idx low, idx high, call low, call high), key (seed low, seed high)."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    call_lo, call_hi = np.full(idx.shape, call & 0xFFFFFFFF, dtype=np.uint64), np.full(idx.shape, call >> 32, dtype=np.uint64)
    r0, r1, _, _ = philox4x32_10((idx & _MASK, idx >> np.uint64(32), call_lo, call_hi), (seed & 0xFFFFFFFF, seed >> 32))
    bits = ((r0 >> np.uint64(5)) << np.uint64(26)) | (r1 >> np.uint64(6))
    return (bits.astype(np.float64) + 0.5) * 1.1102230246251565e-16


# ------------------------------------------------------------------ survive
def dominance(F, viol):
    """(dom (n, n) bool: dom[i, j] = row i dominates row j; the violation as used)."""
    F = np.asarray(F, dtype=np.float64)
    n = F.shape[1]
    v = np.zeros(n) if viol is None else np.array(viol, dtype=np.float64)
    v[np.isnan(F).any(0) | np.isnan(v)] = np.inf
    feas = v == 0.0
    with np.errstate(invalid="ignore"):
        le = np.ones((n, n), dtype=bool)
        lt = np.zeros((n, n), dtype=bool)
        for c in range(F.shape[0]):
            le &= F[c][:, None] <= F[c][None, :]
            lt |= F[c][:, None] < F[c][None, :]
        ff = feas[:, None] & feas[None, :]
        ii = ~feas[:, None] & ~feas[None, :]
        dom = (feas[:, None] & ~feas[None, :]) | (ii & (v[:, None] < v[None, :])) | (ff & le & lt)
    return dom, v


def ranks(dom):
    n = dom.shape[0]
    rank = np.full(n, -1, dtype=np.int32)
    alive = np.ones(n, dtype=bool)
    held = dom.sum(0)                       # living dominators of every row
    r = 0
    while alive.any():
        front = alive & (held == 0)
        rank[front] = r
        alive &= ~front
        held = held - dom[front].sum(0)
        r += 1
    return rank


def crowding(F, rank):
    F = np.asarray(F, dtype=np.float64)
    g_all = np.where(np.isnan(F), np.inf, F)
    crowd = np.zeros(F.shape[1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(int(rank.max()) + 1):
            idx = np.flatnonzero(rank == r)
            for c in range(F.shape[0]):
                g = g_all[c, idx]
                order = np.lexsort((idx, g))
                s = g[order]
                term = np.full(len(idx), np.inf)
                if len(idx) > 2:
                    mn, mx = s[0], s[-1]
                    if mx == mn:
                        term[1:-1] = 0.0
                    else:
                        t = (s[2:] - s[:-2]) / (mx - mn)
                        term[1:-1] = np.where(np.isnan(t), 0.0, t)
                crowd[idx[order]] = crowd[idx[order]] + term
    return crowd


def survive(X, F, viol, n_keep=None):
    """dict X (n_keep, d), F (k, n_keep), viol (n_keep,), rank (int32), crowd, src (int32), in key order."""
    X, F = np.asarray(X, dtype=np.float64), np.asarray(F, dtype=np.float64)
    n = X.shape[0]
    n_keep = n if n_keep is None else n_keep
    dom, v = dominance(F, viol)
    rank = ranks(dom)
    crowd = crowding(F, rank)
    order = np.lexsort((np.arange(n), -crowd, rank))[:n_keep]
    return {"X": X[order], "F": F[:, order], "viol": v[order], "rank": rank[order], "crowd": crowd[order],
            "src": order.astype(np.int32)}


# ------------------------------------------------------------------ vary
_LN2 = 0.6931471805599453


def _lg(x):
    m, n = np.frexp(x)
    low = m < 0.7071067811865476
    m, n = np.where(low, 2.0 * m, m), np.where(low, n - 1, n)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    P = np.full(np.shape(x), 1.0 / 23.0)
    for j in range(21, 0, -2):
        P = P * z + 1.0 / j
    return n.astype(np.float64) * _LN2 + (2.0 * s) * P


def _ex(y):
    n = np.rint(y * 1.4426950408889634)
    r = y - n * _LN2
    T = np.ones(np.shape(y))
    for j in range(14, 0, -1):
        T = 1.0 + (r * T) / j
    return np.ldexp(T, n.astype(np.int32))


def pw(x, e):
    """x^e (x > 0) as the header builds it from IEEE operations."""
    return _ex(e * _lg(np.asarray(x, dtype=np.float64)))


def vary(X, rank, crowd, seed, generation, eta_c=15.0, p_c=0.9, eta_m=20.0, p_m=0.0):
    """(children (Np, d), parents (Np,) int32)."""
    X = np.asarray(X, dtype=np.float64)
    Np, d = X.shape
    p_m = 1.0 / d if p_m == 0.0 else p_m
    q = np.arange(Np // 2, dtype=np.uint64)
    base = q << np.uint64(32)
    u = lambda slot: philox_uniform(seed, generation, base + np.uint64(slot))
    par = np.zeros((Np // 2, 2), dtype=np.int64)
    for e in range(2):
        a = np.minimum(np.floor(u(2 * e) * Np).astype(np.int64), Np - 1)
        b = np.minimum(np.floor(u(2 * e + 1) * Np).astype(np.int64), Np - 1)
        ra, rb, ca, cb = rank[a], rank[b], crowd[a], crowd[b]
        a_wins = (ra < rb) | ((ra == rb) & ((ca > cb) | (~(cb > ca) & (a <= b))))
        par[:, e] = np.where(a_wins, a, b)
    children = np.zeros((Np, d))
    cross = u(4) < p_c
    for v in range(d):
        p0, p1 = X[par[:, 0], v], X[par[:, 1], v]
        w = u(9 + 8 * v)
        ex = 1.0 / (eta_c + 1.0)
        beta = np.where(w <= 0.5, pw(2.0 * w, ex), pw(1.0 / (2.0 * (1.0 - w)), ex))
        do = cross & (u(8 + 8 * v) < 0.5)
        c = [np.where(do, 0.5 * ((1.0 + beta) * p0 + (1.0 - beta) * p1), p0),
             np.where(do, 0.5 * ((1.0 - beta) * p0 + (1.0 + beta) * p1), p1)]
        for e in range(2):
            w = u(11 + 8 * v + 2 * e)
            ex = 1.0 / (eta_m + 1.0)
            delta = np.where(w < 0.5, pw(2.0 * w, ex) - 1.0, 1.0 - pw(2.0 * (1.0 - w), ex))
            x = np.where(u(10 + 8 * v + 2 * e) < p_m, c[e] + delta, c[e])
            children[e::2, v] = np.minimum(np.maximum(x, 0.0), 1.0)
    return children, par.reshape(-1).astype(np.int32)


# ------------------------------------------------------------------ the generation loop
def evolve(x0, evaluate, generations, seed, on_generation=None, **options):
    """The loop of util/pareto_evolve.py: rank the evaluated ``x0``; per generation g = 0, 1, ...: children by ``vary`` with
    generation word g, ``evaluate`` on the children only, ``survive`` on [parents; children].  Returns the last survivors."""
    opt = dict(DEFAULTS, **options)
    x0 = np.asarray(x0, dtype=np.float64)
    Np = x0.shape[0]
    F, viol = evaluate(x0)
    pop = survive(x0, F, viol)
    has_viol = viol is not None
    for g in range(generations):
        children, _ = vary(pop["X"], pop["rank"], pop["crowd"], seed, g, **opt)
        Fc, vc = evaluate(children)
        X2, F2 = np.concatenate((pop["X"], children)), np.concatenate((pop["F"], Fc), 1)
        v2 = np.concatenate((pop["viol"], vc)) if has_viol else None
        pop = survive(X2, F2, v2, Np)
        if on_generation is not None:
            on_generation(g, X2, F2, v2, pop)
    return pop


# ------------------------------------------------------------------ helpers of the tests
def hv2d(front, ref):
    """Exact hypervolume of (n, 2) minimised points against ``ref``."""
    P = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    P = P[(P <= ref).all(1)]
    if not len(P):
        return 0.0
    P = P[np.lexsort((P[:, 1], P[:, 0]))]
    best, hv = ref[1], 0.0
    for x, y in P:
        if y < best:
            hv += (ref[0] - x) * (best - y)
            best = y
    return hv


def front_mask(Fm):
    """Non-dominated rows of (n, k) (minimised; of equal rows all are kept)."""
    Fm = np.asarray(Fm)
    le = (Fm[:, None, :] <= Fm[None, :, :]).all(2)
    lt = (Fm[:, None, :] < Fm[None, :, :]).any(2)
    return ~(le & lt).any(0)
