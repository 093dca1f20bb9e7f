"""numpy ``longdouble`` restatement of the exact-GP function sample (include/mobocmf_hip.h, mobocmf_exact_sample_*;
mobocmf_amd/util/exact_sample.py) from EXPLICIT draws: the yardstick of the host and the device engine.

    C_sig = cos(W_sig x + b_sig), C_noi = cos(W_noi x + b_noi)  (F x n),  c = sqrt(2 a / F)
    Phi   = [ s(l_i) c_sig C_sig ; sqd[l] c_noi C_noi [l_i >= l],  l = 0 .. n_levels - 1 ]
    G     = Phi^T Phi + noise I = s_i s_j c_sig^2 C_sig^T C_sig + ntab[min(l_i, l_j)] c_noi^2 C_noi^T C_noi + noise I
    r     = y - Phi^T theta0 - e,   w = G^-1 r,   theta = theta0 + Phi w
    g_f   : theta'_f = [ s(f) c_sig theta_sig ; c_noi sum_{l <= f} sqd[l] theta_noi,l ]  on  cos([W_sig; W_noi] x + [b_sig; b_noi])

Also the componentwise error bounds of the gram launch (``gram_bounds``), derived from operation counts:

  * a cosine.  Its argument b + sum_k W_k x_k is formed by d fused multiply-adds: at most (d + 1) u A, A = |b| + sum_k |W_k x_k|,
    off the exact argument; |cos'| <= 1 carries that to the value; the cosine itself is allowed 4 u (HIP's double-precision cos is
    documented at 2 ulp and an ulp of a value below 1 is at most u; doubled, for the reduction of a large argument):
        eps = u ((d + 1) A + 4)
  * a product sum S_ij = sum_f c_fi c_fj over F features in the matrix instruction (fused, one rounding per accumulation):
        |S^ - S| <= sum_f (eps_fi + eps_fj) + (F + 1) u sum_f |c_fi c_fj|
  * the epilogue: c^2 = 2 a / F (two roundings), three factors, the sum of the two terms and the noise: 8 u on the magnitudes.
        bound_ij = |s_i s_j| c_sig^2 E^sig_ij + ntab c_noi^2 E^noi_ij + 8 u (|s_i s_j| c_sig^2 Sabs^sig + ntab c_noi^2 Sabs^noi + noise)
  * r_i likewise, with theta0 in the place of the second cosine ((F + 4) u for the four partial sums added afterwards), sqrt(c^2)
    one rounding more, and 8 u (|y_i| + sum |terms| + |e_i|) for the level sum and the two subtractions.
"""
import numpy as np

U = 2.0 ** -53
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 2.0 ** -60


def ld(a):
    return np.asarray(a, np.longdouble)


def tables(ntab):
    """sqd of a noise table: sqrt of its increments (the first one is ntab[0])."""
    ntab = np.asarray(ntab, np.float64)
    return np.sqrt(np.maximum(np.diff(np.concatenate([[0.0], ntab])), 0.0))


def chol_solve(G, r):
    """G^-1 r by a Cholesky factorisation, in the dtype of G (longdouble has no LAPACK)."""
    n = G.shape[0]
    L = np.zeros_like(G)
    for j in range(n):
        v = G[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    z = np.zeros_like(r)
    for i in range(n):
        z[i] = (r[i] - L[i, :i] @ z[:i]) / L[i, i]
    w = np.zeros_like(r)
    for i in range(n - 1, -1, -1):
        w[i] = (z[i] - L[i + 1:, i] @ w[i + 1:]) / L[i, i]
    return w


def restate(x, lev, y, sig, ntab, scal, W_sig, b_sig, W_noi, b_noi, theta0, e, levels=(), solve=True):
    """Every quantity of the draw in longdouble from float64 operands.  Returns a dict: G (both statements: ``G`` from the
    tables, ``G_phi`` from the feature expansion), r, w, theta, folded[level], Phi, and what ``gram_bounds`` needs.
    ``solve=False``: neither the expansion's product nor the solve (the gram launch's checks at large F)."""
    assert HAVE_LONGDOUBLE
    x, y, sig, ntab = ld(x), ld(y), ld(sig), ld(ntab)
    lev = np.asarray(lev, np.int64)
    sqd = np.sqrt(np.maximum(np.diff(np.concatenate([ld([0.0]), ntab])), ld(0.0)))
    a_sig, a_noi, noise = ld(scal[0]), ld(scal[1]), ld(scal[2])
    W_sig, b_sig, W_noi, b_noi, theta0, e = ld(W_sig), ld(b_sig), ld(W_noi), ld(b_noi), ld(theta0), ld(e)
    F, d = W_sig.shape
    n, nl = x.shape[0], sig.shape[0]
    c_sig, c_noi = np.sqrt(2 * a_sig / F), np.sqrt(2 * a_noi / F)
    C_sig, C_noi = np.cos(W_sig @ x.T + b_sig[:, None]), np.cos(W_noi @ x.T + b_noi[:, None])
    blocks = [sig[lev] * c_sig * C_sig] + [sqd[l] * c_noi * C_noi * (lev >= l) for l in range(nl)]
    Phi = np.concatenate(blocks, 0)
    s_i = sig[lev]
    nt = ntab[np.minimum(lev[:, None], lev[None, :])]
    eye = np.eye(n, dtype=np.longdouble)
    G = s_i[:, None] * s_i[None, :] * c_sig ** 2 * (C_sig.T @ C_sig) + nt * c_noi ** 2 * (C_noi.T @ C_noi) + noise * eye
    out = dict(G=G, G_phi=Phi.T @ Phi + noise * eye if solve else None, Phi=Phi, r=y - Phi.T @ theta0 - e, sqd=sqd, c_sig=c_sig, c_noi=c_noi,
               C_sig=C_sig, C_noi=C_noi, s_i=s_i, nt=nt, noise=noise, F=F, d=d,
               A_sig=np.abs(b_sig)[:, None] + np.abs(W_sig) @ np.abs(x).T, A_noi=np.abs(b_noi)[:, None] + np.abs(W_noi) @ np.abs(x).T,
               theta0=theta0, y=y, e=e, lev=lev)
    if solve:
        out["w"] = chol_solve(G, out["r"])
        out["theta"] = theta0 + Phi @ out["w"]
        out["folded"] = {int(f): fold(out["theta"], int(f), sig, sqd, c_sig, c_noi, F) for f in levels}
    return out


def fold(theta, level, sig, sqd, c_sig, c_noi, F):
    noi = sum(sqd[l] * theta[(1 + l) * F:(2 + l) * F] for l in range(level + 1))
    return np.concatenate([sig[level] * c_sig * theta[:F], c_noi * noi])


def gram_bounds(R):
    """(bound on |G^ - G| (n x n), bound on |r^ - r| (n)) of the gram launch for the restatement ``R``: the module's derivation."""
    u, F, d = ld(U), R["F"], R["d"]
    out = []
    eps = {k: u * ((d + 1) * R["A_" + k] + 4) for k in ("sig", "noi")}
    E, Sabs = {}, {}
    for k in ("sig", "noi"):
        C = np.abs(R["C_" + k])
        Sabs[k] = C.T @ C
        col = eps[k].sum(0)                                   # sum_f eps_fi
        E[k] = col[:, None] + col[None, :] + (F + 1) * u * Sabs[k]
    ss = np.abs(R["s_i"][:, None] * R["s_i"][None, :]) * R["c_sig"] ** 2
    nn = R["nt"] * R["c_noi"] ** 2
    out.append(ss * E["sig"] + nn * E["noi"] + 8 * u * (ss * Sabs["sig"] + nn * Sabs["noi"] + R["noise"]))
    nl = R["sqd"].shape[0]
    t0 = np.abs(R["theta0"])
    ts = np.abs(R["s_i"]) * R["c_sig"]
    mag = ts * (np.abs(R["C_sig"]) * t0[:F, None]).sum(0)
    br = ts * ((eps["sig"] * t0[:F, None]).sum(0) + (F + 4) * u * (np.abs(R["C_sig"]) * t0[:F, None]).sum(0))
    for l in range(nl):
        tl = t0[(1 + l) * F:(2 + l) * F, None]
        on = (R["lev"] >= l) * R["sqd"][l] * R["c_noi"]
        m = (np.abs(R["C_noi"]) * tl).sum(0)
        mag = mag + on * m
        br = br + on * ((eps["noi"] * tl).sum(0) + (F + 4) * u * m)
    out.append(br + 8 * u * (np.abs(R["y"]) + mag + np.abs(R["e"])))
    return out


def case(n, d, nl, F, kernel="min", seed=0, noise=1e-2, empty_level=None):
    """Operands of one problem as float64 numpy: inputs in [0, 1]^d, levels cycling over the n_levels (``empty_level``: a level
    no row has), lengthscales around 0.5 sqrt(d), the tables of MFKernel ("min": s = 1, ntab[t] = t) or MFKernel_lin ("lin":
    s[l] = prod rho, ntab its rho polynomial)."""
    rng = np.random.default_rng([seed, n, d, nl, F])
    x = rng.random((n, d))
    lev = np.arange(n) % nl
    if empty_level is not None and nl > 1:
        lev = np.where(lev == empty_level, (empty_level + 1) % nl, lev)
    y = rng.standard_normal(n)
    if kernel == "min":
        sig, ntab = np.ones(nl), np.arange(nl, dtype=np.float64)
    else:
        rho = 0.5 + rng.random(max(nl - 1, 1))
        sig = np.concatenate([[1.0], np.cumprod(rho[:nl - 1])])[:nl]
        t = np.arange(nl) + 1.0
        ntab = (t >= 2).astype(np.float64)
        for k in range(3, nl - 1):
            ntab = ntab + (t >= k) * rho[k - 2] ** 2
    ls_s, ls_n = 0.5 * np.sqrt(d) * (0.7 + 0.6 * rng.random(d)), 0.3 * np.sqrt(d) * (0.7 + 0.6 * rng.random(d))
    scal = np.array([0.8 + 0.4 * rng.random(), 0.1 + 0.1 * rng.random(), noise])
    return dict(x=x, lev=lev.astype(np.int32), y=y, sig=sig, ntab=ntab, scal=scal,
                W_sig=rng.standard_normal((F, d)) / ls_s, b_sig=2 * np.pi * rng.random(F),
                W_noi=rng.standard_normal((F, d)) / ls_n, b_noi=2 * np.pi * rng.random(F),
                theta0=rng.standard_normal((1 + nl) * F), e=np.sqrt(noise) * rng.standard_normal(n))
