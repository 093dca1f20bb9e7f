"""The mini-batch sampler's epoch permutation, the parts that need no GPU: mobocmf_minibatch_permutation_host is a bijection,
equals a numpy restatement written here from DESIGN.md 5.3, passes two derived uniformity bounds on fixed seeds, and the
C-ABI refuses malformed calls on the host."""
import ctypes

import numpy as np
import pytest

ROUNDS = 6


def host_perm(seed, epoch, N):
    from mobocmf_amd import _lib
    lib = _lib.load()
    out = np.empty(N, dtype=np.int64)
    rc = lib.mobocmf_minibatch_permutation_host(seed, epoch, N, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == _lib.OK
    return out


# ------------------------------------------------------------------ DESIGN.md 5.3 in numpy
def philox_word0(c0, c1, c2, c3, k0, k1):
    """Word 0 of Philox4x32-10 (Salmon et al. 2011), vectorised over c0; everything uint64 holding 32-bit values."""
    m32 = np.uint64(0xFFFFFFFF)
    c0 = c0.astype(np.uint64)
    c1, c2, c3 = (np.full_like(c0, v) for v in (c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0


def numpy_perm(seed, epoch, N):
    b = int(N - 1).bit_length()
    hb = b // 2
    ha = b - hb
    ma, mb = np.uint64((1 << ha) - 1), np.uint64((1 << hb) - 1)
    s_lo, s_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    e_lo, e_hi = epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF

    def once(v):
        A, B = v >> np.uint64(hb), v & mb
        for r in range(ROUNDS):
            if r % 2 == 0:
                A = A ^ (philox_word0(B, r, e_lo, e_hi, s_lo, s_hi) & ma)
            else:
                B = B ^ (philox_word0(A, r, e_lo, e_hi, s_lo, s_hi) & mb)
        return (A << np.uint64(hb)) | B

    v = once(np.arange(N, dtype=np.uint64))
    while True:                                  # cycle-walking: again while the value is outside 0..N-1
        out = v >= np.uint64(N)
        if not out.any():
            return v.astype(np.int64)
        v[out] = once(v[out])


SIZES = [1, 2, 3, 5, 17, 1000, 4096, 4097, 65537, 262145]


@pytest.mark.parametrize("N", SIZES)
def test_host_permutation_is_a_bijection_and_depends_on_epoch_and_seed(N):
    p = host_perm(7, 0, N)
    assert np.array_equal(np.sort(p), np.arange(N))
    q, r = host_perm(7, 1, N), host_perm(8, 0, N)
    assert np.array_equal(np.sort(q), np.arange(N)) and np.array_equal(np.sort(r), np.arange(N))
    if N >= 17:                                  # below that two draws coincide with noticeable probability (1/N!)
        assert not np.array_equal(p, q) and not np.array_equal(p, r)
    assert np.array_equal(p, host_perm(7, 0, N))


@pytest.mark.parametrize("N", SIZES)
def test_numpy_restatement_of_the_definition_equals_the_host_function_bitwise(N):
    for seed, epoch in ((0, 0), (3, 5), (2 ** 61 + 12345, 2 ** 33 + 7), (-5, 1)):
        assert np.array_equal(numpy_perm(seed, epoch, N), host_perm(seed, epoch, N)), (seed, epoch)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_uniformity_of_positions_and_of_batch_co_occurrence(seed):
    """N = 4096, 256 epochs, B = 256.  (a) the 16 x 16 table of (row // 256, position // 256) counts: under a uniform
    permutation its chi-square has 225 degrees of freedom; bound = the 1 - 1e-6 quantile, 340.6 (scipy.stats.chi2.ppf).
    (b) how often rows r and r + 1 share a batch: Binomial((N - 1) * 256, (B - 1) / (N - 1)); |z| <= 5.  Both bounds are
    derived, not measured (numpy's own shuffle scores about 202 and z = 0.64)."""
    N, E, B = 4096, 256, 256
    table = np.zeros((16, 16))
    same = 0
    for e in range(E):
        p = host_perm(seed, e, N)                # p[position] = row
        np.add.at(table, (p // 256, np.arange(N) // 256), 1)
        batch_of_row = np.empty(N, dtype=np.int64)
        batch_of_row[p] = np.arange(N) // B
        same += int((batch_of_row[:-1] == batch_of_row[1:]).sum())
    expected = N * E / 256.0
    chi2 = float(((table - expected) ** 2 / expected).sum())
    n, q = (N - 1) * E, (B - 1) / (N - 1)
    z = (same - n * q) / np.sqrt(n * q * (1 - q))
    print("seed %d: chi-square %.1f (bound 340.6), z %.2f (bound 5)" % (seed, chi2, z))
    assert chi2 < 340.6
    assert abs(z) <= 5.0


def test_library_refuses_bad_minibatch_arguments_before_touching_a_gpu():
    from mobocmf_amd import _lib
    lib = _lib.load()
    for name in ("mobocmf_minibatch_permutation_host", "mobocmf_minibatch_indices", "mobocmf_minibatch_gather",
                 "mobocmf_minibatch_accumulate"):
        assert hasattr(lib, name)
    out = np.empty(8, dtype=np.int64)
    po = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.mobocmf_minibatch_permutation_host(0, 0, 0, po) == _lib.BAD_ARG
    assert lib.mobocmf_minibatch_permutation_host(0, 0, -3, po) == _lib.BAD_ARG
    assert lib.mobocmf_minibatch_permutation_host(0, 0, _lib.MINIBATCH_MAX_ROWS + 1, po) == _lib.BAD_ARG
    assert lib.mobocmf_minibatch_permutation_host(0, -1, 8, po) == _lib.BAD_ARG
    assert lib.mobocmf_minibatch_permutation_host(0, 0, 8, None) == _lib.BAD_ARG
    p = ctypes.c_void_p(4096)                    # never dereferenced: every call below is refused on the host

    def indices(N=100, B=16, L=2, fid=p, order=1, rows=16, state=p, src=p, counts=p):
        return lib.mobocmf_minibatch_indices(N, B, L, fid, order, rows, state, src, counts, None)

    assert indices(N=0) == _lib.BAD_ARG and indices(N=_lib.MINIBATCH_MAX_ROWS + 1) == _lib.BAD_ARG
    assert indices(B=0) == _lib.BAD_ARG and indices(B=2 ** 31) == _lib.BAD_ARG
    assert indices(L=0) == _lib.BAD_ARG and indices(L=_lib.MINIBATCH_MAX_LEVELS + 1) == _lib.BAD_ARG
    assert indices(order=2) == _lib.BAD_ARG
    assert indices(rows=0) == _lib.BAD_ARG and indices(rows=17) == _lib.BAD_ARG
    assert indices(N=10, B=16, rows=11) == _lib.BAD_ARG
    for arg in ("fid", "state", "src", "counts"):
        assert indices(**{arg: None}) == _lib.BAD_ARG, arg

    def gather(N=100, d=2, rows=16, **kw):
        a = dict(x=p, y=p, fid=p, src=p, state=p, xb=p, yb=p, fidb=p)
        a.update(kw)
        return lib.mobocmf_minibatch_gather(N, d, rows, a["x"], a["y"], a["fid"], a["src"], a["state"], a["xb"], a["yb"],
                                            a["fidb"], None)

    assert gather(N=0) == _lib.BAD_ARG and gather(d=0) == _lib.BAD_ARG and gather(d=_lib.MAX_D + 1) == _lib.BAD_ARG
    assert gather(rows=0) == _lib.BAD_ARG and gather(rows=101) == _lib.BAD_ARG
    for arg in ("x", "y", "fid", "src", "state", "xb", "yb", "fidb"):
        assert gather(**{arg: None}) == _lib.BAD_ARG, arg
    assert lib.mobocmf_minibatch_accumulate(0, 16, p, p, p, p, None) == _lib.BAD_ARG
    assert lib.mobocmf_minibatch_accumulate(100, 0, p, p, p, p, None) == _lib.BAD_ARG
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert lib.mobocmf_minibatch_accumulate(100, 16, *args, None) == _lib.BAD_ARG


def test_fitter_surface_without_a_gpu():
    """The step class and the functional wrappers exist; without a GPU they raise the package's no-fallback error."""
    import torch
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    from mobocmf_amd.util.graphed_step import GraphedELBOStep, GraphedMiniBatchStep
    assert issubclass(GraphedMiniBatchStep, GraphedELBOStep)
    for name in ("minibatch_state", "minibatch_indices", "minibatch_gather"):
        assert callable(getattr(F, name))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.MobocmfError):
            F.minibatch_state(1, "cpu")
