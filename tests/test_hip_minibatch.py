"""Mini-batches drawn on the device (csrc/minibatch.hip, GraphedMiniBatchStep, the fitter's captured mini-batch path): the index
launch against the host statement of the permutation, the gather, the rows_expected guard, one step and the Adam trajectory
against the ORACLE evaluated on the rows the step reports, captured replay against the eager launches, rollback, the fitter."""
import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests.test_hip_model import _model_param_for, _raw_from_model, rel
from tests.test_minibatch_cpu import host_perm

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fid(N, L, seed=0):
    """Interleaved fidelities (what a shuffled loader sees), every level present."""
    f = np.random.default_rng(seed).integers(0, L, N).astype(np.float64)
    f[:L] = np.arange(L)
    return f


# ------------------------------------------------------------------ 5. the index launch
@pytest.mark.parametrize("N,B", [(45, 16), (512, 192), (8192, 2048), (8192, 3000), (100003, 4096)])
@pytest.mark.parametrize("L", [2, 3])
def test_index_launch_equals_the_host_permutation(N, B, L):
    from mobocmf_amd import functional as F
    seed = 1234 + N
    fid_h = _fid(N, L)
    fid = torch.tensor(fid_h, device=DEV)[:, None]
    nb = -(-N // B)
    st_u, st_o = F.minibatch_state(seed, DEV), F.minibatch_state(seed, DEV)
    counts_u = torch.zeros(8, dtype=torch.int64, device=DEV)
    counts_o = torch.zeros(8, dtype=torch.int64, device=DEV)
    for epoch in range(3):
        perm = host_perm(seed, epoch, N)
        seen = []
        for k in range(nb):
            rows = min(B, N - k * B)
            src_u = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
            src_o = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
            F.minibatch_indices(st_u, fid, B, L, src_u, counts_u, order_by_fidelity=False)
            F.minibatch_indices(st_o, fid, B, L, src_o, counts_o, order_by_fidelity=True)
            want = perm[k * B:k * B + rows]
            su, so = src_u.cpu().numpy(), src_o.cpu().numpy()
            assert np.array_equal(su, want), (epoch, k)
            order = np.argsort(-fid_h[want], kind="stable")
            assert np.array_equal(so, want[order]), (epoch, k)
            cw = [int((fid_h[want] >= l).sum()) for l in range(L)]
            assert counts_u.cpu().tolist()[:L] == cw and counts_o.cpu().tolist()[:L] == cw
            assert st_u.cpu().tolist() == [seed, epoch * nb + k + 1, 0] and st_o.cpu().tolist() == st_u.cpu().tolist()
            seen.append(so)
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N))      # every row exactly once per epoch


# ------------------------------------------------------------------ 6. the gather
@pytest.mark.parametrize("d", [1, 2, 8, 32])
def test_gather_is_bitwise(d):
    from mobocmf_amd import functional as F
    N, rows = 3001, 777
    g = torch.Generator().manual_seed(d)
    x = torch.randn(N, d, dtype=torch.float64, generator=g).to(DEV)
    y = torch.randn(N, 1, dtype=torch.float64, generator=g).to(DEV)
    fid = torch.tensor(_fid(N, 3), device=DEV)[:, None]
    src = torch.randperm(N, generator=g)[:rows].to(DEV)
    st = F.minibatch_state(5, DEV)
    xb = torch.full((rows, d), float("nan"), dtype=torch.float64, device=DEV)
    yb = torch.full((rows, 1), float("nan"), dtype=torch.float64, device=DEV)
    fb = torch.full((rows, 1), float("nan"), dtype=torch.float64, device=DEV)
    F.minibatch_gather(st, src, x, y, fid, xb, yb, fb)
    assert torch.equal(xb, x[src]) and torch.equal(yb, y[src]) and torch.equal(fb, fid[src])


# ------------------------------------------------------------------ 7. the guard
def test_wrong_rows_expected_sets_the_status_and_writes_nothing():
    """An argument check that returns a status: batch 2 of (N = 45, B = 16) has 13 rows; a caller built for 16 gets status 1,
    an untouched src / counts / step, nothing beyond its rows, and the gather that follows leaves the batch buffers alone."""
    from mobocmf_amd import functional as F
    N, B, L = 45, 16, 2
    fid = torch.tensor(_fid(N, L), device=DEV)[:, None]
    st = F.minibatch_state(9, DEV)
    counts = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    buf = torch.full((64,), -5, dtype=torch.int64, device=DEV)
    for _ in range(2):
        F.minibatch_indices(st, fid, B, L, buf[:16], counts)
    assert st.cpu().tolist() == [9, 2, 0]
    buf.fill_(-5)
    counts.fill_(-7)
    F.minibatch_indices(st, fid, B, L, buf[:16], counts)          # batch 2 has 13 rows
    assert st.cpu().tolist() == [9, 2, 1]
    assert bool((buf == -5).all()) and bool((counts == -7).all())
    x = torch.randn(N, 2, dtype=torch.float64, device=DEV)
    xb = torch.full((16, 2), 3.0, dtype=torch.float64, device=DEV)
    yb = torch.full((16, 1), 3.0, dtype=torch.float64, device=DEV)
    fb = torch.full((16, 1), 3.0, dtype=torch.float64, device=DEV)
    F.minibatch_gather(st, buf[:16], x, x[:, :1].contiguous(), fid, xb, yb, fb)
    assert bool((xb == 3.0).all()) and bool((yb == 3.0).all()) and bool((fb == 3.0).all())
    with pytest.raises(FloatingPointError, match="status = 1"):
        F.minibatch_check(st)
    # sticky: the right row count is refused too until the caller has dealt with it
    F.minibatch_indices(st, fid, B, L, buf[:13], counts)
    assert st.cpu().tolist() == [9, 2, 1] and bool((buf == -5).all())
    # a gather over never-written rows (src outside 0..N-1) skips them even with a clear status
    st2 = F.minibatch_state(9, DEV)
    F.minibatch_gather(st2, buf[:16], x, x[:, :1].contiguous(), fid, xb, yb, fb)
    assert bool((xb == 3.0).all())


def _problem(cfg):
    prob = synthetic.make_problem(**cfg)
    N = cfg["N"]
    perm = np.random.default_rng(3).permutation(N)      # fidelities interleaved, as any real data set's
    tc = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    return prob, tc(prob["x"])[perm], tc(prob["y"])[perm], tc(prob["fid"])[perm]


def _make_step(cfg, B, ordered, use_graph=True, seed=77, lr=1e-2):
    from mobocmf_amd import functional as F
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.graphed_step import GraphedMiniBatchStep
    prob, x, y, fid = _problem(cfg)
    S, L, N = cfg["S"], cfg["L"], cfg["N"]
    model = synthetic.model_from_problem(prob, num_samples_for_training=S, device=DEV)
    eps = [None] + [torch.as_tensor(e[:B * S].copy(), dtype=torch.float64) for e in prob["eps"][1:]]
    step = GraphedMiniBatchStep(model, VariationalELBOMF(model, N, L), x.to(DEV), y[:, None].to(DEV), fid[:, None].to(DEV), B,
                                lr=lr, use_graph=use_graph, fixed_eps=[None if e is None else e.to(DEV) for e in eps],
                                order_by_fidelity=ordered, sampler_state=F.minibatch_state(seed, DEV))
    return step, model, (x, y, fid, eps)


STEP_CASES = [("small2d", dict(d=2, L=2, M=8, N=45, S=3, seed=0), 16),
              ("three_fidelities", dict(d=3, L=3, M=10, N=45, S=2, seed=7), 16),
              ("C2_shaped", dict(d=2, L=2, M=128, N=512, S=8, seed=0), 192)]


# ------------------------------------------------------------------ 8. one step and the trajectory against the oracle
@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "unordered"])
@pytest.mark.parametrize("name,cfg,B", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_minibatch_step_and_trajectory_match_oracle(name, cfg, B, ordered):
    """Two epochs of the captured mini-batch step (both graphs: full and ragged batches).  After every step the oracle is
    evaluated on the rows the step reports (``step.src``) with num_data = N, (a) at the step's own pre-step parameters:
    -ELBO, scaled KL (1e-8) and every raw-parameter gradient (1e-5), the gates of test_hip_pruned_oracle; (b) along its own
    torch.optim.Adam trajectory: loss / KL of every step (1e-7) and the parameters at the end (1e-6) -- the C2-shaped case at
    that file's ill-conditioned trajectory gates, 1e-4 and 1e-3."""
    step, model, (x, y, fid, eps) = _make_step(cfg, B, ordered)
    S, L, N = cfg["S"], cfg["L"], cfg["N"]
    ill = name == "C2_shaped"
    nb = -(-N // B)
    assert step.nb == nb and len(step.shapes) == 2 and all(b.graph is not None for b in step.shapes)
    traj = _raw_from_model(model, L)
    opt = torch.optim.Adam(O.flatten_raw(traj), lr=1e-2)
    worst = dict(elbo=0.0, kl=0.0, grad=0.0, tl=0.0, tk=0.0)
    for it in range(2 * nb):
        raw = _raw_from_model(model, L)                  # the step's own parameters before it
        loss, kl = step.step()
        step.stream.synchronize()
        src = step.src.cpu()
        rows = src.numel()
        assert rows == (N - (nb - 1) * B if it % nb == nb - 1 else B)
        perm = host_perm(77, it // nb, N)[(it % nb) * B:(it % nb) * B + rows]
        assert np.array_equal(np.sort(src.numpy()), np.sort(perm))
        if not ordered:
            assert np.array_equal(src.numpy(), perm)         # the permutation's own order, bitwise
        if ordered:
            assert bool((fid[src][:-1] >= fid[src][1:]).all())
            assert step.counts.cpu().tolist()[:L] == [int((fid[src] >= l).sum()) for l in range(L)]
        e_b = [None if e is None else e[:rows * S] for e in eps]
        e_o, skl_o = O.elbo(O.state_from_raw(raw), x[src], y[src], fid[src], eps=e_b, S=S, num_data=N)
        (-e_o).backward()
        worst["elbo"] = max(worst["elbo"], rel(loss, -e_o))
        worst["kl"] = max(worst["kl"], rel(kl, skl_o))
        grads = dict(zip([id(p) for p in model.parameters()], step.grads))
        for l in range(L):
            for key, tt in raw["layers"][l].items():
                g = grads[id(_model_param_for(model, l, key))]
                gref = tt.grad if key != "L_S" else torch.tril(tt.grad)
                worst["grad"] = max(worst["grad"], rel(g.reshape(gref.shape), gref))
            g = grads[id(getattr(model, f"hidden_layer_likelihood_{l}").raw_noise)]
            worst["grad"] = max(worst["grad"], rel(g.reshape(()), raw["raw_noise"][l].grad))
        opt.zero_grad()
        e_t, skl_t = O.elbo(O.state_from_raw(traj), x[src], y[src], fid[src], eps=e_b, S=S, num_data=N)
        (-e_t).backward()
        opt.step()
        worst["tl"] = max(worst["tl"], rel(loss, -e_t))
        worst["tk"] = max(worst["tk"], rel(kl, skl_t))
    step.check()
    tp = 0.0
    for l in range(L):
        for key, tt in traj["layers"][l].items():
            tp = max(tp, rel(_model_param_for(model, l, key).reshape(tt.shape), tt.detach()))
        tp = max(tp, rel(getattr(model, f"hidden_layer_likelihood_{l}").raw_noise.reshape(()), traj["raw_noise"][l].detach()))
    print("%s ordered=%s: -ELBO %.2e, scaled KL %.2e, gradients %.2e | trajectory: loss %.2e, KL %.2e, parameters %.2e"
          % (name, ordered, worst["elbo"], worst["kl"], worst["grad"], worst["tl"], worst["tk"], tp))
    step.retire()
    assert worst["elbo"] < 1e-8 and worst["kl"] < 1e-8
    assert worst["grad"] < 1e-5
    assert worst["tl"] < (1e-4 if ill else 1e-7) and worst["tk"] < (1e-4 if ill else 1e-7)
    assert tp < (1e-3 if ill else 1e-6)


# ------------------------------------------------------------------ 9. captured against eager
def test_captured_replay_equals_the_eager_launches():
    """Same seed, same fixed eps: the same rows bitwise and -- the gate of test_graphed_step_equals_eager_step -- the same losses."""
    cfg, B = dict(d=3, L=2, M=20, N=60, S=2, seed=9), 25
    out = []
    for use_graph in (False, True):
        step, _, _ = _make_step(cfg, B, True, use_graph=use_graph)
        assert (step.graph is not None) == use_graph
        ls, srcs = [], []
        for _ in range(9):
            l, _ = step.step()
            step.stream.synchronize()
            ls.append(float(l))
            srcs.append(step.src.cpu().clone())
        step.check()
        out.append((ls, srcs, step.epoch_loss.item()))
        step.retire()
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    assert out[0][0] == out[1][0]
    assert out[0][2] == out[1][2] and np.isclose(out[0][2], sum(out[0][0][6:9]), rtol=1e-12)      # epoch 2's sum (3 batches / epoch)


# ------------------------------------------------------------------ 10. rollback
def test_rollback_replays_the_batches_drawn_after_the_snapshot():
    cfg, B = dict(d=3, L=2, M=20, N=60, S=2, seed=9), 25
    step, model, _ = _make_step(cfg, B, True)
    for _ in range(4):
        step.step()
    step.check()
    step.snapshot()
    params = [p.detach().clone() for p in model.parameters()]
    first = []
    for _ in range(5):
        l, _ = step.step()
        step.stream.synchronize()
        first.append((step.src.cpu().clone(), float(l)))
    step.restore_and_go_eager()
    step.stream.synchronize()
    assert step.graph is None and all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert step.state.cpu().tolist() == [77, 4, 0]
    for src, l in first:
        l2, _ = step.step()
        step.stream.synchronize()
        assert torch.equal(step.src.cpu(), src)
        # the eager redo runs with check_pd (host-checked Cholesky, same first jitter rung): the same arithmetic up to the order
        # of float64 roundings, amplified by cond(K_mm + 1e-6 I) <= ~1e7 here -- the well-conditioned trajectory gate, 1e-7
        assert abs(float(l2) - l) <= 1e-7 * abs(l)
    step.check()
    # a host / device disagreement about the step count is caught, not trained through
    step.state[1] += 2                                     # device: batch 2 of the epoch (10 rows); host: batch 0 (25 rows)
    torch.cuda.synchronize()
    step.step()
    with pytest.raises(FloatingPointError, match="mini-batch sampler"):
        step.check()
    step.retire()


# ------------------------------------------------------------------ 11. the fitter
def _toy_fitter(names, seeds, N=200, B=64, epochs=3):
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.random((N, 2)))
    fid = torch.tensor((np.arange(N) % 4 == 0).astype(np.float64))[:, None]
    fitter = BlackBoxMFDGPFitter(2, B, num_epochs_1=epochs, num_epochs_2=epochs, device=DEV, num_inducing=16)
    fitter.verbose = False
    for name, seed in zip(names, seeds):
        k = int(name[-1])
        y = torch.sin(3.0 * x[:, :1] + k) + 0.3 * (k + 1) * x[:, 1:] * fid
        fitter.initialize_mfdgp(x, y, fid, name, is_constraint=(k == 2))
    for (_, _, h), seed in zip(fitter._handlers(), seeds):
        h.minibatch_seed = seed
    return fitter


def _train_recording(fitter, monkeypatch):
    """train_mfdgps() with every GraphedMiniBatchStep.step() followed by (on the step's stream) a histogram update and a copy of
    the rows it drew: {seed: (hist [N] on the device, [src, ...], [loss, ...])}."""
    from mobocmf_amd.util import graphed_step
    rec = {}
    orig = graphed_step.GraphedMiniBatchStep.step

    def step(self):
        out = orig(self)
        with torch.cuda.stream(self.stream):
            seed = self._test_seed = getattr(self, "_test_seed", None) or int(self.state[0])
            hist, srcs, losses = rec.setdefault(seed, (torch.zeros(self.num_data, dtype=torch.int64, device=DEV), [], []))
            hist.index_add_(0, self.src, torch.ones_like(self.src))
            srcs.append(self.src.clone())
            losses.append(self.loss.clone())
        return out

    monkeypatch.setattr(graphed_step.GraphedMiniBatchStep, "step", step)
    fitter.train_mfdgps()
    torch.cuda.synchronize()
    monkeypatch.setattr(graphed_step.GraphedMiniBatchStep, "step", orig)
    return rec


def test_fitter_trains_on_captured_minibatches(monkeypatch):
    """batch_size < N: train_mfdgps() takes the captured mini-batch path by default (and with use_graphs=True, which used to
    raise); every row is visited exactly once per epoch; three surrogates in lockstep draw what each draws alone."""
    from mobocmf_amd.util import graphed_step
    names, seeds = ["obj0", "obj1", "con2"], [101, 202, 303]
    fitter = _toy_fitter(names, seeds)
    made = []
    orig_init = graphed_step.GraphedMiniBatchStep.__init__

    def init(self, *a, **kw):
        orig_init(self, *a, **kw)
        made.append(self)

    monkeypatch.setattr(graphed_step.GraphedMiniBatchStep, "__init__", init)
    rec = _train_recording(fitter, monkeypatch)
    assert len(made) == 6 and all(len(g.shapes) == 2 and g.use_graph for g in made)      # 3 surrogates x 2 phases, captured
    assert fitter.models_uncond_trained and sorted(rec) == seeds
    for seed in seeds:
        hist, srcs, losses = rec[seed]
        assert len(srcs) == 2 * 3 * 4                                  # two phases x 3 epochs x ceil(200 / 64) steps
        assert bool((hist == 6).all())                                 # every row once per epoch
        assert bool(torch.isfinite(torch.stack(losses)).all())
        for e in range(6):                                             # the state carries over from phase 1 to phase 2
            got = torch.cat(srcs[4 * e:4 * e + 4]).cpu().numpy()
            assert np.array_equal(np.sort(got), np.arange(200))
            want = host_perm(seed, e, 200)
            assert all(np.array_equal(np.sort(srcs[4 * e + k].cpu().numpy()), np.sort(want[64 * k:64 * k + 64])) for k in range(4))
    for name, seed in zip(names, seeds):                               # each surrogate alone: the same rows at every step
        solo = _toy_fitter([name], [seed])
        rec1 = _train_recording(solo, monkeypatch)
        assert list(rec1) == [seed]
        assert all(torch.equal(a, b) for a, b in zip(rec1[seed][1], rec[seed][1]))
    fitter.num_epochs_1 = fitter.num_epochs_2 = 1
    before = len(made)
    fitter.train_mfdgps(use_graphs=True)                               # no longer refused
    assert len(made) == before + 6


def test_fitter_redoes_the_epochs_since_the_last_verdict_after_a_failed_one(monkeypatch):
    """A verdict that fails on the captured mini-batch path (injected on the host: nothing is faulted on the device) rolls the
    surrogate back to the last verified epoch, sampler included, and the phase finishes eagerly with every step counted once."""
    import warnings
    from mobocmf_amd.layers.mfdgp_hidden_layer import NotPSDError
    from mobocmf_amd.util import blackbox_mfdgp_fitter as BF
    from mobocmf_amd.util import graphed_step
    monkeypatch.setattr(BF, "ITER_PRINT", 3)
    epochs = 7
    fitter = _toy_fitter(["obj0"], [55], epochs=epochs)
    calls = {"n": 0}
    real_check = graphed_step.GraphedMiniBatchStep.check

    def failing_check(self):
        calls["n"] += 1
        if calls["n"] == 2:      # the verdict at epoch 3 (epoch 0 passed)
            raise NotPSDError("injected")
        return real_check(self)

    monkeypatch.setattr(graphed_step.GraphedMiniBatchStep, "check", failing_check)
    made = []
    real_init = graphed_step.GraphedMiniBatchStep.__init__
    monkeypatch.setattr(graphed_step.GraphedMiniBatchStep, "__init__", lambda self, *a, **k: (real_init(self, *a, **k), made.append(self))[0])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fitter._train_mfdgp_minibatch(True, epochs, 3e-3)
    assert any("rolling back 3 epochs and redoing them eagerly" in str(m.message) for m in w)
    g, = made
    assert g.nb == 4 and calls["n"] == 4                      # verdicts at epochs 0, 3 (failed), 3 again after the redo, 6 (the last)
    assert int(g.optimizer.steps_done) == epochs * g.nb
    assert g.state.cpu().tolist() == [55, epochs * g.nb, 0]   # the sampler went back with the parameters
    for p in fitter.get_model("obj0").parameters():
        assert bool(torch.isfinite(p).all())


def test_fitter_keeps_the_full_batch_path_when_the_batch_covers_the_data(monkeypatch):
    from mobocmf_amd.util import graphed_step
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    called = []
    monkeypatch.setattr(BlackBoxMFDGPFitter, "_train_mfdgp_minibatch", lambda self, *a: called.append("mini"))
    orig = BlackBoxMFDGPFitter._train_mfdgp_graphed
    monkeypatch.setattr(BlackBoxMFDGPFitter, "_train_mfdgp_graphed", lambda self, *a: (called.append("full"), orig(self, *a))[1])
    fitter = _toy_fitter(["obj0"], [1], N=40, B=40, epochs=2)
    fitter.train_mfdgps()
    assert called == ["full", "full"]
    del graphed_step
