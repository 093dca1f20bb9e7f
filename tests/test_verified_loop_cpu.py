"""run_verified (util/blackbox_mfdgp_fitter.py), the one training loop of the captured and one-launch paths, on stub step
objects that record every call and raise from chosen check() calls: no GPU, no kernels."""
import warnings

import pytest

from mobocmf_amd.layers.mfdgp_hidden_layer import NotPSDError
from mobocmf_amd.util import blackbox_mfdgp_fitter as BF


class Stub:
    """The protocol run_verified is written against.  ``fail_at``: the 1-based check() calls that raise."""

    def __init__(self, name, log, nb=None, fail_at=(), error=NotPSDError):
        self.name, self.log, self.fail_at, self.error = name, log, set(fail_at), error
        self.checks = 0
        if nb is not None:
            self.nb = nb

    def _say(self, what):
        self.log.append((self.name, what))

    def step(self):
        self._say("step")

    def check(self):
        self.checks += 1
        self._say("check")
        if self.checks in self.fail_at:
            raise self.error("injected at check %d" % self.checks)

    def snapshot(self):
        self._say("snapshot")

    def restore_and_go_eager(self):
        self._say("restore_and_go_eager")

    def restore(self):
        self._say("restore")

    def close(self):
        self._say("close")


def calls(log, name):
    return [what for who, what in log if who == name]


def verified_iterations(log, name, nb=1):
    """Iterations (0-based) after which ``name`` was checked: the number of its steps before each check, over nb, minus 1."""
    out, steps = [], 0
    for what in calls(log, name):
        steps += what == "step"
        if what == "check":
            out.append(steps // nb - 1)
    return out


@pytest.fixture(autouse=True)
def every_four(monkeypatch):
    monkeypatch.setattr(BF, "ITER_PRINT", 4)


def test_the_schedule_verifies_every_iter_print_iterations_and_the_last_one():
    log = []
    g = Stub("a", log)
    seen = []
    out = BF.run_verified([g], 10, BF.REDO_EAGERLY, ["a: "], "epochs", lambda i, j, s: seen.append((i, j, s)))
    assert out == (10, None)
    assert verified_iterations(log, "a") == [0, 4, 8, 9]
    assert seen == [(0, 0, g), (4, 0, g), (8, 0, g), (9, 0, g)]                    # reported where verified
    # one snapshot before the first step, then check -> snapshot at every verification; closed once, last
    assert calls(log, "a")[:4] == ["snapshot", "step", "check", "snapshot"]
    assert calls(log, "a").count("snapshot") == 5 and calls(log, "a").count("step") == 10
    assert calls(log, "a").count("close") == 1 and calls(log, "a")[-1] == "close"


def test_iter_print_is_read_when_the_loop_runs(monkeypatch):
    log = []
    monkeypatch.setattr(BF, "ITER_PRINT", 3)
    BF.run_verified([Stub("a", log)], 7, BF.REDO_EAGERLY, [""], "epochs")
    assert verified_iterations(log, "a") == [0, 3, 6]                              # 6 is also the last


def test_surrogates_with_unequal_nb_advance_in_lockstep():
    log = []
    a, b, c = Stub("a", log, nb=3), Stub("b", log, nb=1), Stub("c", log)          # c has no nb: one step per iteration
    BF.run_verified([a, b, c], 2, BF.REDO_EAGERLY, ["", "", ""], "epochs")
    epoch = ["a", "b", "c", "a", "a"]                                              # k = 0: all three; k = 1, 2: a alone
    verdicts = [(n, w) for n in "abc" for w in ("check", "snapshot")]
    want = [(n, "snapshot") for n in "abc"] + [(n, "step") for n in epoch] + verdicts + [(n, "step") for n in epoch] + verdicts + \
        [(n, "close") for n in "abc"]
    assert log == want


def test_a_failed_verdict_is_rolled_back_and_redone_eagerly_by_that_surrogate_alone():
    log = []
    a, b = Stub("a", log, nb=2), Stub("b", log, nb=3, fail_at=[3])                 # b's third check is the one at iteration 8
    seen = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = BF.run_verified([a, b], 10, BF.REDO_EAGERLY, ["OBJ 0: ", "OBJ 1: "], "epochs", lambda i, j, s: seen.append((i, j)))
    assert out == (10, None)
    assert [str(m.message) for m in w] == ["OBJ 1: injected at check 3 -- rolling back 4 epochs and redoing them eagerly"]
    cb = calls(log, "b")
    at = cb.index("restore_and_go_eager")
    assert cb.count("restore_and_go_eager") == 1 and cb[at - 1] == "check"
    # (i - last_good) * nb = (8 - 4) * 3 steps of b, then its check and snapshot; nobody else moves meanwhile
    assert cb[at + 1:at + 15] == ["step"] * 12 + ["check", "snapshot"]
    start = log.index(("b", "restore_and_go_eager"))
    assert log[start:start + 15] == [("b", w) for w in ["restore_and_go_eager"] + ["step"] * 12 + ["check", "snapshot"]]
    assert calls(log, "a").count("step") == 10 * 2 and "restore_and_go_eager" not in calls(log, "a")
    assert cb.count("step") == 10 * 3 + 12
    assert seen == [(i, j) for i in (0, 4, 8, 9) for j in (0, 1)]                  # b is reported after its redo, too
    assert verified_iterations(log, "a", 2) == [0, 4, 8, 9]
    assert cb.count("close") == 1 and calls(log, "a").count("close") == 1


def test_the_redo_counts_from_the_last_verified_iteration_of_that_surrogate():
    log = []
    g = Stub("a", log, fail_at=[1], error=FloatingPointError)                      # nothing verified yet: last_good = -1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        BF.run_verified([g], 1, BF.REDO_EAGERLY, ["conditioned training: "], "iterations")
    assert [str(m.message) for m in w] == \
        ["conditioned training: injected at check 1 -- rolling back 1 iterations and redoing them eagerly"]
    assert calls(log, "a") == ["snapshot", "step", "check", "restore_and_go_eager", "step", "check", "snapshot", "close"]


def test_hand_over_restores_and_returns_what_stands_without_another_step():
    log = []
    g = Stub("group", log, fail_at=[3])                                             # verified at 0 and 4, fails at 8
    seen = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = BF.run_verified([g], 10, BF.HAND_OVER, [""], "epochs", lambda i, j, s: seen.append(i))
    assert out == (5, g)                                                            # last_good + 1 iterations stand
    assert [str(m.message) for m in w] == ["injected at check 3 -- rolling back 4 epochs; the layer path continues"]
    c = calls(log, "group")
    assert c.count("step") == 9 and c[-3:] == ["check", "restore", "close"]         # no step, check or snapshot after restore()
    assert "restore_and_go_eager" not in c and seen == [0, 4]


def test_hand_over_that_never_fails_completes_and_closes():
    log = []
    g = Stub("group", log)
    assert BF.run_verified([g], 5, BF.HAND_OVER, [""], "iterations") == (5, None)
    assert calls(log, "group").count("close") == 1 and "restore" not in calls(log, "group")


def test_an_error_from_the_check_after_the_redo_propagates():
    log = []
    g = Stub("a", log, fail_at=[2, 3])                                              # the verdict at 4 and the one after its redo
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotPSDError, match="injected at check 3"):
            BF.run_verified([g], 10, BF.REDO_EAGERLY, [""], "epochs")
    c = calls(log, "a")
    assert c[-6:] == ["restore_and_go_eager", "step", "step", "step", "step", "check"]


def test_other_exceptions_from_check_are_not_caught():
    log = []
    with pytest.raises(RuntimeError):
        BF.run_verified([Stub("a", log, fail_at=[1], error=RuntimeError)], 3, BF.REDO_EAGERLY, [""], "epochs")
    assert "restore_and_go_eager" not in calls(log, "a")


def test_no_iterations_still_snapshots_and_closes():
    log = []
    assert BF.run_verified([Stub("a", log)], 0, BF.HAND_OVER, [""], "epochs") == (0, None)
    assert calls(log, "a") == ["snapshot", "close"]
