"""The jitter-retry policy (gp-plus_amd/psd_safe.py) on the host alone: fake ``attempt`` closures and a stub context, no GPU and no
library.  What is pinned: the schedule, the one warning, the NaN probe's place, the NotPSDError's text, and that a time-out status
repeats the attempt without consuming its jitter."""
import warnings

import pytest

from gpplus_amd import settings
from gpplus_amd._lib import GppError
from gpplus_amd.backend import INFO_EXEC_TIMEOUT, INFO_PANEL_TIMEOUT, OPT_COOP_PANEL, OPT_DAG_SCHED
from gpplus_amd.errors import NanError, NotPSDError
from gpplus_amd.psd_safe import jitter_schedule, psd_safe


class StubContext:
    """What ``backend.panel_timed_out`` touches of a GppContext."""

    def __init__(self, coop_panel=True, dag_sched=True):
        self.coop_panel, self.dag_sched = coop_panel, dag_sched
        self.options = []

    def set_option(self, option, value):
        self.options.append((option, value))
        if option == OPT_COOP_PANEL:
            self.coop_panel = bool(value)
        elif option == OPT_DAG_SCHED:
            self.dag_sched = bool(value)


class Attempts:
    """An ``attempt`` that answers with the given status words in turn (the last one for ever) and records its jitters."""

    def __init__(self, *statuses):
        self.statuses, self.jitters = list(statuses), []

    def __call__(self, jitter):
        self.jitters.append(jitter)
        return self.statuses.pop(0) if len(self.statuses) > 1 else self.statuses[0]


class Probe:
    def __init__(self, attempts, error=None):
        self.attempts, self.error, self.seen = attempts, error, []

    def __call__(self):
        self.seen.append(list(self.attempts.jitters))  # what had been attempted when the probe ran
        if self.error is not None:
            raise self.error


def test_schedule_follows_the_settings():
    assert jitter_schedule() == [0.0, 1e-8, 1e-8 * 10, 1e-8 * 100]
    with settings.cholesky_jitter(1e-6), settings.cholesky_max_tries(2):
        assert jitter_schedule() == [0.0, 1e-6, 1e-6 * 10]
    with settings.cholesky_max_tries(0):
        assert jitter_schedule() == [0.0]


def test_first_attempt_succeeds():
    attempt = Attempts(0)
    probe = Probe(attempt)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert psd_safe(StubContext(), attempt, probe) == 0.0
    assert attempt.jitters == [0.0] and probe.seen == []


def test_third_attempt_succeeds_with_one_warning():
    attempt = Attempts(5, 5, 0)
    probe = Probe(attempt)
    with pytest.warns(RuntimeWarning) as rec:
        used = psd_safe(StubContext(), attempt, probe)
    assert used == jitter_schedule()[2] and abs(used - 1e-7) < 1e-20
    assert attempt.jitters == jitter_schedule()[:3]
    assert len(rec) == 1 and "added jitter of 1.0e-07 to the diagonal" in str(rec[0].message)
    assert probe.seen == [[0.0]]  # once, after the failure without jitter and before the next attempt


def test_exhausted_schedule_raises_with_jitter_and_minor():
    attempt = Attempts(251)
    with pytest.raises(NotPSDError) as err:
        psd_safe(StubContext(), attempt)
    assert "1.0e-06" in str(err.value) and "251" in str(err.value)
    assert len(attempt.jitters) == 4
    attempt = Attempts(251)
    with settings.cholesky_jitter(1e-5), settings.cholesky_max_tries(5), pytest.raises(NotPSDError) as err:
        psd_safe(StubContext(), attempt)
    assert len(attempt.jitters) == 6 and attempt.jitters[1] == 1e-5
    assert "1.0e-01" in str(err.value) and "251" in str(err.value)


def test_nan_probe_propagates_after_one_attempt():
    attempt = Attempts(1)
    with pytest.raises(NanError, match="weights"):
        psd_safe(StubContext(), attempt, Probe(attempt, NanError("cholesky: NaN/Inf in weights of the covariance")))
    assert attempt.jitters == [0.0]


@pytest.mark.parametrize("status, option, what", [(INFO_PANEL_TIMEOUT | 17, OPT_COOP_PANEL, "cooperative panel"),
                                                  (INFO_EXEC_TIMEOUT | 17, OPT_DAG_SCHED, "executor")])
def test_timeout_repeats_the_same_jitter(status, option, what):
    ctx = StubContext()
    attempt = Attempts(status, 0)
    with pytest.warns(RuntimeWarning) as rec:
        assert psd_safe(ctx, attempt) == 0.0
    assert attempt.jitters == [0.0, 0.0]
    assert ctx.options == [(option, 0)]
    assert len(rec) == 1 and what in str(rec[0].message) and "timed out after 17 ms" in str(rec[0].message)
    # and with jitter: the time-out does not consume the attempt
    ctx, attempt = StubContext(), Attempts(3, status, 3, 0)
    with pytest.warns(RuntimeWarning) as rec:
        used = psd_safe(ctx, attempt)
    s = jitter_schedule()
    assert attempt.jitters == [s[0], s[1], s[1], s[2]] and used == s[2]
    assert len(rec) == 2  # the time-out's and the jitter's


@pytest.mark.parametrize("status, ctx", [(INFO_PANEL_TIMEOUT | 17, StubContext(coop_panel=False)),
                                         (INFO_EXEC_TIMEOUT | 17, StubContext(dag_sched=False))])
def test_timeout_with_nothing_left_to_switch_off_raises(status, ctx):
    attempt = Attempts(status)
    with pytest.raises(GppError, match="timed out"):
        psd_safe(ctx, attempt)
    assert attempt.jitters == [0.0] and ctx.options == []


def test_custom_timeout_handler_replaces_the_default():
    ctx = StubContext()
    calls = []

    def handler(c, info):
        calls.append((c, info))
        raise KeyError("mine")

    attempt = Attempts(INFO_PANEL_TIMEOUT | 17)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the default would warn
        with pytest.raises(KeyError):
            psd_safe(ctx, attempt, on_timeout=handler)
    assert calls == [(ctx, INFO_PANEL_TIMEOUT | 17)] and ctx.options == [] and attempt.jitters == [0.0]
