"""The per-element jitter policy of the batched evaluations (``psd_safe.psd_safe_batched``) on the host alone: fake attempts on CPU
tensors, no GPU and no library.  What is pinned: the (B, 1) jitters each attempt is handed, that a passed element keeps the jitter
it passed with while a failing one takes the schedule's next, the stop rule, the returned mask and that nothing warns or raises."""
import warnings

import pytest
import torch

from gpplus_amd import settings
from gpplus_amd.psd_safe import jitter_schedule, psd_safe_batched


class Attempts:
    """An ``attempt`` for B elements: element b fails (status b + 1, a leading minor) until the jitter it is handed reaches
    ``needs[b]`` (None: it never passes); records a copy of every ``extra`` it was handed."""

    def __init__(self, needs):
        self.needs, self.extras = needs, []

    def __call__(self, extra):
        assert extra.shape == (len(self.needs), 1) and extra.dtype == torch.float64 and extra.device.type == "cpu"
        self.extras.append(extra.reshape(-1).tolist())
        info = torch.tensor([0 if n is not None and e >= n else b + 1 for b, (n, e) in enumerate(zip(self.needs, self.extras[-1]))],
                            dtype=torch.int32)
        return info == 0, info.clone()


@pytest.fixture(autouse=True)
def _no_warnings():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        yield


def test_all_pass_at_once():
    attempt = Attempts([0.0] * 3)
    ok, info = psd_safe_batched(3, "cpu", attempt)
    assert attempt.extras == [[0.0, 0.0, 0.0]]
    assert ok.tolist() == [True] * 3 and info.tolist() == [0] * 3


def test_one_element_passes_with_jitter_and_one_never():
    j0, j1, j2 = jitter_schedule()[1:]
    attempt = Attempts([0.0, j0, 0.0, None])
    ok, info = psd_safe_batched(4, "cpu", attempt)
    # element 1 keeps the jitter it passed with; element 3 walks the whole schedule; the others never get any
    assert attempt.extras == [[0.0, 0.0, 0.0, 0.0], [0.0, j0, 0.0, j0], [0.0, j0, 0.0, j1], [0.0, j0, 0.0, j2]]
    assert ok.dtype == torch.bool and ok.tolist() == [True, True, True, False]
    assert info.tolist() == [0, 0, 0, 4]  # the host words of the last attempt


def test_stops_as_soon_as_every_element_passes():
    j0, j1, _ = jitter_schedule()[1:]
    attempt = Attempts([j1, 0.0])
    ok, _ = psd_safe_batched(2, "cpu", attempt)
    assert attempt.extras == [[0.0, 0.0], [j0, 0.0], [j1, 0.0]]
    assert ok.tolist() == [True, True]


def test_no_retries_means_one_attempt():
    attempt = Attempts([None, 0.0])
    with settings.cholesky_max_tries(0):
        ok, info = psd_safe_batched(2, "cpu", attempt)
    assert attempt.extras == [[0.0, 0.0]]
    assert ok.tolist() == [False, True] and info.tolist() == [1, 0]


def test_the_jitter_follows_the_settings():
    attempt = Attempts([None])
    with settings.cholesky_jitter(1e-5), settings.cholesky_max_tries(2):
        ok, _ = psd_safe_batched(1, "cpu", attempt)
    assert attempt.extras == [[0.0], [1e-5], [1e-5 * 10]]
    assert ok.tolist() == [False]
