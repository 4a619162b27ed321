"""CPU: the float criterion of tests/_sensitivity.py (check_float) on oracle outputs alone -- no device involved.

check_float holds a float frame to the contract's 1e-4 and accepts a sample beyond that only near pixels where the
oracle itself moves under float32-level jitter.  These tests show that it catches what the float assertion used before it let through
(a 2e-4 bias on 1 % of stable pixels), that it accepts deviations confined to the pixels the probe marks unstable, and that it rejects a NaN."""
import numpy as np
import pytest

from _sensitivity import _dilate, check_float

H, W = 96, 128


@pytest.fixture(scope="module")
def hummingbird():
    """hummingbird.py's x / (x + y + z + 1e-8) cancellation makes its float output unstable at some pixels of a structured frame."""
    from animal_vision_amd.animals import Hummingbird
    from animal_vision_amd.synthetic import structured_frame
    from oracle import np_backend

    sp = Hummingbird()
    frame = structured_frame(1, H, W).astype(np.float32) / 255.0
    _, want = np_backend.run(sp, frame)
    runs = {k: np_backend.run_jittered(sp, frame, k)[1] for k in list(range(6)) + [6]}
    moved = np.zeros((H, W))
    for k in range(6):
        moved = np.maximum(moved, np.abs(runs[k].astype(np.float64) - want.astype(np.float64)).max(axis=2))
    unstable, stable = moved > 1e-4, ~_dilate(moved > 2.5e-5, 3)  # check_float's tol and probe_tol
    assert want.dtype == np.float32 and want.shape == (H, W, 3)
    assert unstable.any() and stable.mean() > 0.5, "the frame no longer has both stable and unstable pixels"
    return want, runs.__getitem__, unstable, stable


def _old_float_assertion(got, want):
    """The criterion of test_species_float_frames_vs_oracle / test_mantis_float_frames_vs_oracle."""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return float((d > 4e-3).mean()) <= 2e-3 and float(np.median(d)) < 1e-5


def test_oracle_against_itself_passes(hummingbird):
    want, rerun, _, _ = hummingbird
    st = check_float(want.copy(), want, "identity", rerun)
    assert st["outlier_px"] == 0 and st["max"] == 0.0


def test_a_seventh_jittered_run_passes(hummingbird):
    """A second correct float32 evaluation (one more jittered oracle run, not among the probe's six) meets the criterion."""
    want, rerun, unstable, _ = hummingbird
    st = check_float(rerun(6), want, "seventh run", rerun)
    assert st["outlier_px"] > 0 and st["unexplained_px"] == 0


def test_bias_on_one_percent_of_stable_pixels_fails(hummingbird):
    want, rerun, _, stable = hummingbird
    ys, xs = np.nonzero(stable)
    pick = np.random.default_rng(0).choice(ys.size, size=H * W // 100, replace=False)
    got = want.copy()
    sign = np.where(want[ys[pick], xs[pick], 1] > 0.5, -1.0, 1.0).astype(np.float32)
    got[ys[pick], xs[pick], 1] += sign * np.float32(2e-4)
    assert _old_float_assertion(got, want), "the old float assertion was expected to accept this bias"
    with pytest.raises(AssertionError, match="stable under float32-level jitter"):
        check_float(got, want, "biased", rerun)


def test_deviations_only_at_unstable_pixels_pass(hummingbird):
    want, rerun, unstable, _ = hummingbird
    got = want.copy()
    got[unstable] = np.clip(want[unstable] + np.float32(0.05), 0.0, 1.0)
    st = check_float(got, want, "unstable only", rerun)
    assert 0 < st["outlier_px"] <= st["unstable_px"] == int(unstable.sum()) and st["unexplained_px"] == 0
    assert st["max_stable"] <= 1e-4


def test_deviation_one_pixel_outside_the_dilated_mask_fails(hummingbird):
    want, rerun, unstable, stable = hummingbird
    ys, xs = np.nonzero(stable)
    got = want.copy()
    got[unstable] = np.clip(want[unstable] + np.float32(0.05), 0.0, 1.0)
    got[ys[0], xs[0], 0] = want[ys[0], xs[0], 0] + np.float32(-3e-4 if want[ys[0], xs[0], 0] > 0.5 else 3e-4)
    with pytest.raises(AssertionError, match="stable under float32-level jitter"):
        check_float(got, want, "one stray pixel", rerun)


def test_more_outliers_than_unstable_pixels_fails():
    """Outliers inside the dilated mask but more of them than the probe marks unstable: over the cap."""
    want = np.full((32, 32, 3), 0.5, np.float32)
    moved = want.copy()
    moved[16, 16, 0] += np.float32(0.01)
    got = want.copy()
    got[15:18, 15:18, 0] += np.float32(0.01)
    with pytest.raises(AssertionError, match="more outlier pixels"):
        check_float(got, want, "over the cap", lambda seed: moved)


def test_nan_fails(hummingbird):
    want, rerun, _, _ = hummingbird
    got = want.copy()
    got[H // 2, W // 3, 2] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_float(got, want, "nan", rerun)
    got = want.copy()
    got[0, 0, 0] = np.inf
    with pytest.raises(AssertionError, match="non-finite"):
        check_float(got, want, "inf", rerun)


def test_outliers_without_a_probe_fail():
    want = np.full((8, 8, 3), 0.25, np.float32)
    got = want.copy()
    got[3, 3, 1] += np.float32(2e-4)
    with pytest.raises(AssertionError, match="no sensitivity probe"):
        check_float(got, want, "no probe")
    got[3, 3, 1] = want[3, 3, 1] + np.float32(5e-5)
    assert check_float(got, want, "within tol")["outlier_px"] == 0
