"""Shared criterion for the float32 UV pipelines whose last step is a uint8 encode (tests/test_uv_species_gpu.py,
tests/test_mantis_gpu.py, bench.py's parity_checked).

Contract: the baseline is bit-exact; the stylised frame is a float32 pipeline held to 1e-4
relative before the encode, i.e. codes within +-1 of the oracle's.  A sample further off than that is accepted ONLY where
the oracle's own arithmetic is unstable at float32 rounding level -- a categorical decision (mask, argmax, floor) within
rounding of its boundary, or a cancellation such as hummingbird.py:178-185's x / (x + y + z + 1e-8) with every term
at 1e-8.  That is established per frame, not assumed: the oracle is re-run `runs` times with every stage result,
reduction and transcendental jittered by a relative 2^-20 (oracle/np_backend.JitterBackend); the pixels whose output
code moves by >= 2 under that jitter, dilated by `dilate` pixels (a flipped pixel leaks into its neighbours through
the blurs that follow), are the only places where an outlier may sit.  On top of that the number of outlier pixels per
frame is capped in absolute terms."""
import numpy as np


def _dilate(mask: np.ndarray, r: int) -> np.ndarray:
    if r <= 0 or not mask.any():
        return mask
    out = mask.copy()
    for _ in range(r):  # r steps of the 3x3 structuring element
        m = out.copy()
        m[1:, :] |= out[:-1, :]
        m[:-1, :] |= out[1:, :]
        out = m.copy()
        m[:, 1:] |= out[:, :-1]
        m[:, :-1] |= out[:, 1:]
        out = m
    return out


def outlier_stats(got: np.ndarray, want: np.ndarray, rerun_jittered=None, *, runs: int = 6, dilate: int = 3) -> dict:
    """rerun_jittered(seed) -> the oracle's uint8 output under jitter (same shape as `want`)."""
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    px = diff.max(axis=2) if diff.ndim == 3 else diff
    out_px = px > 1
    st = {"frac_gt1": float((diff > 1).mean()), "frac_ne": float((diff > 0).mean()), "max": int(diff.max()), "outlier_px": int(out_px.sum()),
          "pixels": int(px.size)}
    if st["outlier_px"] and rerun_jittered is not None:
        unstable = np.zeros(px.shape, bool)
        for k in range(runs):
            j = rerun_jittered(k)
            dj = np.abs(j.astype(np.int16) - want.astype(np.int16))
            unstable |= (dj.max(axis=2) if dj.ndim == 3 else dj) >= 2
        cover = _dilate(unstable, dilate)
        st["unstable_px"] = int(unstable.sum())
        st["unexplained_px"] = int((out_px & ~cover).sum())
        if st["unexplained_px"]:
            ys, xs = np.nonzero(out_px & ~cover)
            st["unexplained_at"] = [(int(y), int(x), int(px[y, x])) for y, x in list(zip(ys, xs))[:8]]
    return st


def check_codes(got, want, what, rerun_jittered=None, *, frac_any: float = 0.05, frac_beyond: float = 2e-3, px_cap_abs: int = 16, px_cap_rel: float = 1e-3,
                runs: int = 6, dilate: int = 3):
    st = outlier_stats(got, want, rerun_jittered, runs=runs, dilate=dilate)
    assert st["frac_ne"] <= frac_any, (what, "fraction of samples != oracle:", st)
    assert st["frac_gt1"] <= frac_beyond, (what, "fraction of samples beyond +-1:", st)
    assert st["outlier_px"] <= px_cap_abs + px_cap_rel * st["pixels"], (what, "outlier pixels over the absolute cap:", st)
    if st["outlier_px"]:
        assert rerun_jittered is not None, (what, "samples beyond +-1 and no sensitivity probe given:", st)
        assert st["unexplained_px"] == 0, (what, "samples beyond +-1 where the oracle is stable under float32-level jitter:", st)
    return st



def check_float(got, want, what, rerun_jittered=None, *, tol: float = 1e-4, probe_tol: float = 2.5e-5, runs: int = 6, dilate: int = 3):
    """The float contract itself, for stylised frames in [0, 1] (float inputs: from_float01 hands the encode's [0, 1] result back as is, so an
    absolute `tol` is the contract's 1e-4 relative to full scale).

    Every sample must be finite.  A sample further than `tol` from the oracle is an outlier.  The oracle is re-run `runs` times under the 2^-20
    jitter of outlier_stats (rerun_jittered(seed) -> its float output), only when there are outliers.  Outliers may sit only inside the mask of
    pixels that the jitter moves by more than `probe_tol`, dilated by `dilate` pixels, and there may be no more outlier pixels than the jitter
    moves by more than `tol` (`unstable_px`): the device must not reach further than a second correct float32 evaluation does.
    probe_tol = tol / 4 because six random draws under-sample a pixel's sensitivity: on structured_frame(1, 1080, 1920) / 255, a seventh
    jittered oracle run put 415-465 hummingbird pixels beyond 1e-4 outside the mask taken at 1e-4, 4-7 outside the mask at 1e-4 / 2, none at
    1e-4 / 4.  Returns the statistics (max_stable: the largest deviation outside the dilated mask)."""
    got64, want64 = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got64.shape == want64.shape, (what, got64.shape, want64.shape)
    assert np.isfinite(got64).all(), (what, "non-finite samples:", int((~np.isfinite(got64)).sum()))
    assert np.isfinite(want64).all(), (what, "the oracle's output is not finite")
    diff = np.abs(got64 - want64)
    px = diff.max(axis=2) if diff.ndim == 3 else diff
    out_px = px > tol
    st = {"max": float(diff.max()), "outlier_px": int(out_px.sum()), "unstable_px": 0, "unexplained_px": 0, "max_stable": float(px.max()),
          "pixels": int(px.size)}
    if st["outlier_px"]:
        assert rerun_jittered is not None, (what, "samples beyond tol and no sensitivity probe given:", st)
        moved = np.zeros(px.shape)
        for k in range(runs):
            dj = np.abs(np.asarray(rerun_jittered(k), np.float64) - want64)
            moved = np.maximum(moved, dj.max(axis=2) if dj.ndim == 3 else dj)
        cover = _dilate(moved > probe_tol, dilate)
        st["unstable_px"] = int((moved > tol).sum())
        st["unexplained_px"] = int((out_px & ~cover).sum())
        st["max_stable"] = float(px[~cover].max()) if (~cover).any() else 0.0
        if st["unexplained_px"]:
            ys, xs = np.nonzero(out_px & ~cover)
            st["unexplained_at"] = [(int(y), int(x), float(px[y, x])) for y, x in list(zip(ys, xs))[:8]]
    assert st["unexplained_px"] == 0, (what, "samples beyond tol where the oracle is stable under float32-level jitter:", st)
    assert st["outlier_px"] <= st["unstable_px"], (what, "more outlier pixels than the jitter moves beyond tol:", st)
    return st
