"""CPU: the oracle's OpenCV restatements (oracle/cvref.cpp) against float64 statements of the definitions (tests/_geom_ref.py).

The kernels of csrc/geom.hip are held bit-equal to cvref.cpp, which was written from the same reading of OpenCV as they were; this
module anchors that checker to the mathematics, so that a misreading shared by both (a half-pixel shift, a wrong Keys `a`,
replicate instead of reflect, a wrong clamp: each >= 1e-2 on noise) does not pass.  Bounds are derived, not fitted; N is the
largest of H, W, Hd, Wd of a case:

  NEAREST            equal
  LINEAR             2 N 2^-23 + 2^-20   the source coordinate is rounded to float32: the weight is off by at most ulp(coordinate)
  CUBIC              twice LINEAR's      (|d keys / dt| <= 2 per tap pair; four taps)
  AREA, enlarging    LINEAR's            (either axis enlarging: computed as LINEAR)
  AREA, integer      2^-20               float32 block mean
  AREA, otherwise    4e-3                overlaps below 1e-3 are dropped without renormalising, up to two per axis, cell >= 1
  uint8 LINEAR/AREA  1 code              11-bit fixed point / rounding to a code (the 2x2 (sum + 2) >> 2 case is 0.5 at ties)
  Sobel              2^-19               sums of at most 8 float32 terms of magnitude < 1
  remap              2^-20               the 1/32-px weights are exact in float32; three float32 additions

Observed maxima on this suite's inputs (uniform [0, 1) float32, 0..255 uint8), largest over the cases of a row:

  case                                        bound       observed
  NEAREST, 21 shapes                          0           0
  LINEAR   N <= 101 (17 shapes)               2.5e-05     4.6e-06
  LINEAR   (270,480,4)->(240,135)             1.2e-04     4.5e-08
  LINEAR   (31,1000,3)->(999,30)              2.4e-04     2.7e-05
  LINEAR   (60,84,3)->(1920,1080)             4.6e-04     3.6e-06
  LINEAR   (3000,7,1)->(7,2999)               7.2e-04     1.2e-04
  CUBIC    N <= 101 (17 shapes)               5.0e-05     4.7e-06
  CUBIC    (270,480,4)->(240,135)             2.3e-04     2.8e-07
  CUBIC    (31,1000,3)->(999,30)              4.8e-04     3.8e-05
  CUBIC    (60,84,3)->(1920,1080)             9.2e-04     4.9e-06
  CUBIC    (3000,7,1)->(7,2999)               1.4e-03     1.2e-04
  AREA     enlarging, N <= 101                2.5e-05     1.8e-06
  AREA     (60,84,3)->(1920,1080)             4.6e-04     3.6e-06
  AREA     integer ratio                      9.5e-07     7.4e-08
  AREA     other shrinking                    4.0e-03     1.4e-07
  AREA     (3000,7,1)->(7,2999)               4.0e-03     5.6e-04
  uint8    LINEAR, 21 shapes                  1           0.81
  uint8    AREA, 21 shapes                    1           0.81
  Sobel    6 sizes                            1.9e-06     3.6e-07
  remap    3 sizes x 2 borders                9.5e-07     1.1e-07
  remap    with NaN, +-inf, +-1e30            9.5e-07     1.0e-07
"""
import numpy as np
import pytest

import _geom_ref as R
from _geom_cases import NONFINITE, REMAP_SIZES, SHAPES, SOBEL_SIZES, put_nonfinite, spanning_maps


def linear_bound(shape, dsize):
    return 2 * max(shape[0], shape[1], dsize[0], dsize[1]) * 2.0 ** -23 + 2.0 ** -20


def f32_bound(shape, dsize, interp):
    (H, W, _), (Wd, Hd) = shape, dsize
    if interp == R.INTER_NEAREST:
        return 0.0
    if interp == R.INTER_LINEAR or (interp == R.INTER_AREA and (Wd > W or Hd > H)):
        return linear_bound(shape, dsize)
    if interp == R.INTER_CUBIC:
        return 2 * linear_bound(shape, dsize)
    return 2.0 ** -20 if (W % Wd == 0 and H % Hd == 0) else 4e-3


def float_image(shape):
    return np.random.default_rng(sum(shape)).random(shape, dtype=np.float32)


def u8_image(shape):
    return np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("shape,dsize", SHAPES)
def test_resize_f32_vs_definition(oracle, shape, dsize):
    img = float_image(shape)
    for interp in (R.INTER_NEAREST, R.INTER_LINEAR, R.INTER_CUBIC, R.INTER_AREA):
        got = oracle.cv_resize(img, dsize, interp)
        err = float(np.abs(got - R.resize64(img, dsize, interp)).max())
        print(f"resize f32 {shape}->{dsize} interp {interp}: {err:.3g} (bound {f32_bound(shape, dsize, interp):.3g})")
        assert got.dtype == np.float32 and got.shape == (dsize[1], dsize[0], shape[2])
        assert err <= f32_bound(shape, dsize, interp), (shape, dsize, interp, err)


@pytest.mark.parametrize("shape,dsize", SHAPES)
def test_resize_u8_vs_definition(oracle, shape, dsize):
    img = u8_image(shape)
    for interp in (R.INTER_LINEAR, R.INTER_AREA):
        got = oracle.cv_resize(img, dsize, interp)
        err = float(np.abs(got - R.resize64(img, dsize, interp)).max())
        print(f"resize u8 {shape}->{dsize} interp {interp}: {err:.3g} (bound 1)")
        assert got.dtype == np.uint8 and err <= 1.0, (shape, dsize, interp, err)


@pytest.mark.parametrize("size", SOBEL_SIZES)
def test_sobel_vs_definition(oracle, size):
    p = np.random.default_rng(9).random(size, dtype=np.float32)
    gx, gy = R.sobel64(p)
    ex, ey = float(np.abs(oracle.cv_sobel3(p, 1, 0) - gx).max()), float(np.abs(oracle.cv_sobel3(p, 0, 1) - gy).max())
    print(f"sobel {size}: gx {ex:.3g} gy {ey:.3g} (bound {2.0 ** -19:.3g})")
    assert max(ex, ey) <= 2.0 ** -19, (size, ex, ey)


@pytest.mark.parametrize("size", REMAP_SIZES)
@pytest.mark.parametrize("border", [0.0, 0.25])
def test_remap_vs_definition(oracle, size, border):
    H, W = size
    img = float_image((H, W, 3))
    mx, my = spanning_maps(H, W, 5)
    err = float(np.abs(oracle.cv_remap_linear(img, mx, my, border) - R.remap64(img, mx, my, border)).max())
    print(f"remap {size} border {border}: {err:.3g} (bound {2.0 ** -20:.3g})")
    assert err <= 2.0 ** -20, (size, border, err)


@pytest.mark.parametrize("border", [0.0, 0.25])
def test_remap_nonfinite_coordinates_give_the_border(oracle, border):
    """A coordinate whose 1/32-px quantisation is NaN or outside int32 converts to INT_MIN in cv2 (x86 cvtss2si's "integer
    indefinite"), which saturates to -32768: the pixel takes borderValue, whatever the other coordinate is."""
    H, W = 37, 53
    img = float_image((H, W, 3))
    mx, my = put_nonfinite(*spanning_maps(H, W, 6))
    got = oracle.cv_remap_linear(img, mx, my, border)
    n = 2 * len(NONFINITE) + 1
    assert np.array_equal(got.reshape(-1, 3)[:n], np.full((n, 3), border, np.float32))
    err = float(np.abs(got - R.remap64(img, mx, my, border)).max())
    print(f"remap non-finite border {border}: {err:.3g} (bound {2.0 ** -20:.3g})")
    assert err <= 2.0 ** -20, (border, err)


def test_split_vs_definition(oracle):
    rng = np.random.default_rng(4)
    for W in (1, 2, 3, 5, 64, 65):
        a, b = rng.integers(0, 256, (3, W, 3), dtype=np.uint8), rng.integers(0, 256, (3, W, 3), dtype=np.uint8)
        for seam in (False, True):
            assert np.array_equal(oracle.make_split_frame_nolabel(a, b, seam), R.split64(a, b, seam)), (W, seam)
