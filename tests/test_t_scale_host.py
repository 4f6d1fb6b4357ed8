"""The exponent of the frame kernel's scaled visit time on the CPU (rt_internal.h visit_time_exp,
`__host__ __device__`: rt_host_visit_time_exp runs what a launch runs).

The coherent slot test clamps axis 0's entry distance to [0, 1] in scaled time t 2^-E, so 2^E must
exceed every entry distance a ray of the launch can have: kVisitTimeFactor = 2 times the larger of
the camera's distance to the farthest corner of the culling tree's root box (primary rays, unit
directions) and the box's diagonal (shadow rays start inside the box).  Checked here, against
exact rational arithmetic on the fp32 inputs:

  * 4^E >= 4 r^2 and 4^(E-1) < 4 r^2 (the smallest such E), r^2 the larger squared distance, with a
    relative slack of 2^-45 for the helper's double roundings (five additions and products);
  * |E| <= 64, the bound reached only where the rule asks for more (boxes beyond 2^62 or below
    2^-66), and 0 for a box or camera that is not finite or a box and camera at one point;
  * within that bound the reciprocal of any tested direction component (|d| >= 1e-6, |d| <= 1 for
    a unit vector, so 1 <= |1 / d| <= 2^20) times 2^-E is normal and finite, and scaling it back
    returns its bits.

Cases: the camera inside the box, on a face, on a corner, and 1, 100 and 10^6 box sizes away along
an axis and a diagonal; unit boxes, flat and degenerate ones, and the boxes of tests/placed.py's
scales and offsets (scenes.PLACEMENTS); 2,000 random ones over 2^-40 .. 2^40."""
from fractions import Fraction

import numpy as np
import pytest

import scenes

F = np.float32
LIMIT = 64
SLACK = Fraction(1, 2 ** 45)
INT_MIN = -2 ** 31


def time_exp(box, cam):
    from ceng795_amd import _lib
    b = np.ascontiguousarray(box, F)
    c = np.ascontiguousarray(cam, F)
    assert b.shape == (6,) and c.shape == (3,)
    return _lib.lib().rt_host_visit_time_exp(b.ctypes.data, c.ctypes.data)


def r2_exact(box, cam):
    b = [Fraction(float(x)) for x in np.asarray(box, F)]
    c = [Fraction(float(x)) for x in np.asarray(cam, F)]
    far = sum(max(abs(c[x] - b[x]), abs(c[x] - b[x + 3])) ** 2 for x in range(3))
    diag = sum((b[x + 3] - b[x]) ** 2 for x in range(3))
    return max(far, diag)


def check(box, cam, what=""):
    e = time_exp(box, cam)
    need = 4 * r2_exact(box, cam)  # (2 r)^2
    assert -LIMIT <= e <= LIMIT, (what, e)
    if need == 0:
        assert e == 0, what
        return e
    p = Fraction(4) ** e
    if e < LIMIT:
        assert p >= need * (1 - SLACK), (what, e)
    if e > -LIMIT:
        assert p / 4 < need * (1 + SLACK), (what, e)
    return e


def cameras_for(box):
    lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
    c, size = (lo + hi) / 2, float(np.sqrt(((hi - lo) ** 2).sum()))
    yield "inside", c
    yield "on a face", np.array([hi[0], c[1], c[2]])
    yield "on a corner", hi
    for k in (1, 100, 1e6):
        yield f"{k:g} sizes along x", c + np.array([k * size, 0, 0])
        yield f"{k:g} sizes along the diagonal", c - k * (hi - lo)


BASE_BOXES = {
    "unit": (-1, -1, -1, 1, 1, 1),
    "height field": (-3, -1.65, -8, 3, -1.33, -2),
    "flat": (-2, 0, -2, 2, 0, 2),
    "line": (0, 0, -5, 0, 0, 5),
}


@pytest.mark.parametrize("name", list(BASE_BOXES))
def test_base_boxes(name):
    box = np.array(BASE_BOXES[name], F)
    for what, cam in cameras_for(box):
        e = check(box, cam.astype(F), f"{name}/{what}")
        if what == "inside" and name == "unit":
            assert e == 3  # the diagonal 2 sqrt 3 = 3.46 decides: 2^3 >= 6.93 > 2^2


@pytest.mark.parametrize("placement", list(scenes.PLACEMENTS))
def test_placed_scales(placement):
    s, T = scenes.PLACEMENTS[placement]
    for name, b in BASE_BOXES.items():
        b = np.asarray(b, np.float64)
        box = (b * s + np.tile(np.asarray(T, np.float64), 2)).astype(F)
        for what, cam in cameras_for(box):
            e = check(box, cam.astype(F), f"{name}@{placement}/{what}")
            assert abs(e) < LIMIT


def test_random_boxes():
    rng = np.random.default_rng(795)
    for i in range(2000):
        size = 2.0 ** rng.uniform(-40, 40)
        centre = rng.normal(size=3) * 2.0 ** rng.uniform(-40, 40)
        half = rng.uniform(0, 1, 3) * size
        box = np.concatenate([centre - half, centre + half]).astype(F)
        cam = (centre + rng.normal(size=3) * size * 10.0 ** rng.uniform(-3, 6)).astype(F)
        check(box, cam, f"random {i}")


def test_the_bound_is_reached_only_beyond_it():
    assert check(np.array([-1, -1, -1, 1, 1, 1], F) * F(2.0 ** 70), np.zeros(3, F)) == LIMIT
    assert check(np.array([-1, -1, -1, 1, 1, 1], F) * F(2.0 ** -80), np.zeros(3, F)) == -LIMIT
    assert check(np.array([-1, -1, -1, 1, 1, 1], F), np.array([3e38, 0, 0], F)) == LIMIT
    big = np.array([-3e38, -3e38, -3e38, 3e38, 3e38, 3e38], F)  # squares beyond fp32, not double
    assert check(big, np.array([3e38, -3e38, 3e38], F)) == LIMIT
    assert check(np.zeros(6, F), np.zeros(3, F)) == 0  # a point: nothing to scale


def test_not_finite_gives_zero():
    unit = np.array([-1, -1, -1, 1, 1, 1], F)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            box = unit.copy()
            box[k] = bad
            assert time_exp(box, np.zeros(3, F)) == 0
        for k in range(3):
            cam = np.zeros(3, F)
            cam[k] = bad
            assert time_exp(unit, cam) == 0
    from ceng795_amd import _lib
    assert _lib.lib().rt_host_visit_time_exp(None, np.zeros(3, F).ctypes.data) == INT_MIN
    assert _lib.lib().rt_host_visit_time_exp(unit.ctypes.data, None) == INT_MIN


def test_reciprocals_stay_normal():
    tiny, huge = 2.0 ** -126, float(np.finfo(F).max)
    rcs = np.array([1.0, 1.0 / F(1e-6), 2.0 ** 20, F(1) / F(0.99999994)], F)
    for e in range(-LIMIT, LIMIT + 1):
        v = np.ldexp(rcs, -e).astype(F)
        assert np.isfinite(v).all() and (np.abs(v) >= tiny).all()
        assert (np.abs(v) <= huge).all()
        assert np.array_equal(np.ldexp(v, e).astype(F), rcs)  # exact: the scaling loses no bit
