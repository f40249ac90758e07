"""plink_glm's host pieces: the two-sided p-values the fits report (against scipy) and the bind-time model rule."""

import math

import numpy as np
import pytest

scipy_stats = pytest.importorskip("scipy.stats")


def _close(got, exp, rel=1e-8):
    # below the smallest normal double the reference value itself is not representable to 1e-8
    return abs(got - exp) <= rel * abs(exp) + 1e-300


@pytest.mark.parametrize("df", [1, 2, 3, 5, 10, 30, 100, 1000, 12345, 1e5, 1e6])
def test_p_from_t_matches_scipy(lib, df):
    for t in [0.0, 1e-8, 0.1, 0.5, 1.0, 1.96, 2.5, 3.0, 5.0, 8.0, 12.0, 20.0, 30.0, 40.0]:
        for sgn in (1.0, -1.0):
            got = lib.glm_p_from_t(sgn * t, df)
            exp = 2.0 * scipy_stats.t.sf(abs(t), df) if t > 0 else 1.0
            assert _close(got, exp), (t, df, got, exp)


def test_p_from_t_edges(lib):
    assert math.isnan(lib.glm_p_from_t(float("nan"), 5))
    assert math.isnan(lib.glm_p_from_t(1.0, 0))
    assert lib.glm_p_from_t(float("inf"), 5) == 0.0


def test_p_from_z_matches_scipy(lib):
    for z in np.concatenate([np.linspace(0, 5, 51), np.linspace(5, 37, 65)]):
        for sgn in (1.0, -1.0):
            got = lib.glm_p_from_z(sgn * z)
            exp = 2.0 * scipy_stats.norm.sf(z)
            assert _close(got, exp), (z, got, exp)
    assert lib.glm_p_from_z(37.0) > 1e-300
    assert math.isnan(lib.glm_p_from_z(float("nan")))


def test_glm_model_rule(lib):
    m, y = lib.glm_model([0, 1, 0, 1, 1, 0])
    assert m == lib.GLM_LOGISTIC and np.array_equal(y, [0, 1, 0, 1, 1, 0])
    m, y = lib.glm_model([1, 2, 1, 2, 2, 1])
    assert m == lib.GLM_LOGISTIC and np.array_equal(y, [0, 1, 0, 1, 1, 0])
    m, y = lib.glm_model([1.2, 3.4, 2.1])
    assert m == lib.GLM_LINEAR and np.array_equal(y, [1.2, 3.4, 2.1])
    # mixed 0/1/2 is neither rule
    m, _ = lib.glm_model([0, 1, 2])
    assert m == lib.GLM_LINEAR
    # NULL / NaN values are skipped by the rule and kept as NaN
    m, y = lib.glm_model([1, None, 2, float("nan"), 2])
    assert m == lib.GLM_LOGISTIC
    assert np.array_equal(np.isnan(y), [False, True, False, True, False]) and np.nansum(y) == 2.0
    m, y = lib.glm_model([0, None, 1])
    assert m == lib.GLM_LOGISTIC and y[0] == 0 and y[2] == 1
    # explicit models pass the values through
    m, y = lib.glm_model([0, 1, 0], "linear")
    assert m == lib.GLM_LINEAR
    m, y = lib.glm_model([1.5, 2.5], "logistic")
    assert m == lib.GLM_LOGISTIC and np.array_equal(y, [1.5, 2.5])
    with pytest.raises(ValueError):
        lib.glm_model([0, 1], "probit")


def test_glm_abi_constants(lib):
    assert lib.GLM_ERRCODES[0] is None and len(lib.GLM_ERRCODES) == 7
    assert lib.GLM_ROW_DTYPE.itemsize == 48
    import ctypes
    assert ctypes.sizeof(lib.PghGlmRow) == 48
