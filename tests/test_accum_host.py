"""Gradient accumulation without a GPU: the NumPy twin of llie_grad_accumulate (the definition), what the
C entry refuses before any launch, the window lengths of `accumulation_windows`, and the --accumulate flag of scripts/train.py."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

M = importlib.import_module("cv-diffusion-model_amd")
T = importlib.import_module("cv-diffusion-model_amd.training")
native = importlib.import_module("cv-diffusion-model_amd._native")

EPS32 = 2.0 ** -24  # unit roundoff of fp32


def train_script():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return importlib.import_module("train")
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))


def test_public_names():
    for name in ("grad_accumulate_array", "accumulation_windows"):
        assert name in M.__all__ and getattr(M, name) is getattr(T, name)
    assert "llie_grad_accumulate" in native.EXPORTS and native.lib().llie_grad_accumulate
    for cls in (M.TrainStep, M.DistillStep):
        for name in ("accumulate", "apply", "discard", "window_images"):
            assert hasattr(cls, name), (cls.__name__, name)


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize("weight", [1, 2, 3, 5, 7])
def test_twin_against_float64(weight):
    """acc + weight * grad in fp32 with two roundings: against the float64 value the error of an element is at most one
    rounding of the product plus one of the sum, |w g| u + |a + w g (1 + u)| u <= (|w g| + |a + w g|) u (1 + u), u = 2^-24;
    with `first` it is the one rounding of the product.  (Magnitudes of order 1: no underflow.)"""
    rng = np.random.default_rng(weight)
    a = rng.standard_normal(4099).astype(np.float32)
    g = rng.standard_normal(4099).astype(np.float32)
    a64, g64 = a.astype(np.float64), g.astype(np.float64)
    out = T.grad_accumulate_array(a, g, weight, False)
    assert out.dtype == np.float32 and out.shape == a.shape
    exact = a64 + weight * g64
    bound = (np.abs(weight * g64) + np.abs(exact)) * EPS32 * (1 + 2 * EPS32)
    assert (np.abs(out.astype(np.float64) - exact) <= bound).all()
    # it is exactly the two fp32 operations
    w32 = np.float32(weight)
    assert np.array_equal(out, a + (w32 * g).astype(np.float32))
    first = T.grad_accumulate_array(a, g, weight, True)
    assert first.dtype == np.float32
    assert (np.abs(first.astype(np.float64) - weight * g64) <= np.abs(weight * g64) * EPS32).all()
    # the inputs are left alone
    assert np.array_equal(a64, a.astype(np.float64)) and np.array_equal(g64, g.astype(np.float64))


def test_twin_first_ignores_a_poisoned_accumulator():
    g = np.linspace(-2, 2, 37, dtype=np.float32)
    poisoned = np.full(37, np.nan, dtype=np.float32)
    out = T.grad_accumulate_array(poisoned, g, 3.0, True)
    assert np.isfinite(out).all() and np.array_equal(out, np.float32(3.0) * g)
    assert np.array_equal(T.grad_accumulate_array(None, g, 3.0, True), out)  # `acc` is not read at all
    assert np.isnan(T.grad_accumulate_array(poisoned, g, 3.0, False)).all()


def test_twin_propagates_inf_and_nan_and_refuses_bad_weights():
    g = np.array([1.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    one = T.grad_accumulate_array(None, g, 2.0, True)
    assert one[0] == 2.0 and one[1] == np.inf and one[2] == -np.inf and np.isnan(one[3])
    two = T.grad_accumulate_array(one, -g, 2.0, False)  # inf followed by -inf is NaN
    assert two[0] == 0.0 and np.isnan(two[1:]).all()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.grad_accumulate_array(None, g, bad, True)
    with pytest.raises(ValueError):
        T.grad_accumulate_array(np.zeros(3, np.float32), g, 1.0, False)


# ------------------------------------------------------------------ the C entry's refusals (all before any HIP call)
def test_abi_refusals_and_empty_call():
    L = native.lib()
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 16
    acc, grad = base, base + 32 * 4  # host memory: never dereferenced, a refusal comes before any launch

    def call(a, g, n, w, first=1):
        return L.llie_grad_accumulate(a, g, n, w, first, None)

    assert call(None, grad, 4, 1.0) == native.ERR_ARG
    assert call(acc, None, 4, 1.0) == native.ERR_ARG
    assert call(acc, grad, -1, 1.0) == native.ERR_ARG
    for w in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(acc, grad, 4, w) == native.ERR_ARG, w
        assert call(acc, grad, 0, w) == native.ERR_ARG, w  # also for an empty call
    assert "weight" in native.last_error()
    # overlapping ranges: the same buffer, a partial overlap from either side; touching ranges do not overlap
    assert call(acc, acc, 4, 1.0, 0) == native.ERR_ARG
    assert call(acc, acc + 12, 4, 1.0) == native.ERR_ARG
    assert call(acc + 12, acc, 4, 1.0) == native.ERR_ARG
    assert "overlap" in native.last_error()
    assert call(acc, acc + 16, 0, 1.0) == 0
    # a pointer that is not a float's
    assert call(acc + 2, grad, 4, 1.0) == native.ERR_ARG
    # n == 0: OK, nothing launched (there is no device here to launch on)
    before = L.llie_last_kernel()
    assert call(acc, grad, 0, 1.0) == 0 and call(acc, grad, 0, 3.0, 0) == 0
    assert L.llie_last_kernel() == before


# ------------------------------------------------------------------ window lengths
def test_accumulation_windows_sweep():
    for n in range(1, 21):
        for k in range(1, 9):
            w = T.accumulation_windows(n, k)
            assert sum(w) == n and len(w) == -(-n // k), (n, k, w)
            assert all(v == k for v in w[:-1]) and 1 <= w[-1] <= k, (n, k, w)
    assert T.accumulation_windows(3, 2) == [2, 1] and T.accumulation_windows(4, 2) == [2, 2] and T.accumulation_windows(3, 1) == [1, 1, 1]
    assert T.accumulation_windows(0, 4) == []
    for n, k in ((3, 0), (3, -1), (-1, 2)):
        with pytest.raises(ValueError):
            T.accumulation_windows(n, k)


# ------------------------------------------------------------------ the script and the trainer's keyword
def test_train_script_accumulate_flag(capsys):
    mod = train_script()
    assert mod.parse_args([]).accumulate == 1
    assert mod.parse_args(["--accumulate", "8"]).accumulate == 8
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit):
            mod.parse_args(["--accumulate", bad])
        assert "--accumulate" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.parse_args(["--accumulate", "1.5"])
    # a keyword of the trainer, not a TrainingConfig field (so not in a checkpoint's "config")
    assert "accumulate" not in M.TrainingConfig().__dict__
    import inspect
    for fn in (M.LowLightTrainer.__init__, M.train_model):
        p = inspect.signature(fn).parameters["accumulate"]
        assert p.default == 1 and p.kind is inspect.Parameter.KEYWORD_ONLY
