"""CPU-only checks of the weight EMA: the sigma_rel <-> gamma relation, the power profile as an fp64 recursion, argument validation and
the C-ABI boundary (no kernel is launched)."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _sigma_rel(gamma):
    return math.sqrt((gamma + 1.0) / ((gamma + 2.0) ** 2 * (gamma + 3.0)))


def test_sigma_rel_to_gamma_values():
    from hdmoe_hip.ema import sigma_rel_to_gamma
    assert abs(sigma_rel_to_gamma(0.05) - 16.9722) <= 1e-4
    assert abs(sigma_rel_to_gamma(0.10) - 6.9372) <= 1e-4
    for s in (0.05, 0.10, 0.15, 0.25):
        assert abs(_sigma_rel(sigma_rel_to_gamma(s)) - s) <= 1e-12, s
    assert abs(sigma_rel_to_gamma(12.0 ** -0.5)) <= 1e-9                    # the upper end is gamma = 0


@pytest.mark.parametrize("bad", [0, 0.0, -0.05, 0.3, float("nan")])
def test_sigma_rel_out_of_range_raises(bad):
    from hdmoe_hip.ema import sigma_rel_to_gamma
    with pytest.raises(ValueError, match="sigma_rel"):
        sigma_rel_to_gamma(bad)


def test_profile_count_is_validated_before_anything_else():
    from hdmoe_hip.ema import WeightEMA
    m = torch.nn.Linear(3, 3)
    for bad in ([], [0.05] * 5):
        with pytest.raises(ValueError, match="sigma_rels"):
            WeightEMA(m, sigma_rels=bad)
        with pytest.raises(ValueError, match="betas"):
            WeightEMA(m, betas=[0.9] * len(bad))
    with pytest.raises(ValueError, match="sigma_rel"):
        WeightEMA(m, sigma_rels=[0.05, 0.3])
    with pytest.raises(ValueError, match="betas"):
        WeightEMA(m, betas=[1.0])


@pytest.mark.parametrize("gamma", [0.0, 6.9372, 16.9722])
def test_power_profile_impulse_response(gamma):
    """fp64 recursion e_t = beta_t e_{t-1} + (1 - beta_t) x_t over an impulse at step j: the weight of step j in e_T is
    (1 - beta_j) (j / T)^(gamma + 1), and the weights of j = 1..T sum to 1."""
    from hdmoe_hip.ema import power_beta
    T = 300
    assert power_beta(gamma, 1) == 0.0 and 0.0 < power_beta(gamma, 2) < 1.0
    total = 0.0
    for j in range(1, T + 1):
        e = 0.0
        for t in range(1, T + 1):
            b = power_beta(gamma, t)
            e = b * e + (1.0 - b) * (1.0 if t == j else 0.0)
        closed = (1.0 - power_beta(gamma, j)) * (j / T) ** (gamma + 1.0)
        assert abs(e - closed) <= 1e-12 * max(closed, 1e-300) + 1e-15, (j, e, closed)
        total += e
    assert abs(total - 1.0) <= 1e-12


def test_header_declares_and_library_exports_the_ema_entry_points():
    from hdmoe_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "hdmoe.h")).read()
    declared = set(re.findall(r"\bint\s+(hdmoe_\w+)\s*\(", hdr))
    assert {"hdmoe_mt_ema", "hdmoe_mt_swap", "hdmoe_ema_desc_bytes"} <= declared
    lib = _lib.lib()
    for name in ("hdmoe_mt_ema", "hdmoe_mt_swap"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert _lib.SIGNATURES["hdmoe_mt_ema"] == "ppiippis" and _lib.SIGNATURES["hdmoe_mt_swap"] == "ppiis"
    from hdmoe_hip import ema
    assert lib.hdmoe_ema_desc_bytes() == ema._DESC.itemsize == 48


def test_invalid_arguments_return_einval_without_a_launch():
    """Every rejected call returns before touching a pointer or the device, so fake non-null addresses are safe here."""
    from hdmoe_hip import _lib
    lib = _lib.lib()
    some = ctypes.c_void_p(4096)                                             # never dereferenced
    ema = lambda descs, chunks, n, k, step=some, coefs=some, mode=0: lib.hdmoe_mt_ema(descs, chunks, n, k, step, coefs, mode, None)
    for k in (0, 5, -1):
        assert ema(some, some, 3, k) == EINVAL
    assert ema(None, some, 3, 2) == EINVAL and ema(some, None, 3, 2) == EINVAL
    assert ema(some, some, 3, 2, step=None) == EINVAL and ema(some, some, 3, 2, coefs=None) == EINVAL
    assert ema(some, some, 3, 2, mode=2) == EINVAL and ema(some, some, -1, 2) == EINVAL
    assert ema(None, None, 0, 2) == 0                                        # nchunks == 0: a valid no-op
    swap = lambda descs, chunks, n, k: lib.hdmoe_mt_swap(descs, chunks, n, k, None)
    for k in (-1, 4):
        assert swap(some, some, 3, k) == EINVAL
    assert swap(None, some, 3, 0) == EINVAL and swap(some, None, 3, 0) == EINVAL
    assert swap(None, None, 0, 3) == 0


def test_cpu_or_non_fp32_models_are_refused():
    from hdmoe_hip.ema import WeightEMA
    with pytest.raises(RuntimeError):
        WeightEMA(torch.nn.Linear(3, 3))
    import hdmoe_hip
    assert hdmoe_hip.WeightEMA is WeightEMA


def test_checkpoint_keys_without_an_ema_are_the_references(tmp_path):
    import inspect
    from Utils import training
    assert inspect.signature(training.save_checkpoint).parameters["ema"].default is None
    assert inspect.signature(training.load_checkpoint).parameters["ema"].default is None
    assert inspect.signature(training.Trainer.__init__).parameters["ema"].default is None
    m = torch.nn.Linear(2, 2)
    path = training.save_checkpoint(m, torch.optim.SGD(m.parameters(), lr=0.1), 1, 0.0, {"save_dir": str(tmp_path)}, "c.pt")
    assert set(torch.load(path, weights_only=False)) == {"step", "model_state_dict", "optimizer_state_dict", "mse", "config"}
