"""CPU-only checks of the post-hoc EMA reconstruction (hdmoe_hip/posthoc.py): the closed-form profile inner product against quadrature,
the least-squares weights, the accuracy of the method on an fp64 random walk, snapshot files, the C-ABI boundary of hdmoe_mt_combine
(no kernel is launched) and the Trainer keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GAMMAS = (0.0, 6.94, 16.97)


# ------------------------------------------------------------------------------------------------------------ 1. profile_dot
def _quadrature(t_a, g_a, t_b, g_b, n):
    """Trapezoid rule on n intervals over [0, min(t_a, t_b)] (both profiles vanish beyond their own end; the product is smooth there)."""
    tau = np.linspace(0.0, min(t_a, t_b), n + 1)
    pa = (g_a + 1.0) * tau ** g_a / t_a ** (g_a + 1.0)
    pb = (g_b + 1.0) * tau ** g_b / t_b ** (g_b + 1.0)
    y = pa * pb
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(tau)))


@pytest.mark.parametrize("t_a,t_b", [(300.0, 1000.0), (1000.0, 1000.0), (1000.0, 450.0)])
@pytest.mark.parametrize("g_a", GAMMAS)
@pytest.mark.parametrize("g_b", GAMMAS)
def test_profile_dot_matches_quadrature(t_a, t_b, g_a, g_b):
    from hdmoe_hip.posthoc import profile_dot
    n = 1 << 18
    fine, coarse = _quadrature(t_a, g_a, t_b, g_b, n), _quadrature(t_a, g_a, t_b, g_b, n // 2)
    quad_err = abs(fine - coarse)                      # the trapezoid error falls 4x per halving: |fine - coarse| = 3x the fine grid's error
    got = float(profile_dot(t_a, g_a, t_b, g_b))
    assert abs(got - fine) <= quad_err + 1e-13 * abs(fine), (got, fine, quad_err)
    assert got == float(profile_dot(t_b, g_b, t_a, g_a))                   # symmetric


# ------------------------------------------------------------------------------------------------------------ 2. solve_weights
def _sources(T, every, srel=(0.05, 0.10)):
    from hdmoe_hip.ema import sigma_rel_to_gamma
    steps, gammas = [], []
    for t in range(every, T + 1, every):
        for s in srel:
            steps.append(t)
            gammas.append(sigma_rel_to_gamma(s))
    return steps, gammas


def test_target_equal_to_a_source_is_one_hot():
    from hdmoe_hip.posthoc import solve_weights
    steps, gammas = _sources(1000, 50)
    for i in (0, 17, len(steps) - 1):
        X, fit = solve_weights(steps, gammas, [steps[i]], [gammas[i] * (1.0 + 5e-13)])
        want = np.zeros((len(steps), 1))
        want[i, 0] = 1.0
        assert np.array_equal(X, want) and fit[0] == 0.0


def test_interior_target_weights():
    from hdmoe_hip.ema import sigma_rel_to_gamma
    from hdmoe_hip.posthoc import profile_dot, solve_weights
    steps, gammas = _sources(1000, 50)
    g = sigma_rel_to_gamma(0.075)
    X, fit = solve_weights(steps, gammas, [1000, 1000], [g, gammas[-1]])    # one solved column next to a one-hot one
    print(f"sum of weights {X[:, 0].sum():.6f}, max |x| {np.abs(X[:, 0]).max():.3f}, fit_error {fit[0]:.3e}")
    assert abs(X[:, 0].sum() - 1.0) <= 1e-3
    assert X[-1, 1] == 1.0 and np.count_nonzero(X[:, 1]) == 1 and fit[1] == 0.0
    st, sg = np.array(steps, dtype=np.float64), np.array(gammas)
    A = profile_dot(st[:, None], sg[:, None], st[None, :], sg[None, :])
    B = profile_dot(st, sg, 1000.0, g)
    assert np.abs(A @ X[:, 0] - B).max() <= 1e-10 * np.abs(B).max()
    assert 0.0 < fit[0] < 0.05


def test_fit_error_falls_with_the_snapshot_interval():
    from hdmoe_hip.ema import sigma_rel_to_gamma
    from hdmoe_hip.posthoc import solve_weights
    for srel in (0.075, 0.15):
        errs = [float(solve_weights(*_sources(1000, every), [1000], [sigma_rel_to_gamma(srel)])[1][0]) for every in (200, 100, 50, 25)]
        print(srel, errs)
        assert all(b < a for a, b in zip(errs, errs[1:])), errs


def test_solve_weights_rejects():
    from hdmoe_hip.posthoc import solve_weights
    steps, gammas = _sources(1000, 250)
    with pytest.raises(ValueError, match="same profile"):
        solve_weights(steps + [steps[2]], gammas + [gammas[2]], [1000], [3.0])
    with pytest.raises(ValueError, match="extrapolation"):
        solve_weights(steps, gammas, [1001], [3.0])
    with pytest.raises(ValueError, match="step"):
        solve_weights(steps, gammas, [0], [3.0])
    with pytest.raises(ValueError, match="step"):
        solve_weights([0] + steps, [3.0] + gammas, [500], [3.0])
    solve_weights(steps, gammas, [1], [3.0])                                # step 1 is the first valid one


# ------------------------------------------------------------------------------------------------------------ 3. the method
def _random_walk(T, every, targets, n=256, seed=0):
    """fp64: a random walk of per-step increment 0.02 N(0,1), averaged exactly by the recursion `power_beta` defines; profiles 0.05 and
    0.10 saved every `every` steps.  Returns (saved [(step, gamma, e)], {sigma_rel: exactly tracked e at T})."""
    from hdmoe_hip.ema import power_beta, sigma_rel_to_gamma
    rng = np.random.default_rng(seed)
    g = {s: sigma_rel_to_gamma(s) for s in (0.05, 0.10) + tuple(targets)}
    p = rng.standard_normal(n)
    e = {s: p.copy() for s in g}
    saved = []
    for t in range(1, T + 1):
        p = p + 0.02 * rng.standard_normal(n)
        for s in g:
            b = power_beta(g[s], t)
            e[s] = b * e[s] + (1.0 - b) * p
        if t % every == 0:
            saved += [(t, g[s], e[s].copy()) for s in (0.05, 0.10)]
    return saved, e, g


@pytest.mark.parametrize("T,every", [(1000, 50), (400, 25)])
def test_reconstruction_beats_the_nearer_tracked_profile_tenfold(T, every):
    from hdmoe_hip.posthoc import solve_weights
    saved, e, g = _random_walk(T, every, (0.075,))
    X, fit = solve_weights([s[0] for s in saved], [s[1] for s in saved], [T], [g[0.075]])
    rec = sum(x * s[2] for x, s in zip(X[:, 0], saved))
    err = float(np.abs(rec - e[0.075]).max())
    near = min(float(np.abs(e[s] - e[0.075]).max()) for s in (0.05, 0.10))
    print(f"T = {T}, every {every}: reconstruction max err {err:.3e}, nearer tracked profile {near:.3e}, ratio {near / err:.0f}x, "
          f"fit_error {fit[0]:.3e}")
    assert near >= 10.0 * err


# ------------------------------------------------------------------------------------------------------------ 4. files
def _state(step, seed=0, mode="power", names=("a.weight", "a.bias", "b"), shapes=((3, 4), (3,), (5,))):
    from hdmoe_hip.ema import sigma_rel_to_gamma
    gen = torch.Generator().manual_seed(seed)
    srel = [0.05, 0.10]
    return {"step": step, "mode": mode, "sigma_rels": srel if mode == "power" else None,
            "gammas": [sigma_rel_to_gamma(s) for s in srel] if mode == "power" else None, "betas": None if mode == "power" else [0.9, 0.99],
            "profiles": [{n: torch.randn(sh, generator=gen) for n, sh in zip(names, shapes)} for _ in srel]}


def test_load_sources_reads_directories_checkpoints_and_dicts(tmp_path):
    from hdmoe_hip import posthoc
    from hdmoe_hip.ema import SNAPSHOT_FORMAT
    assert SNAPSHOT_FORMAT == "hdmoe-ema-snapshot-1"
    d = tmp_path / "snaps"
    d.mkdir()
    for step in (30, 10, 20):
        torch.save(dict(_state(step, seed=step), format=SNAPSHOT_FORMAT), str(d / f"ema_{step:08d}.pt"))
    (d / "notes.txt").write_text("not a snapshot")
    ck = tmp_path / "ckpt.pt"
    torch.save({"step": 40, "model_state_dict": {}, "ema_state_dict": _state(40, seed=40)}, str(ck))
    got = posthoc.load_sources([str(d), ck, _state(50, seed=50), {"ema_state_dict": _state(60, seed=60)}])
    assert [s["step"] for s in got] == [10, 20, 30, 40, 50, 60]
    assert got[0]["label"].endswith("ema_00000010.pt") and got[0]["format"] == SNAPSHOT_FORMAT
    assert torch.equal(got[3]["profiles"][1]["b"], _state(40, seed=40)["profiles"][1]["b"])
    assert [s["step"] for s in posthoc.load_sources(str(d))] == [10, 20, 30]
    assert [s["step"] for s in posthoc.load_sources(_state(7))] == [7]


def test_load_sources_rejects(tmp_path):
    from hdmoe_hip import posthoc
    f = tmp_path / "const.pt"
    torch.save(_state(10, mode="constant"), str(f))
    with pytest.raises(ValueError, match="const.pt"):
        posthoc.load_sources([_state(5), str(f)])
    with pytest.raises(ValueError, match="step"):
        posthoc.load_sources([_state(0)])
    with pytest.raises(ValueError, match="format"):
        posthoc.load_sources([dict(_state(3), format="something-else")])
    with pytest.raises(ValueError):
        posthoc.load_sources([{"model_state_dict": {}}])
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no \\*.pt"):
        posthoc.load_sources(tmp_path / "empty")
    with pytest.raises(ValueError):
        posthoc.load_sources([])
    with pytest.raises(KeyError, match="names"):
        posthoc.load_sources([_state(5), _state(6, names=("a.weight", "a.bias", "c"))])
    with pytest.raises(KeyError, match="order"):
        posthoc.load_sources([_state(5), _state(6, names=("a.bias", "a.weight", "b"), shapes=((3,), (3, 4), (5,)))])
    with pytest.raises(ValueError, match="shape"):
        posthoc.load_sources([_state(5), _state(6, shapes=((3, 4), (3,), (6,)))])


def test_save_snapshot_exists_and_the_package_exports_the_interface():
    import hdmoe_hip
    from hdmoe_hip.ema import WeightEMA
    assert callable(WeightEMA.save_snapshot) and "sync" in WeightEMA.save_snapshot.__doc__
    assert hdmoe_hip.posthoc.reconstruct and hdmoe_hip.ReconstructedEMA is hdmoe_hip.posthoc.ReconstructedEMA
    assert not hasattr(hdmoe_hip.ReconstructedEMA, "update")
    for name in ("swapped", "profile_state_dict", "copy_to"):
        assert getattr(hdmoe_hip.ReconstructedEMA, name) is getattr(WeightEMA, name)
    with pytest.raises(RuntimeError):                                       # a CPU model is refused like WeightEMA refuses it
        hdmoe_hip.posthoc.reconstruct(torch.nn.Linear(3, 3), [_state(5, names=("weight", "bias"), shapes=((3, 3), (3,)))], [0.075])


# ------------------------------------------------------------------------------------------------------------ 5. C ABI
def test_header_declares_and_library_exports_the_combine_entry_point():
    from hdmoe_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "hdmoe.h")).read()
    assert "hdmoe_mt_combine" in set(re.findall(r"\bint\s+(hdmoe_\w+)\s*\(", hdr))
    assert isinstance(getattr(_lib.lib(), "hdmoe_mt_combine"), ctypes._CFuncPtr)
    assert _lib.SIGNATURES["hdmoe_mt_combine"] == "ppiilps"


def test_combine_invalid_arguments_return_einval_without_a_launch():
    """Every rejected call returns before touching a pointer or the device, so fake non-null addresses are safe here."""
    from hdmoe_hip import _lib
    lib = _lib.lib()
    some = ctypes.c_void_p(4096)                                             # never dereferenced
    comb = lambda src, dst, nsrc, ndst, numel, w=some: lib.hdmoe_mt_combine(src, dst, nsrc, ndst, numel, w, None)
    for nsrc in (0, -1, 4097):
        assert comb(some, some, nsrc, 2, 100) == EINVAL
    for ndst in (0, -1, 9):
        assert comb(some, some, 3, ndst, 100) == EINVAL
    assert comb(some, some, 3, 2, -1) == EINVAL
    assert comb(None, some, 3, 2, 100) == EINVAL and comb(some, None, 3, 2, 100) == EINVAL
    assert comb(some, some, 3, 2, 100, w=None) == EINVAL
    assert comb(some, some, 3, 2, 0) == 0 and comb(some, some, 4096, 8, 0) == 0   # numel == 0: a valid no-op


# ------------------------------------------------------------------------------------------------------------ 6. Trainer keywords
def test_trainer_snapshot_keywords():
    from Utils import training
    sig = inspect.signature(training.Trainer.__init__).parameters
    assert sig["ema_snapshot_every"].default is None and sig["ema_snapshot_dir"].default is None
    m = torch.nn.Linear(2, 2)                                               # never reaches the device: the keywords are checked first
    with pytest.raises(ValueError, match="ema"):
        training.Trainer(m, {}, {}, {}, {}, {}, ema=None, ema_snapshot_every=2, ema_snapshot_dir="x")
    with pytest.raises(ValueError, match="ema_snapshot_dir"):
        training.Trainer(m, {}, {}, {}, {}, {}, ema=object(), ema_snapshot_every=2)
