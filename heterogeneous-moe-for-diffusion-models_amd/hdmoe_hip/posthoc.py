"""Post-hoc EMA: rebuild the power-function average of any sigma_rel, at any saved step, from snapshots of a few tracked ones.

    ema = WeightEMA(model, sigma_rels=(0.05, 0.10))
    ... Trainer(..., ema=ema, ema_snapshot_every=5000, ema_snapshot_dir="run/ema")        # or ema.save_snapshot(path) by hand
    rec = hdmoe_hip.posthoc.reconstruct(model, "run/ema", sigma_rels=[0.03, 0.075, 0.15])
    print(rec.fit_error)
    with rec.swapped(1):                                                                   # the parameters ARE sigma_rel 0.075 in here
        images = sampler.sample(...)

Karras et al., "Analyzing and Improving the Training Dynamics of Diffusion Models" (EDM2), section 3.2: an average with power profile
p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) on [0, t] is a linear functional of the weight trajectory, so the average of a
profile that was not tracked is approximated by the combination sum_s x_s e_s of the saved ones whose combined profile is closest to the
wanted one in L2.  The normal equations A x = b need only inner products of profiles, which have the closed form of `profile_dot`.  The
solve runs on the host in fp64; the combination of the saved tensors is one pass of `hdmoe_mt_combine` over all of them on the device.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call
from .ema import _ALIGN, SNAPSHOT_FORMAT, _Profiles, sigma_rel_to_gamma

MAX_TARGETS_PER_LAUNCH = 8                  # hdmoe_mt_combine: 1 <= ndst <= 8
MAX_SOURCES = 4096                          # hdmoe_mt_combine: 1 <= nsrc <= 4096
_SAME_GAMMA = 1e-12                         # relative: a target this close to a saved profile of the same step IS that profile


# -------------------------------------------------------------------------------------------------------------------- solver
def profile_dot(t_a, gamma_a, t_b, gamma_b):
    """Inner product of the continuous power profiles (t_a, gamma_a) and (t_b, gamma_b); arguments broadcast, fp64.  With `lo` the
    profile that ends first and `hi` the other: (g_lo + 1)(g_hi + 1)(t_lo / t_hi)^g_hi / ((g_lo + g_hi + 1) t_hi)."""
    t_a, g_a, t_b, g_b = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (t_a, gamma_a, t_b, gamma_b)))
    a_first = t_a <= t_b
    t_lo, t_hi = np.where(a_first, t_a, t_b), np.where(a_first, t_b, t_a)
    g_lo, g_hi = np.where(a_first, g_a, g_b), np.where(a_first, g_b, g_a)
    return (g_lo + 1.0) * (g_hi + 1.0) * (t_lo / t_hi) ** g_hi / ((g_lo + g_hi + 1.0) * t_hi)


def _same_gamma(a, b):
    return np.abs(a - b) <= _SAME_GAMMA * np.maximum(np.abs(a), np.abs(b))


def solve_weights(src_steps, src_gammas, dst_steps, dst_gammas) -> Tuple[np.ndarray, np.ndarray]:
    """(X [nsrc][ndst], fit_error [ndst]): column t of X holds the weights of the saved profiles whose combination is the least-squares
    fit of target profile t, A X = B with A = <src, src> and B = <src, dst>.  fit_error[t] = sqrt(max(0, 1 - B_t . X_t / <dst_t, dst_t>))
    is the relative part of the target profile the sources cannot represent (0: exact); it is for the user to read, nothing is cut off.
    A target that is one of the sources gets that source alone, weight 1, without solving."""
    st, sg = np.asarray(src_steps, dtype=np.float64).reshape(-1), np.asarray(src_gammas, dtype=np.float64).reshape(-1)
    dt, dg = np.asarray(dst_steps, dtype=np.float64).reshape(-1), np.asarray(dst_gammas, dtype=np.float64).reshape(-1)
    if st.shape != sg.shape or dt.shape != dg.shape or st.size == 0 or dt.size == 0:
        raise ValueError(f"solve_weights: {st.size} source steps / {sg.size} gammas, {dt.size} target steps / {dg.size} gammas")
    if not (np.all(st >= 1) and np.all(dt >= 1)):
        raise ValueError("solve_weights: every step must be >= 1")
    if not (np.all(sg >= 0) and np.all(dg >= 0)):
        raise ValueError("solve_weights: every gamma must be >= 0")
    if np.any(dt > st.max()):
        raise ValueError(f"solve_weights: target step {int(dt.max())} lies beyond the last source step {int(st.max())} (no extrapolation)")
    same_src = (st[:, None] == st[None, :]) & _same_gamma(sg[:, None], sg[None, :])
    np.fill_diagonal(same_src, False)
    if same_src.any():
        i, j = np.argwhere(same_src)[0]
        raise ValueError(f"solve_weights: sources {i} and {j} are the same profile (step {int(st[i])}, gamma {sg[i]:.6g})")
    hit = (st[:, None] == dt[None, :]) & _same_gamma(sg[:, None], dg[None, :])               # [nsrc][ndst], at most one per column
    X = np.zeros((st.size, dt.size), dtype=np.float64)
    fit = np.zeros(dt.size, dtype=np.float64)
    todo = ~hit.any(axis=0)
    X[:, ~todo] = hit[:, ~todo]
    if todo.any():
        A = profile_dot(st[:, None], sg[:, None], st[None, :], sg[None, :])
        B = profile_dot(st[:, None], sg[:, None], dt[None, todo], dg[None, todo])
        Xs = np.linalg.solve(A, B)
        X[:, todo] = Xs
        fit[todo] = np.sqrt(np.maximum(0.0, 1.0 - np.sum(B * Xs, axis=0) / profile_dot(dt[todo], dg[todo], dt[todo], dg[todo])))
    return X, fit


# -------------------------------------------------------------------------------------------------------------------- sources
def _as_state(obj, label: str) -> dict:
    if isinstance(obj, dict) and "ema_state_dict" in obj:                                     # a training checkpoint
        obj = obj["ema_state_dict"]
    if not isinstance(obj, dict) or not {"step", "mode", "profiles"} <= set(obj):
        raise ValueError(f"load_sources: {label} is neither a WeightEMA state dict, a snapshot nor a checkpoint with 'ema_state_dict'")
    if "format" in obj and obj["format"] != SNAPSHOT_FORMAT:
        raise ValueError(f"load_sources: {label} has format {obj['format']!r}, expected {SNAPSHOT_FORMAT!r}")
    if obj["mode"] != "power":
        raise ValueError(f"load_sources: {label} holds mode {obj['mode']!r}: a constant-beta average is not a power profile")
    if int(obj["step"]) < 1:
        raise ValueError(f"load_sources: {label} was saved at step {obj['step']}, before the first update")
    if obj.get("gammas") is None or len(obj["gammas"]) != len(obj["profiles"]) or not obj["profiles"]:
        raise ValueError(f"load_sources: {label} holds {len(obj['profiles'])} profiles but gammas = {obj.get('gammas')!r}")
    return dict(obj, step=int(obj["step"]), gammas=[float(g) for g in obj["gammas"]], label=label)


def load_sources(sources) -> List[dict]:
    """Normalise `sources` to a list of WeightEMA state dicts (plus "label" for messages), in the order given.  `sources` is one of, or a
    list of any mix of: a `WeightEMA.save_snapshot` file, a training checkpoint with "ema_state_dict", an in-memory state dict, a
    directory (every ``*.pt`` in it, sorted by name).  Files are read to the host.  Raises ValueError for a constant-beta average or a
    step < 1, and KeyError (names, order) or ValueError (shapes) when the sources do not all hold the same parameters."""
    if isinstance(sources, (str, os.PathLike, dict)):
        sources = [sources]
    out = []
    for i, s in enumerate(sources):
        if isinstance(s, dict):
            out.append(_as_state(s, f"source {i} (dict)"))
            continue
        path = os.fspath(s)
        if os.path.isdir(path):
            files = sorted(f for f in os.listdir(path) if f.endswith(".pt"))
            if not files:
                raise ValueError(f"load_sources: no *.pt file in {path}")
            paths = [os.path.join(path, f) for f in files]
        else:
            paths = [path]
        out.extend(_as_state(torch.load(f, map_location="cpu", weights_only=False), f) for f in paths)
    if not out:
        raise ValueError("load_sources: no source given")
    first = out[0]["profiles"][0]
    names = list(first.keys())
    for st in out:
        for prof in st["profiles"]:
            if list(prof.keys()) != names:
                diff = sorted(set(prof.keys()) ^ set(names))
                raise KeyError(f"load_sources: parameter names of {st['label']} differ from {out[0]['label']}: {diff[:4]}" if diff else
                               f"load_sources: parameter order of {st['label']} differs from {out[0]['label']}")
            for n in names:
                if tuple(prof[n].shape) != tuple(first[n].shape):
                    raise ValueError(f"load_sources: shape of '{n}' in {st['label']} is {tuple(prof[n].shape)}, "
                                     f"in {out[0]['label']} {tuple(first[n].shape)}")
    return out


# -------------------------------------------------------------------------------------------------------------------- result
class ReconstructedEMA(_Profiles):
    """Averages rebuilt by `reconstruct`: `WeightEMA`'s reading interface (`swapped`, `profile_state_dict`, `copy_to`, same semantics)
    over any number of targets.  There is nothing to update.

    sigma_rels, gammas   the targets, in the order asked for
    step                 the training step they are averages up to
    weights              fp64 [nsrc][ntargets]: weight of every (snapshot, profile) source, sources in `load_sources` order
    fit_error            fp64 [ntargets], see `solve_weights`"""

    def __init__(self, model: torch.nn.Module, sigma_rels: Sequence[float], gammas: Sequence[float], step: int, weights: np.ndarray,
                 fit_error: np.ndarray):
        self.sigma_rels, self.gammas, self.step = list(sigma_rels), list(gammas), int(step)
        self.weights, self.fit_error = weights, fit_error
        self._track(model, len(self.gammas))


def _alloc(what: str, nbuf: int, numel: int, make):
    try:
        return make()
    except torch.OutOfMemoryError as e:
        raise RuntimeError(f"posthoc.reconstruct: {what} need {nbuf} x {4 * numel} = {4 * numel * nbuf} bytes of device memory, all resident "
                           f"at once (there is no streaming path): {e}") from e


@torch.no_grad()
def reconstruct(model: torch.nn.Module, sources, sigma_rels: Sequence[float], step: Optional[int] = None) -> ReconstructedEMA:
    """The power-function averages `sigma_rels` of `model`'s parameters at training step `step` (default: the last saved step), rebuilt
    from `sources` (see `load_sources`).  `model` gives the device, the parameter order and the shapes; they must match the sources
    (KeyError / ValueError as in `WeightEMA.load_state_dict`).  Every saved profile that carries weight is copied to the device, all at
    once, combined by `hdmoe_mt_combine` in groups of up to 8 targets, and freed.  Syncs (host copies)."""
    sigma_rels = [float(s) for s in sigma_rels]
    if not sigma_rels:
        raise ValueError("posthoc.reconstruct: sigma_rels is empty")
    gammas = [sigma_rel_to_gamma(s) for s in sigma_rels]
    states = load_sources(sources)
    src = [(st, k) for st in states for k in range(len(st["profiles"]))]
    src_steps = [st["step"] for st, _ in src]
    step = max(src_steps) if step is None else int(step)
    X, fit = solve_weights(src_steps, [st["gammas"][k] for st, k in src], [step] * len(gammas), gammas)
    numel = max(sum((p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN for p in model.parameters() if p.is_floating_point()), 1)
    rec = _alloc("the targets", len(gammas), numel, lambda: ReconstructedEMA(model, sigma_rels, gammas, step, X, fit))
    assert rec._flat_numel == numel
    rec._check_saved([st["profiles"][0] for st in states], "posthoc.reconstruct")
    used = [i for i in range(len(src)) if np.any(X[i] != 0.0)]               # an exact one-hot target needs its own source only
    if len(used) > MAX_SOURCES:
        raise ValueError(f"posthoc.reconstruct: {len(used)} saved profiles, at most {MAX_SOURCES} can be combined")
    dev = rec.device

    def pack():
        bufs = []
        for i in used:
            st, k = src[i]
            host = torch.zeros(numel, dtype=torch.float32)
            for n, o in zip(rec.names, rec._offs):
                v = st["profiles"][k][n]
                host[o:o + v.numel()].copy_(v.reshape(-1))
            bufs.append(host.to(dev))
        return bufs

    bufs = _alloc("the sources", len(used), numel, pack)
    src_table = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64).to(dev)
    for g0 in range(0, len(gammas), MAX_TARGETS_PER_LAUNCH):
        flats = rec._flat[g0:g0 + MAX_TARGETS_PER_LAUNCH]
        dst_table = torch.tensor([f.data_ptr() for f in flats], dtype=torch.int64).to(dev)
        w = torch.from_numpy(np.ascontiguousarray(X[used, g0:g0 + len(flats)])).to(dev)
        call("hdmoe_mt_combine", src_table, dst_table, len(bufs), len(flats), numel, w)
    del bufs                                                                  # (stream-ordered: the allocator reuses them behind the launches)
    return rec
