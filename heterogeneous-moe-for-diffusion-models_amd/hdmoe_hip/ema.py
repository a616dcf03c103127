"""Exponential moving average (EMA) of the weights: EDM2 power-function profiles, one fused launch per step.

    ema = WeightEMA(model, sigma_rels=(0.05, 0.10))     # or betas=(0.999,) for the classic constant decay
    ...
    optimizer.step(); ema.update()                       # Trainer(..., ema=ema) does this
    with ema.swapped(0):                                 # the parameters ARE profile 0 in here; restored bit for bit on exit
        images = sampler.sample(...)

The power profile of Karras et al., "Analyzing and Improving the Training Dynamics of Diffusion Models" (EDM2), section 3.1 weights the
iterate of step j in proportion to j^gamma: beta_t = (1 - 1/t)^(gamma + 1), e_t = beta_t e_{t-1} + (1 - beta_t) p_t, with gamma given
through the relative width sigma_rel of the averaging window.  The step count lives on the device and the kernel derives beta from it, so
`update()` takes no host value that changes from step to step: it never syncs, never allocates and can be captured in a hipGraph once.
`ema.save_snapshot(path)` writes the averages to a file; from a few of those `hdmoe_hip.posthoc.reconstruct` rebuilds the average of any
other sigma_rel afterwards.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ._lib import call, lib

MAX_PROFILES = 4
POWER, CONSTANT = 0, 1                      # HDMOE_EMA_POWER / HDMOE_EMA_CONSTANT (include/hdmoe.h)
_DESC = np.dtype([("p", "<u8"), ("e", "<u8", (MAX_PROFILES,)), ("numel", "<i8")])
_CHUNK = 4096
_ALIGN = 64                                 # profile views start on 256-byte boundaries: the kernel's 16-byte path applies whenever p allows it
SIGMA_REL_MAX = 12.0 ** -0.5                # gamma = 0
SNAPSHOT_FORMAT = "hdmoe-ema-snapshot-1"    # WeightEMA.save_snapshot files


def sigma_rel_to_gamma(sigma_rel: float) -> float:
    """Exponent gamma of the power profile whose relative standard deviation is `sigma_rel` (EDM2, algorithm 2):
    sigma_rel^2 = (gamma + 1) / ((gamma + 2)^2 (gamma + 3)), the largest real root of
    gamma^3 + 7 gamma^2 + (16 - sigma_rel^-2) gamma + (12 - sigma_rel^-2)."""
    s = float(sigma_rel)
    if not (0.0 < s <= SIGMA_REL_MAX):
        raise ValueError(f"sigma_rel must lie in (0, 12^-1/2 = {SIGMA_REL_MAX:.6f}] (gamma >= 0), got {sigma_rel!r}")
    t = s ** -2
    roots = np.roots([1.0, 7.0, 16.0 - t, 12.0 - t])
    g = float(max(r.real for r in roots if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real))))
    for _ in range(3):                      # Newton polish of the companion-matrix root
        f = ((g + 7.0) * g + (16.0 - t)) * g + (12.0 - t)
        g -= f / ((3.0 * g + 14.0) * g + (16.0 - t))
    return max(g, 0.0)


def power_beta(gamma: float, t: int) -> float:
    """beta_t = (1 - 1/t)^(gamma + 1) in fp64; 0 at t <= 1 (the first average is the first iterate)."""
    if t <= 1:
        return 0.0
    return math.exp((float(gamma) + 1.0) * math.log1p(-1.0 / float(t)))


class _Profiles:
    """What WeightEMA and posthoc.ReconstructedEMA share: the tracked parameters, flat fp32 profiles in one layout with per-parameter
    views, the kernels' descriptor tables (one per group of four profiles) and the reading interface."""

    def _track(self, model: torch.nn.Module, nprofiles: int) -> None:
        """Collect the parameters and allocate `nprofiles` zero-filled flat profiles (per-parameter offsets rounded up to _ALIGN)."""
        me = type(self).__name__
        self.nprofiles = int(nprofiles)
        self.names, self._params = [], []
        for name, p in model.named_parameters():
            if not p.is_floating_point():
                continue
            if not p.is_cuda:
                raise RuntimeError(f"{me}: parameter '{name}' is not on the GPU (no CPU fallback in the product path)")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError(f"{me} handles contiguous float32 parameters, '{name}' is {p.dtype}")
            self.names.append(name)
            self._params.append(p)
        if not self._params:
            raise ValueError(f"{me}: the model has no floating-point parameter")
        assert lib().hdmoe_ema_desc_bytes() == _DESC.itemsize
        dev = self._params[0].device
        self.device = dev
        self._offs, total = [], 0
        for p in self._params:
            self._offs.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self._flat_numel = max(total, 1)
        self._flat = [torch.zeros(self._flat_numel, dtype=torch.float32, device=dev) for _ in range(self.nprofiles)]
        self._views = [[f[o:o + p.numel()].view(p.shape) for o, p in zip(self._offs, self._params)] for f in self._flat]
        self._descs = self._chunks = None
        self._n, self._sig = 0, None
        self._swapped = None

    # ---------------------------------------------------------------------------------------------------------------- table
    def _table(self, group: int = 0):
        """(tensor, chunk) table on the device for profiles 4 * group .. 4 * group + 3; rebuilt only when a parameter's storage moved
        (same rule as optim._Table)."""
        sig = tuple(p.data_ptr() for p in self._params)
        if sig != self._sig:
            descs = np.zeros(((self.nprofiles + MAX_PROFILES - 1) // MAX_PROFILES, len(self._params)), dtype=_DESC)
            chunks = []
            for i, p in enumerate(self._params):
                descs["p"][:, i], descs["numel"][:, i] = p.data_ptr(), p.numel()
                for k in range(self.nprofiles):
                    descs["e"][k // MAX_PROFILES, i, k % MAX_PROFILES] = self._views[k][i].data_ptr()
                chunks.extend((i, c) for c in range((p.numel() + _CHUNK - 1) // _CHUNK))
            self._descs = [torch.from_numpy(d.view(np.uint8).copy()).to(self.device) for d in descs]
            self._chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).contiguous().to(self.device)
            self._n, self._sig = len(chunks), sig
        return self._descs[group], self._chunks, self._n

    def _check_profile(self, k: int) -> int:
        if not 0 <= int(k) < self.nprofiles:
            raise ValueError(f"profile must lie in 0..{self.nprofiles - 1}, got {k}")
        return int(k)

    def _check_saved(self, profiles, where: str) -> None:
        """Saved profiles ({name: tensor} each) against the tracked parameters: names or order (KeyError), shapes (ValueError)."""
        for prof in profiles:
            if list(prof.keys()) != self.names:
                diff = sorted(set(prof.keys()) ^ set(self.names))
                raise KeyError(f"{where}: parameter names differ {diff[:4]}" if diff else f"{where}: parameter order differs")
            for n, v in zip(self.names, self._views[0]):
                if tuple(prof[n].shape) != tuple(v.shape):
                    raise ValueError(f"{where}: shape of '{n}' is {tuple(prof[n].shape)}, expected {tuple(v.shape)}")

    # ---------------------------------------------------------------------------------------------------------------- reading
    def profile_state_dict(self, k: int = 0) -> Dict[str, torch.Tensor]:
        """{state_dict key: averaged tensor} of profile k (views of the live average, not copies): load it with
        ``model.load_state_dict(..., strict=False)`` -- buffers are not part of it."""
        if self._swapped is not None:
            raise RuntimeError(f"{type(self).__name__}.profile_state_dict() inside swapped(): the profile currently holds the raw parameters")
        k = self._check_profile(k)
        return dict(zip(self.names, self._views[k]))

    def _swap(self, k: int) -> None:
        from . import bank as _bank
        descs, chunks, n = self._table(k // MAX_PROFILES)
        call("hdmoe_mt_swap", descs, chunks, n, k % MAX_PROFILES)
        _bank.invalidate_weights()                           # the kernel writes through raw pointers: Tensor._version stays

    @contextlib.contextmanager
    def swapped(self, profile: int = 0):
        """Inside the context the model's parameters hold profile `profile` and the profile holds the raw parameters (exchanged in
        place, no temporary copy of the model); on exit they are exchanged back, bit for bit.  The cached eval-mode weight images are
        invalidated both times.  `update()` and a nested `swapped` raise inside."""
        k = self._check_profile(profile)
        if self._swapped is not None:
            raise RuntimeError(f"{type(self).__name__}.swapped() cannot be nested")
        with torch.no_grad():
            self._swap(k)
        self._swapped = k
        try:
            yield self
        finally:
            with torch.no_grad():
                self._swap(k)
            self._swapped = None

    @torch.no_grad()
    def copy_to(self, model: torch.nn.Module, profile: int = 0) -> None:
        """One-way export: write profile `profile` into `model`'s parameters (the tracked model or another instance of it)."""
        me = type(self).__name__
        src = self.profile_state_dict(profile)
        dst = dict(model.named_parameters())
        missing = [n for n in src if n not in dst]
        if missing:
            raise KeyError(f"{me}.copy_to: the model lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
        for n, e in src.items():
            if dst[n].shape != e.shape:
                raise ValueError(f"{me}.copy_to: shape of '{n}' is {tuple(dst[n].shape)}, the average has {tuple(e.shape)}")
            dst[n].copy_(e)
        from . import bank as _bank
        _bank.invalidate_weights()


class WeightEMA(_Profiles):
    """Up to four EMA profiles of every floating-point parameter of `model` (``named_parameters()`` order; buffers are not averaged).

    Exactly one of `sigma_rels` (power profiles, the default) and `betas` (constant decay) is used, 1 to 4 entries.  Each profile is one
    flat fp32 allocation with per-parameter views, initialised to the current parameters.

    ``update()`` averages EVERY tracked tensor in EVERY step.  That includes parameters no optimizer group holds (their average simply
    stays equal to them) and -- the one place where the semantics are not obvious -- the tensors of an expert that ``FusedAdamW`` skipped
    because no sample was routed to it in that step: its parameters did not move, its step still counts, and its average keeps converging
    to them.  The average is over training steps, not over the updates a tensor happened to receive."""

    def __init__(self, model: torch.nn.Module, sigma_rels: Optional[Sequence[float]] = (0.05, 0.10), betas: Optional[Sequence[float]] = None):
        if betas is not None:
            betas = [float(b) for b in betas]
            if not 1 <= len(betas) <= MAX_PROFILES:
                raise ValueError(f"betas needs 1 to {MAX_PROFILES} entries, got {len(betas)}")
            if not all(0.0 <= b < 1.0 for b in betas):
                raise ValueError(f"betas must lie in [0, 1), got {betas}")
            self.mode, self.sigma_rels, self.gammas, self.betas = CONSTANT, None, None, betas
            coefs = betas
        else:
            sigma_rels = [float(s) for s in (sigma_rels if sigma_rels is not None else ())]
            if not 1 <= len(sigma_rels) <= MAX_PROFILES:
                raise ValueError(f"sigma_rels needs 1 to {MAX_PROFILES} entries, got {len(sigma_rels)}")
            self.mode, self.sigma_rels, self.betas = POWER, sigma_rels, None
            self.gammas = [sigma_rel_to_gamma(s) for s in sigma_rels]
            coefs = self.gammas
        self._track(model, len(coefs))
        with torch.no_grad():
            for views in self._views:
                torch._foreach_copy_(views, [p.detach() for p in self._params])
        self._step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._coefs = torch.tensor(coefs, dtype=torch.float64, device=self.device)

    # ---------------------------------------------------------------------------------------------------------------- update
    @torch.no_grad()
    def update(self, ok: Optional[torch.Tensor] = None) -> None:
        """Advance the device step count and fold the current parameters into every profile: one launch on the current stream, no sync,
        no allocation (capturable).  Every tracked tensor is updated, also those the optimizer skipped this step (see the class docstring).

        ``ok``: a device int32 verdict (`hdmoe_hip.optim.GradHealth.ok`).  Where it reads 0 the call writes nothing -- the step count
        and every profile stay as they are, like the optimizer step that the same verdict rejected; where it reads non-zero the call is
        the unguarded one bit for bit."""
        if self._swapped is not None:
            raise RuntimeError("WeightEMA.update() inside swapped(): the parameters currently hold an EMA profile")
        if ok is not None and (not torch.is_tensor(ok) or ok.dtype != torch.int32 or ok.numel() < 1 or ok.device != self.device):
            raise ValueError("WeightEMA.update: ok is an int32 tensor on the parameters' device")
        descs, chunks, n = self._table()
        if ok is None:
            call("hdmoe_mt_ema", descs, chunks, n, self.nprofiles, self._step, self._coefs, self.mode)
        else:
            call("hdmoe_mt_ema_ok", descs, chunks, n, self.nprofiles, self._step, self._coefs, self.mode, ok)

    @property
    def step(self) -> int:
        """Number of updates so far.  A host read: it syncs -- for logging and saving only."""
        return int(self._step.item())

    def num_bytes_per_update(self) -> int:
        """Bytes one update moves: p read once, every profile read and written once."""
        return (1 + 2 * self.nprofiles) * 4 * sum(p.numel() for p in self._params)

    # ---------------------------------------------------------------------------------------------------------------- checkpoint
    def state_dict(self) -> dict:
        """Host copies: what a resume, or a later post-hoc reconstruction of other sigma_rel, needs."""
        if self._swapped is not None:
            raise RuntimeError("WeightEMA.state_dict() inside swapped()")
        return {"step": self.step, "mode": "power" if self.mode == POWER else "constant",
                "sigma_rels": None if self.sigma_rels is None else list(self.sigma_rels),
                "gammas": None if self.gammas is None else list(self.gammas),
                "betas": None if self.betas is None else list(self.betas),
                "profiles": [{n: v.detach().cpu().clone() for n, v in zip(self.names, views)} for views in self._views]}

    def save_snapshot(self, path) -> str:
        """Write `state_dict()` plus ``"format": SNAPSHOT_FORMAT`` to `path` with one ``torch.save``: a source for
        `hdmoe_hip.posthoc.reconstruct`.  Copies every profile to the host, so it syncs; it raises inside `swapped()`."""
        if self._swapped is not None:
            raise RuntimeError("WeightEMA.save_snapshot() inside swapped()")
        torch.save(dict(self.state_dict(), format=SNAPSHOT_FORMAT), str(path))
        return str(path)

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        if self._swapped is not None:
            raise RuntimeError("WeightEMA.load_state_dict() inside swapped()")
        mode = {"power": POWER, "constant": CONSTANT}.get(state.get("mode"))
        if mode != self.mode:
            raise ValueError(f"WeightEMA.load_state_dict: the checkpoint's mode is {state.get('mode')!r}, this object is "
                             f"{'power' if self.mode == POWER else 'constant'}")
        coefs = state["gammas"] if mode == POWER else state["betas"]
        profiles = state["profiles"]
        if coefs is None or len(coefs) != self.nprofiles or len(profiles) != self.nprofiles:
            raise ValueError(f"WeightEMA.load_state_dict: the checkpoint holds {len(profiles)} profiles, this object {self.nprofiles}")
        self._check_saved(profiles, "WeightEMA.load_state_dict")
        for views, prof in zip(self._views, profiles):
            for n, v in zip(self.names, views):
                v.copy_(prof[n])
        if mode == POWER:
            self.sigma_rels, self.gammas = (None if state.get("sigma_rels") is None else list(state["sigma_rels"])), [float(g) for g in coefs]
        else:
            self.betas = [float(b) for b in coefs]
        self._coefs.copy_(torch.tensor([float(c) for c in coefs], dtype=torch.float64))     # in place: a captured update keeps reading it
        self._step.fill_(int(state["step"]))
