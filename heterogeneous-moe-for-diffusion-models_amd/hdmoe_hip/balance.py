"""Auxiliary-loss-free load balancing of the noisy top-k routers by a per-expert selection bias.

Each `models.model_components.Router` carries a bias that is added to its scores for the top-k selection only (csrc/router.hip,
hdmoe_router_head_bias_fwd): the gate probabilities, the logits the losses read and the k gate weights never see it, so it has no
gradient and nothing of the loss changes.  The head counts, per step and in integers, the rows it routed to every expert (``load``) and
every expert's fair share of the rows whose mask allows it (``target``, in units of 2^-20 row); behind the optimizer step one launch per
router moves the bias by a fixed ``rate`` towards the under-loaded experts, re-centres it and clamps it (hdmoe_balance_bias_update).
The sign decision compares integers whose sums do not depend on the order of the atomics: it is reproducible run to run and, the
accumulators being sum-all-reduced by `hdmoe_hip.dp.GradBuckets.finish`, identical on every data-parallel rank.

Nothing here syncs.  The bias lives in a non-persistent buffer: ``model.state_dict()`` keeps the reference's layout, the EMA (which
averages parameters) does not touch it, and `state_dict()` / `load_state_dict()` below carry it through a checkpoint.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from . import ops


def routers_of(model: torch.nn.Module) -> List[Tuple[str, torch.nn.Module]]:
    """(name, module) of every top-k router of `model`, in registration order (HDMOEM: net.Unet_router, net.vit_router)."""
    return [(n, m) for n, m in model.named_modules() if callable(getattr(m, "enable_balance", None))]


def balanced_routers(model: torch.nn.Module) -> List[Tuple[str, torch.nn.Module]]:
    """Those of `routers_of` whose balancing is enabled (they hold the bias and the two accumulators)."""
    return [(n, m) for n, m in routers_of(model) if "balance_bias" in m._buffers]


class RouterBalance:
    """``RouterBalance(model, rate, bias_max=8.0)`` enables the selection bias on every router of `model` (after the model has been moved
    to its device) and owns the update.

    ``step(ok=None)``: one launch per router behind the optimizer step.  ``ok``: the device verdict of a guarded step
    (`hdmoe_hip.optim.GradHealth.ok`); where it reads 0 the bias stays bit for bit, the step's counts are still cleared.
    ``last()``: {router name: {"bias", "load", "target"}}, the device tensors behind the last `step` (load / target: that step's counts,
    int64; target in units of 2^-20 row).  ``read()``: the same as host lists (it syncs).
    ``clear()``: zero the accumulators (forwards that belong to no step: the warm-up runs of a graph capture)."""

    def __init__(self, model: torch.nn.Module, rate: float, bias_max: float = 8.0):
        for key, val in (("rate", rate), ("bias_max", bias_max)):
            if isinstance(val, bool) or not isinstance(val, (int, float)) or not math.isfinite(val) or val <= 0:
                raise ValueError(f"RouterBalance: {key} must be a finite number > 0, got {val!r}")
        self.rate, self.bias_max = float(rate), float(bias_max)
        self.routers = routers_of(model)
        if not self.routers:
            raise ValueError("RouterBalance: the model has no top-k router")
        self._last = {}
        for name, r in self.routers:
            r.enable_balance()
            acc = r._buffers["balance_load"]
            self._last[name] = (torch.zeros_like(acc), torch.zeros_like(acc))

    def step(self, ok: Optional[torch.Tensor] = None) -> None:
        for name, r in self.routers:
            b = r._buffers
            ll, lt = self._last[name]
            ops.balance_bias_update(b["balance_bias"], b["balance_load"], b["balance_target"], ll, lt, ok, self.rate, self.bias_max)

    def clear(self) -> None:
        for _, r in self.routers:
            r._buffers["balance_load"].zero_()
            r._buffers["balance_target"].zero_()

    def last(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return {name: {"bias": r._buffers["balance_bias"], "load": self._last[name][0], "target": self._last[name][1]}
                for name, r in self.routers}

    def read(self) -> Dict[str, Dict[str, list]]:
        return {name: {k: v.detach().cpu().tolist() for k, v in d.items()} for name, d in self.last().items()}

    def state_dict(self) -> dict:
        return {"rate": self.rate, "bias_max": self.bias_max,
                "bias": {name: r._buffers["balance_bias"].detach().cpu().clone() for name, r in self.routers}}

    def load_state_dict(self, state: dict) -> None:
        """Restores the biases in place (a captured step reads them by pointer); rate and bias_max stay this object's."""
        bias = state["bias"]
        names = [name for name, _ in self.routers]
        if sorted(bias) != sorted(names):
            raise ValueError(f"RouterBalance.load_state_dict: the state holds the routers {sorted(bias)}, the model {sorted(names)}")
        for name, r in self.routers:
            dst = r._buffers["balance_bias"]
            if tuple(bias[name].shape) != tuple(dst.shape):
                raise ValueError(f"RouterBalance.load_state_dict: {name}: {tuple(bias[name].shape)} entries for {tuple(dst.shape)} experts")
            dst.copy_(bias[name].to(dst.dtype))
