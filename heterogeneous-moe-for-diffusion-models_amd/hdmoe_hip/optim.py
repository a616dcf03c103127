"""Fused optimizer side of a training iteration (row N3): multi-tensor gradient-norm clipping and AdamW in HIP.

Drop-in for the two lines of the reference loop (Utils/training.py:195-196)

    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)   ->  hdmoe_hip.optim.clip_grad_norm_(model.parameters(), 1.0)
    optimizer.step()                                           ->  FusedAdamW(...).step()

`FusedAdamW` subclasses ``torch.optim.Optimizer`` (param_groups, ``state_dict()`` in torch.optim.AdamW's layout -- so the
reference's ``save_checkpoint`` output stays loadable by either implementation -- and LR schedulers keep working).  The whole
update is one launch over a (tensor, chunk) table; ``step(clip=(params, max_norm))`` additionally fuses the clip coefficient
into the update so norm -> clip -> update never syncs with the host.
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from ._lib import call, lib

_DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("step", "<u8"), ("use", "<u8"), ("numel", "<i8"), ("group", "<i4"),
                  ("pad0", "<i4")])
_CHUNK = 4096


class _Table:
    """Device-side (tensor, chunk) table over a list of parameters that currently have gradients."""

    def __init__(self, entries, steps=None, uses=None):
        """entries: list of (param, grad, m or None, v or None, group); steps: per-entry device float step counters; uses: per-entry device
        address of a float "received a gradient this step" flag (0 = always)."""
        assert lib().hdmoe_opt_desc_bytes() == _DESC.itemsize
        dev = entries[0][0].device
        descs = np.zeros(len(entries), dtype=_DESC)
        chunks = []
        for i, (p, g, m, v, grp) in enumerate(entries):
            d = descs[i]
            d["p"], d["g"] = p.data_ptr(), g.data_ptr()
            d["m"], d["v"] = (0 if m is None else m.data_ptr()), (0 if v is None else v.data_ptr())
            d["step"] = 0 if steps is None else steps[i].data_ptr()
            d["use"] = 0 if uses is None else uses[i]
            d["numel"], d["group"] = p.numel(), grp
            chunks.extend((i, c) for c in range((p.numel() + _CHUNK - 1) // _CHUNK))
        self.descs = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).contiguous().to(dev)
        self.n = len(chunks)
        self.ntensors = len(entries)
        self.ws = torch.empty(max(self.n, 1), dtype=torch.float32, device=dev)          # per-chunk partial sums of the deterministic norm
        self.sig = tuple((p.data_ptr(), g.data_ptr()) for p, g, _, _, _ in entries) + tuple(uses or ())


_norm_tables = {}


def _grad_entries(params):
    out = []
    for p in params:
        if p.grad is not None:
            if p.dtype != torch.float32 or not p.grad.is_contiguous():
                raise TypeError("hdmoe_hip.optim handles contiguous float32 parameters/gradients")
            out.append((p, p.grad, None, None, 0))
    return out


def grad_norm_sq(params: Iterable[torch.nn.Parameter], key=None) -> Tuple[torch.Tensor, Optional[_Table]]:
    ents = _grad_entries(list(params))
    dev = ents[0][0].device if ents else torch.device("cuda")
    out = torch.empty(1, dtype=torch.float32, device=dev)
    if not ents:
        out.zero_()
        return out, None
    sig = tuple((p.data_ptr(), g.data_ptr()) for p, g, _, _, _ in ents)
    tab = _norm_tables.get(key) if key is not None else None
    if tab is None or tab.sig != sig:
        tab = _Table(ents)
        if key is not None:
            _norm_tables[key] = tab
    call("hdmoe_mt_sumsq", out, tab.descs, tab.chunks, tab.n, tab.ws)
    return out, tab


MAX_HEALTH_GROUPS = 64                       # hdmoe_mt_stats: 1 <= ngroups <= 64
STATS_GRAD, STATS_PARAM = 0, 1               # HDMOE_STATS_GRAD / HDMOE_STATS_PARAM (include/hdmoe.h)
_STATS_WS_PER_CHUNK = 6                      # HDMOE_STATS_WS_PER_CHUNK


def health_groups(model: torch.nn.Module):
    """Statistics groups of an HDMOEM model (or its preconditioning wrapper): ``(names, group_of)``.

    `names`: ``Unet_experts.0 .. E-1``, ``VIT_experts.0 .. E-1``, ``Unet_router``, ``vit_router``, ``cross_attn``, ``scaling_net`` when
    the model has one, ``other``.  `group_of`: one index into `names` per parameter, in ``model.parameters()`` order -- every parameter
    lies in exactly one group (what no named component holds is ``other``).  Pure Python: works on a CPU model.  More than 64 groups
    (the statistics kernel's limit) raises ValueError."""
    net = getattr(model, "net", model)
    names, owner = [], {}

    def add(name, module):
        names.append(name)
        for p in module.parameters():
            owner.setdefault(id(p), len(names) - 1)

    for lst in ("Unet_experts", "VIT_experts"):
        for e, expert in enumerate(getattr(net, lst, None) or ()):
            add(f"{lst}.{e}", expert)
    for name in ("Unet_router", "vit_router", "cross_attn"):
        mod = getattr(net, name, None)
        if mod is None:
            names.append(name)
        else:
            add(name, mod)
    if getattr(net, "scaling_net", None) is not None:
        add("scaling_net", net.scaling_net)
    names.append("other")
    if len(names) > MAX_HEALTH_GROUPS:
        raise ValueError(f"health_groups: {len(names)} groups, the statistics pass handles up to {MAX_HEALTH_GROUPS}")
    other = len(names) - 1
    return names, [owner.get(id(p), other) for p in model.parameters()]


class GradHealth:
    """Per-group statistics and the finite-or-not verdict of a parameter list, one `hdmoe_mt_stats` pass per measurement.

    `params`: the parameters (those with a gradient enter the table, in this order, as in `grad_norm_sq`; the table is rebuilt when a
    pointer changes).  `group_of`: one group index per parameter; `names`: the group names (1..64).  The gradient rows, the parameter
    rows, the verdict and the counters live in ONE device allocation, so `read()` is one device-to-host copy:

        counts_g (G+1, 2) i64 | counts_p (G+1, 2) i64 | counters (4,) i64 | stats_g (G+1, 4) f32 | stats_p (G+1, 4) f32 | ok (1,) i32

    ``total_sumsq`` -- the 1-element view of the gradient total's sum of squares -- is what the clip of ``FusedAdamW.step(clip=...,
    health=self)`` reads: for gradients without a non-finite element it equals `hdmoe_mt_sumsq`'s value bit for bit."""

    def __init__(self, params, group_of, names):
        self.params = list(params)
        self.names = [str(n) for n in names]
        self.group_of = [int(g) for g in group_of]
        G = len(self.names)
        if not 1 <= G <= MAX_HEALTH_GROUPS:
            raise ValueError(f"GradHealth: 1 to {MAX_HEALTH_GROUPS} groups, got {G}")
        if len(self.group_of) != len(self.params):
            raise ValueError(f"GradHealth: {len(self.params)} parameters, {len(self.group_of)} group indices")
        if any(not 0 <= g < G for g in self.group_of):
            raise ValueError(f"GradHealth: group indices must lie in 0..{G - 1}")
        if not self.params:
            raise ValueError("GradHealth: no parameters")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("hdmoe_hip: tensors must live on the GPU (no CPU fallback in the product path)")
        self.ngroups = G
        R = G + 1
        o_cnt_g, o_cnt_p, o_ctr = 0, 16 * R, 32 * R
        o_st_g, o_st_p, o_ok = o_ctr + 32, o_ctr + 32 + 16 * R, o_ctr + 32 + 32 * R
        self._buf = torch.zeros(o_ok + 8, dtype=torch.uint8, device=dev)
        view = lambda off, n, dt, shape: self._buf[off:off + n].view(dt).view(shape)
        self._counts = (view(o_cnt_g, 16 * R, torch.int64, (R, 2)), view(o_cnt_p, 16 * R, torch.int64, (R, 2)))
        self.counters = view(o_ctr, 32, torch.int64, (4,))
        self._stats = (view(o_st_g, 16 * R, torch.float32, (R, 4)), view(o_st_p, 16 * R, torch.float32, (R, 4)))
        self.ok = view(o_ok, 4, torch.int32, (1,))
        self.stats, self.counts = self._stats[0], self._counts[0]          # the gradient rows
        self.total_sumsq = self.stats[G, 1:2]
        empty = torch.tensor([0.0, 0.0, float("inf"), float("-inf")], dtype=torch.float32, device=dev)
        for st in self._stats:                                              # an unmeasured block reads as empty groups
            st.copy_(empty.expand(R, 4))
        self.counters[3] = -1
        self.ok.fill_(1)
        self._host = torch.empty(self._buf.numel(), dtype=torch.uint8).pin_memory()
        self._layout = (o_cnt_g, o_cnt_p, o_ctr, o_st_g, o_st_p, o_ok)
        self._table = self._ws = None

    def covers(self, params) -> bool:
        """True when `params` are this object's parameters: the same tensors in the same order."""
        params = list(params)
        return len(params) == len(self.params) and all(a is b for a, b in zip(params, self.params))

    def _ensure_table(self):
        ents = []
        for p, grp in zip(self.params, self.group_of):
            if p.grad is not None:
                if p.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise TypeError("hdmoe_hip.optim handles contiguous float32 parameters/gradients")
                ents.append((p, p.grad, None, None, grp))
        sig = tuple((p.data_ptr(), g.data_ptr()) for p, g, _, _, _ in ents)
        if self._table is None or self._table.sig != sig:
            self._table = _Table(ents) if ents else None
            n = self._table.n if ents else 0
            self._ws = torch.empty(max(_STATS_WS_PER_CHUNK * n, 1), dtype=torch.float32, device=self._buf.device)
        return self._table

    @torch.no_grad()
    def measure(self, step: int, which: str = "grad", verdict: bool = True) -> None:
        """One pass over the gradients (``which="grad"``) or the parameters (``"param"``) of the tensors that have a gradient: fills that
        block's rows; with `verdict` it also writes ``ok`` and advances the counters (`step` becomes the last-skipped step when the
        verdict is 0).  Two launches on the current stream, no sync, no allocation once the table stands."""
        if which not in ("grad", "param"):
            raise ValueError(f"GradHealth.measure: which is 'grad' or 'param', got {which!r}")
        w = STATS_GRAD if which == "grad" else STATS_PARAM
        tab = self._ensure_table()
        call("hdmoe_mt_stats", self._stats[w], self._counts[w], self.ok if verdict else None, self.counters if verdict else None,
             None if tab is None else tab.descs, None if tab is None else tab.chunks, 0 if tab is None else tab.n, self.ngroups, w,
             int(step), self._ws)

    def read(self) -> dict:
        """Sync and fetch everything with one device-to-host copy.  Returns host values: ``ok``, the counters (``measured``, ``skipped``,
        ``skipped_in_a_row``, ``last_skipped_step``), ``grad_norm`` (the total over the finite gradient elements), ``groups`` (the
        names), and under ``"grad"`` / ``"param"`` the per-group lists ``norm``, ``rms``, ``absmax``, ``mean``, ``nonfinite``, ``numel``
        plus ``"total"``, a dictionary of the same keys for the whole table.  norm, rms, absmax and mean are over the finite elements;
        absmax is 0 and rms / mean are NaN where there is none."""
        self._host.copy_(self._buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        h = self._host.numpy()
        R = self.ngroups + 1
        o_cnt_g, o_cnt_p, o_ctr, o_st_g, o_st_p, o_ok = self._layout
        counters = h[o_ctr:o_ctr + 32].view(np.int64)
        out = {"ok": int(h[o_ok:o_ok + 4].view(np.int32)[0]), "measured": int(counters[0]), "skipped": int(counters[1]),
               "skipped_in_a_row": int(counters[2]), "last_skipped_step": int(counters[3]), "groups": list(self.names)}
        for key, o_st, o_cnt in (("grad", o_st_g, o_cnt_g), ("param", o_st_p, o_cnt_p)):
            st = h[o_st:o_st + 16 * R].view(np.float32).reshape(R, 4).astype(np.float64)
            cn = h[o_cnt:o_cnt + 16 * R].view(np.int64).reshape(R, 2)
            nfin = (cn[:, 1] - cn[:, 0]).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                cols = {"norm": np.sqrt(st[:, 1]), "rms": np.sqrt(st[:, 1] / nfin), "mean": st[:, 0] / nfin,
                        "absmax": np.where(nfin > 0, np.maximum(-st[:, 2], st[:, 3]), 0.0)}
            cols["nonfinite"], cols["numel"] = cn[:, 0], cn[:, 1]
            blk = {k: v[:-1].tolist() for k, v in cols.items()}
            blk["total"] = {k: v[-1].item() for k, v in cols.items()}
            out[key] = blk
        out["grad_norm"] = out["grad"]["total"]["norm"]
        return out


def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (L2): scales the gradients in place, returns the total norm.
    Two launches, no host sync."""
    params = list(parameters) if not isinstance(parameters, torch.Tensor) else [parameters]
    ss, tab = grad_norm_sq(params, key=("clip", id(params[0]) if params else 0, len(params)))
    if tab is not None:
        call("hdmoe_mt_clip_scale", tab.descs, tab.chunks, tab.n, ss, float(max_norm))
    return _sqrt_scalar(ss)


def _sqrt_scalar(ss: torch.Tensor) -> torch.Tensor:
    # the returned total norm is only reported/logged; a 1-element sqrt on the device keeps the call sync-free
    return torch.sqrt(ss)[0]


class FusedAdamW(torch.optim.Optimizer):
    """AdamW over all parameters in two launches (global-norm clip + update), ``torch.optim.AdamW``'s state_dict layout.

    Every tensor keeps its own step counter (``state[p]["step"]``, a device float as in torch's capturable mode) and the bias corrections
    are computed from it on the device.  An expert that received no sample in a step has ``.grad is None`` in the reference
    (`if not mask.any(): continue`, models/model_config1.py:26-29) and torch.optim.AdamW then skips its tensors: no weight decay, no
    moment decay, no step increment (Utils/training.py:195-197).  Here such an expert's gradient is an exact zero in its flat-bucket
    view instead, so the skip is driven by the dispatch plan: ``track_expert_usage`` registers the expert lists, the model's forward
    leaves the per-expert routed-row counts of the step in ``<ModuleList>._hdmoe_usage`` (device floats; averaged over the ranks
    with the gradients, hdmoe_hip/dp.py), and the update kernel skips a tensor whose expert's count is 0."""
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > 8:
            raise ValueError("FusedAdamW supports up to 8 parameter groups")
        if len({tuple(g["betas"]) for g in self.param_groups}) > 1 or len({g["eps"] for g in self.param_groups}) > 1:
            raise ValueError("FusedAdamW needs the same betas/eps in every group (lr and weight_decay may differ)")
        self._table = None
        self._usage = {}                                     # id(param) -> (expert ModuleList, expert index)

    def track_expert_usage(self, expert_lists) -> None:
        """``expert_lists``: ModuleLists of experts (HDMOEM.Unet_experts / VIT_experts).  Their parameters are updated only in steps in
        which the expert received at least one sample (on any rank)."""
        for lst in expert_lists:
            for e, expert in enumerate(lst):
                for p in expert.parameters():
                    self._usage[id(p)] = (lst, e)
        self._table = None

    def _use_ptr(self, p) -> int:
        src = self._usage.get(id(p))
        if src is None:
            return 0
        u = getattr(src[0], "_hdmoe_usage", None)            # written by the model's forward (models/_assembly.py _dispatch_nhwc)
        return 0 if u is None else u.data_ptr() + 4 * src[1]

    def zero_grad(self, set_to_none: bool = False):
        """Zero the gradients IN PLACE.  torch's default (set_to_none=True) would detach the flat DP bucket views / the weight bank's
        gradient buffers that the backward kernels accumulate into (the all-reduce would then run on stale buffers), so it is
        only honoured when asked for explicitly."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    p.grad.zero_()

    def _ensure_state(self):
        ents = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif st["step"].device != p.device or st["step"].dtype != torch.float32:   # a checkpoint written by torch.optim.AdamW (host counters)
                    st["step"] = st["step"].to(device=p.device, dtype=torch.float32)
                ents.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"], gi))
        uses = tuple(self._use_ptr(p) for p, *_ in ents)
        sig = tuple((p.data_ptr(), g.data_ptr()) for p, g, _, _, _ in ents) + uses
        if self._table is None or self._table.sig != sig:
            self._table = _Table(ents, [self.state[p]["step"] for p, *_ in ents], uses) if ents else None
        return ents

    @torch.no_grad()
    def step(self, closure=None, clip: Optional[Tuple[Iterable[torch.nn.Parameter], float]] = None, health: Optional[GradHealth] = None):
        """One AdamW update.  ``clip=(parameters, max_norm)`` fuses clip_grad_norm_ over `parameters` into the update
        (gradients themselves are left unscaled).

        ``health=h`` (needs `clip`; `h` a `GradHealth` over exactly the clip's parameters whose ``measure()`` ran on this step's
        gradients): the clip reads ``h.total_sumsq`` instead of launching its own norm pass, and the update is guarded by ``h.ok`` on
        the device -- a step whose gradients hold a non-finite element, or whose norm overflows, writes nothing: no weight decay, no
        moment decay, no step increment.  A step with a good verdict is the unguarded step bit for bit.  The routed-row counters are
        cleared either way: they belong to the step's forwards."""
        if health is not None:                                # in front of any device work
            if clip is None:
                raise ValueError("FusedAdamW.step: health needs clip=(parameters, max_norm), the list the verdict is about")
            clip = (list(clip[0]), clip[1])
            if not health.covers(clip[0]):
                raise ValueError("FusedAdamW.step: health was built over another parameter list than clip's (same tensors, same order)")
        loss = closure() if closure is not None else None
        ents = self._ensure_state()
        if not ents:
            return loss
        ss, max_norm = None, 0.0
        if clip is not None:
            ss = health.total_sumsq if health is not None else grad_norm_sq(clip[0], key=("step", id(self)))[0]
            max_norm = float(clip[1])
        g0 = self.param_groups[0]
        from . import bank as _bank
        _bank.note_weights_changed()                          # (the kernel writes the parameters through raw pointers: Tensor._version stays)
        args = (self._table.descs, self._table.chunks, self._table.n, self._table.ntensors, ss, max_norm,
                [g["lr"] for g in self.param_groups], [g["weight_decay"] for g in self.param_groups], len(self.param_groups),
                g0["betas"][0], g0["betas"][1], g0["eps"])
        if health is not None:
            call("hdmoe_mt_adamw_ok", *args, health.ok)
        else:
            call("hdmoe_mt_adamw", *args)
        self.clear_usage()
        return loss

    def clear_usage(self) -> None:
        """The routed-row counters of the tracked expert lists accumulate over the forwards of a step (models/_assembly.py): start the
        next one at zero.  `step` ends with it; whoever runs forwards that belong to no step (a capture's warm-ups) calls it too."""
        seen = set()
        for lst, _ in self._usage.values():
            if id(lst) not in seen:
                seen.add(id(lst))
                u = getattr(lst, "_hdmoe_usage", None)
                if u is not None:
                    u.zero_()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table = None
