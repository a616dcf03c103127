"""Held-out evaluation on the device: per-noise-level denoising error and the routing map of both routers.

The reference has no validation pass: its only quality signal is the training loss of the current batch (random sigma, router masks,
dropout, raw weights), and its expert-specialisation plot (``graphs/plotter.py`` plot_expert_specialization_advanced) probes the routers
with a dummy input.  `Evaluator` runs the model forward only, in eval mode, over a `LatentDataset` at FIXED sigma levels with noise
keyed by (seed, item, level) -- csrc/evalstats.hip, RNG contract in include/hdmoe.h -- so the numbers belong to the weights alone: two
checkpoints see the same items, the same noise and the same sigma grid.  Per level it accumulates, on the device and without atomics,
the denoising error and the gate probabilities of both routers; the host reads one table at the end.

A batch is three library launches around the forward (`ops.eval_inputs`, the text gather, `ops.eval_accumulate`), all capturable: with
``graphed=True`` an evaluation is ``rounds * ceil(n / B)`` replays of one hipGraph with no sync between them.
"""
from __future__ import annotations

import contextlib
import inspect
import math
import statistics
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .utils import LatentDataset, _null_row, model_extras, null_text

MAX_LEVELS, MAX_BATCH = 64, 4096


def default_levels(K: int, p_mean: float, p_std: float, sigma_min: float, sigma_max: float) -> list:
    """The K mid-quantiles of the training log-normal, sigma_k = exp(p_mean + p_std * Phi^-1((k + 1/2) / K)), clamped to
    [sigma_min, sigma_max]: level k sits at percentile (k + 1/2) / K of the axis the mask generators' expert centres live on."""
    nd = statistics.NormalDist()
    return [min(max(math.exp(p_mean + p_std * nd.inv_cdf((k + 0.5) / K)), sigma_min), sigma_max) for k in range(K)]


def rank_slice(N: int, world: int, rank: int) -> Tuple[int, int]:
    """(first, count) of the contiguous slice of range(N) that `rank` of `world` evaluates: disjoint, covering, sizes within one."""
    return rank * N // world, (rank + 1) * N // world - rank * N // world


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


class Evaluator:
    """``Evaluator(model, model_config, mask_config, dataset, batch_size)`` measures `model` on the items of `dataset`
    (`Utils.utils.LatentDataset` with text rows); ``evaluate()`` returns the per-level numbers.

    ``levels``: an int K = the K mid-quantiles of the training log-normal (`default_levels`), or a sequence of positive sigmas used as
    given; 1 <= K <= 64.  Item i is evaluated at level (i + r) % K in round r = 0 .. ``rounds`` - 1 (1 <= rounds <= K): with rounds = K
    every (item, level) pair is visited exactly once.  ``seed`` keys the noise.  ``graphed=True`` captures the batch through
    `hdmoe_hip.graph.GraphedStep` at the first ``evaluate()``; False runs the same function eagerly, with bit-identical results.
    ``ema``: a `hdmoe_hip.ema.WeightEMA` of `model` for ``evaluate(profile=k)``.  ``null_text_emb``: the null row the model was trained
    with (None: zeros) for ``evaluate(text="null")``.  ``world`` / ``rank`` default to the process group's if one is initialised,
    otherwise (1, 0): rank r evaluates a contiguous slice of the items, the tables are summed over the group.

    The forward runs under ``torch.no_grad()`` in eval mode, with all-ones router masks and zeta 0.  Evaluation is invisible to
    training: the model's mode, the optimizer's routed-row counters and the library's seed stream are left as found, and no parameter
    or gradient buffer is written.  ValueError names the argument of every violated condition before any device work."""

    def __init__(self, model, model_config, mask_config, dataset: LatentDataset, batch_size: int, *, levels: Union[int, Sequence[float]] = 16,
                 rounds: int = 1, seed: int = 0, graphed: bool = True, ema=None, null_text_emb: Optional[torch.Tensor] = None,
                 world: Optional[int] = None, rank: Optional[int] = None):
        if not isinstance(dataset, LatentDataset):
            raise ValueError(f"Evaluator: dataset is a Utils.utils.LatentDataset, got {type(dataset).__name__}")
        if dataset.text is None:
            raise ValueError("Evaluator: the dataset needs text rows (LatentDataset(text=...)): the model is text-conditioned")
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or not 1 <= batch_size <= MAX_BATCH:
            raise ValueError(f"Evaluator: batch_size is an int in [1, {MAX_BATCH}], got {batch_size}")
        if isinstance(levels, bool):
            raise ValueError("Evaluator: levels is an int K or a sequence of positive sigmas, got a bool")
        if isinstance(levels, int):
            if not 1 <= levels <= MAX_LEVELS:
                raise ValueError(f"Evaluator: levels = K needs 1 <= K <= {MAX_LEVELS}, got {levels}")
            sig = default_levels(levels, mask_config["p_mean"], mask_config["p_std"], model_config["sigma_min"], model_config["sigma_max"])
        else:
            try:
                sig = [float(v) for v in levels]
            except (TypeError, ValueError):
                raise ValueError(f"Evaluator: levels is an int K or a sequence of positive sigmas, got {type(levels).__name__}") from None
            if not 1 <= len(sig) <= MAX_LEVELS:
                raise ValueError(f"Evaluator: levels holds {len(sig)} sigmas, 1 <= K <= {MAX_LEVELS}")
            if not all(math.isfinite(v) and v > 0.0 for v in sig):
                raise ValueError(f"Evaluator: levels must be positive and finite, got {sig}")
        K = len(sig)
        if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= K:
            raise ValueError(f"Evaluator: rounds is an int in [1, K] = [1, {K}], got {rounds}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"Evaluator: seed is an int, got {type(seed).__name__}")
        if null_text_emb is not None and not torch.is_tensor(null_text_emb):
            raise ValueError(f"Evaluator: null_text_emb is a tensor of one text row or None, got {type(null_text_emb).__name__}")
        if null_text_emb is not None and tuple(null_text_emb.shape) != tuple(dataset.text.shape[1:]):
            raise ValueError(f"Evaluator: null_text_emb has shape {tuple(null_text_emb.shape)}, a text row is {tuple(dataset.text.shape[1:])}")
        if ema is not None and not (hasattr(ema, "swapped") and hasattr(ema, "nprofiles")):
            raise ValueError(f"Evaluator: ema is a hdmoe_hip.ema.WeightEMA or None, got {type(ema).__name__}")
        if (world is None) != (rank is None):
            raise ValueError("Evaluator: world and rank are given together or not at all")
        if world is None:
            dist = torch.distributed.is_available() and torch.distributed.is_initialized()
            world, rank = (torch.distributed.get_world_size(), torch.distributed.get_rank()) if dist else (1, 0)
        if isinstance(world, bool) or not isinstance(world, int) or isinstance(rank, bool) or not isinstance(rank, int) \
                or world < 1 or not 0 <= rank < world:
            raise ValueError(f"Evaluator: world >= 1 and rank in [0, world), got world={world}, rank={rank}")
        self.model, self.cfg, self.mask_cfg, self.dataset = model, model_config, mask_config, dataset
        self.batch_size, self.sigmas, self.K, self.rounds, self.seed = batch_size, sig, K, rounds, seed & 0xFFFFFFFFFFFFFFFF
        self.graphed, self.ema, self.null_text_emb = bool(graphed), ema, null_text_emb
        self.world, self.rank = world, rank
        self.first, self.n_rank = rank_slice(dataset.N, world, rank)
        self.E = int(model_config["num_experts"])
        self.sigma_data = float(model_config["sigma_data"])
        self._model_extra = model_extras(model, mask_config)
        if "return_log_var" in inspect.signature(model.forward).parameters:
            self._model_extra["return_log_var"] = True
        self.buf = None                                      # static buffers, allocated by the first evaluate()
        self._step = None                                    # hdmoe_hip.graph.GraphedStep of the batch
        self._text_mode = None

    # ------------------------------------------------------------------------------------------------------------ the batch
    def _alloc(self) -> None:
        from hdmoe_hip import ops
        ds, B, dev = self.dataset, self.batch_size, self.dataset.device
        shape = (B,) + tuple(ds.mean.shape[1:])
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.buf = {"x": torch.zeros(shape, **f32), "x0": torch.zeros(shape, **f32), "sigma": torch.zeros(B, 1, 1, 1, **f32),
                    "level": torch.zeros(B, **i32), "item": torch.zeros(B, **i32), "keep": torch.zeros(B, **f32),
                    "text": torch.zeros((B,) + tuple(ds.text.shape[1:]), dtype=ds.text.dtype, device=dev),
                    "levels": torch.tensor(self.sigmas, **f32), "umask": torch.ones(B, self.E, **f32), "vmask": torch.ones(B, self.E, **f32),
                    "acc": torch.zeros(self.K, 6 + 4 * self.E, dtype=torch.float64, device=dev),
                    "ws": torch.zeros(ops.eval_ws_floats(B, ds.mean[0].numel()), **f32)}
        self._null = _null_row(self.null_text_emb, ds.text)

    def _inputs(self, rnd: int, first: int, count: int) -> None:
        """The batch's inputs into the static buffers.  round, first and count are launch scalars, so -- like `Trainer._batch` in front
        of its captured step -- these launches are enqueued eagerly in front of every replay; nothing syncs."""
        from hdmoe_hip import ops
        b, ds = self.buf, self.dataset
        ops.eval_inputs(b["x"], b["x0"], b["sigma"], b["level"], b["item"], ds.mean, b["levels"], self.seed, rnd, first, count, scale=ds.scale)
        if self._text_mode == "cond":                        # the existing gather at p = 0: a pure gather, `keep` all ones
            ops.text_gather_dropout(b["text"], b["keep"], ds.text, ds.text_index, b["item"], self._null, self.seed, 0, 0.0, ds.N)

    def _forward_accumulate(self) -> None:
        from hdmoe_hip import ops
        b = self.buf
        with torch.no_grad():
            out = self.model(x=b["x"], sigma=b["sigma"], text_emb=b["text"], Unet_router_mask=b["umask"], Vit_router_mask=b["vmask"], zeta=0.0,
                             **self._model_extra)
            lv = out.get("log_var")
            ops.eval_accumulate(b["acc"], b["ws"], _f32c(out["denoised"]), b["x0"], b["sigma"], b["level"],
                                None if lv is None else _f32c(lv).reshape(-1), _f32c(out["Unet_router_loss"]), _f32c(out["vit_router_loss"]),
                                self.sigma_data)

    def _batches(self):
        """(round, first item, valid rows) of every batch of this rank, in order."""
        B = self.batch_size
        for rnd in range(self.rounds):
            for off in range(0, self.n_rank, B):
                yield rnd, self.first + off, min(B, self.n_rank - off)

    # ------------------------------------------------------------------------------------------------------------ evaluate
    @contextlib.contextmanager
    def _untouched(self):
        """Everything a forward leaves behind outside its outputs, put back on exit: the train / eval mode, the routed-row counters that
        `FusedAdamW.track_expert_usage` reads (a forward adds into them), the library's seed stream (host counter and device step
        counter: GraphedStep's warm-ups and the captured batch advance them)."""
        from hdmoe_hip import ops
        model, dev = self.model, self.dataset.device
        was_training = model.training
        usage = [(u, u.clone()) for u in (getattr(m, "_hdmoe_usage", None) for m in model.modules()) if torch.is_tensor(u)]
        host_seed = dict(ops._seed_state)
        ctr = ops.step_counter(dev)
        ctr_was = ctr.clone()
        try:
            model.eval()
            yield
        finally:
            model.train(was_training)
            for u, saved in usage:
                u.copy_(saved)
            for m in model.modules():                        # a counter the evaluation itself installed: nothing of it was the optimizer's
                u = getattr(m, "_hdmoe_usage", None)
                if torch.is_tensor(u) and not any(u is v for v, _ in usage):
                    u.zero_()
            ctr.copy_(ctr_was)
            ops._seed_state.update(host_seed)

    def _run(self) -> None:
        from hdmoe_hip import graph as hgraph
        bank = getattr(self.model, "_hdmoe_bank", None)
        if bank is not None:                                 # a captured forward holds no weight-prepare launch (EDM_Sampler.sample does the same)
            bank.refresh_eval()
        b = self.buf
        if self.graphed and self._step is None:
            # the capture runs the batch function a few times: on a batch of its own, before the table is zeroed
            rnd, first, count = next(self._batches())
            self._inputs(rnd, first, count)
            self._step = hgraph.GraphedStep(self._forward_accumulate, self.dataset.device)
            bank = getattr(self.model, "_hdmoe_bank", None)
            if bank is not None:
                bank.refresh_eval()
        b["acc"].zero_()                                     # eagerly: a captured memset node is not to be trusted (csrc/loss.hip)
        run = self._step if self.graphed else self._forward_accumulate
        for rnd, first, count in self._batches():
            self._inputs(rnd, first, count)                  # eval_inputs -> forward -> eval_accumulate, no sync in between
            run()

    def evaluate(self, profile: Optional[int] = None, text: str = "cond") -> dict:
        """One pass over this rank's items, `rounds` times: {"sigma", "count", "mse", "mse_stderr", "edm_weighted", "nll", "log_var"} (K,)
        and {"unet_usage", "vit_usage", "unet_selected", "vit_selected"} (K, E) numpy float64 per level -- usage the mean gate
        probability, selected the fraction of samples with a probability > 0 --, the scalars "mse_mean" (count-weighted over the levels)
        and "n", and "acc", the raw (K, 6 + 4E) table summed over the ranks.  A level without samples has count 0 and NaN means.
        ``profile=k``: the weights of EMA profile k (inside ``ema.swapped(k)``).  ``text="null"``: the unconditional branch, every
        sample's text the null row."""
        if text not in ("cond", "null"):
            raise ValueError(f"Evaluator.evaluate: text is 'cond' or 'null', got {text!r}")
        if profile is not None:
            if self.ema is None:
                raise ValueError("Evaluator.evaluate: profile needs an Evaluator built with ema=...")
            if isinstance(profile, bool) or not isinstance(profile, int) or not 0 <= profile < self.ema.nprofiles:
                raise ValueError(f"Evaluator.evaluate: profile must lie in 0..{self.ema.nprofiles - 1}, got {profile}")
        if self.buf is None:
            self._alloc()
        if text != self._text_mode:
            self._text_mode = text
            if text == "null":                               # filled once; the gather is then left out of the batch
                self.buf["text"].copy_(null_text(self.null_text_emb, self.buf["text"]))
        with self._untouched():
            with (self.ema.swapped(profile) if profile is not None else contextlib.nullcontext()):
                self._run()
        acc = self.buf["acc"]
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(acc, op=torch.distributed.ReduceOp.SUM)
        return summarize(acc.cpu().numpy().copy(), self.sigmas, self.E)          # the one host copy


def summarize(acc: np.ndarray, sigmas: Sequence[float], E: int) -> dict:
    """The per-level means of a raw (K, 6 + 4E) table of `hdmoe_eval_accumulate` (host arithmetic only)."""
    acc = np.asarray(acc, dtype=np.float64)
    n = acc[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = lambda col: np.where(n > 0, col / n, np.nan)
        mse = mean(acc[:, 1])
        var = np.maximum(mean(acc[:, 2]) - mse * mse, 0.0)
        res = {"sigma": np.asarray(sigmas, dtype=np.float64), "count": n.copy(), "mse": mse, "mse_stderr": np.sqrt(var / n),
               "edm_weighted": mean(acc[:, 3]), "nll": mean(acc[:, 4]), "log_var": mean(acc[:, 5])}
        for j, key in enumerate(("unet_usage", "unet_selected", "vit_usage", "vit_selected")):
            res[key] = np.where(n[:, None] > 0, acc[:, 6 + j * E:6 + (j + 1) * E] / n[:, None], np.nan)
        total = float(n.sum())
        res["mse_mean"] = float(acc[:, 1].sum() / total) if total > 0 else float("nan")
    res["mse_stderr"] = np.where(n > 0, res["mse_stderr"], np.nan)
    res["n"] = total
    res["acc"] = acc
    return res
