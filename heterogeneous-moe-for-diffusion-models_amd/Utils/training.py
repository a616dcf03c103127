"""Training iteration and checkpoint format -- the optimizer side of the hot path.

Mirrors reference ``Utils/training.py``: optimizer groups (:55-60), cosine schedule (:62-65), the per-iteration order
forward -> loss -> zero_grad -> backward -> clip_grad_norm_(1.0) -> step -> scheduler.step (:125-197) and the checkpoint
dictionary (:242-271, read back at :303-304).  What the reference takes from the network (Flowers102, the SD VAE, CLIP;
``Utils/VAE_CLIP.py``) is outside this path: `train_steps` is fed latents and text embeddings by the caller, or the trainer draws them
itself from a device-resident `Utils.utils.LatentDataset` of pre-encoded latents and text rows.

Differences that are deliberate and visible:
  * gradient clipping + AdamW run as two multi-tensor HIP launches with no host sync (hdmoe_hip/optim.py);
  * the reference's router group reads ``model.net.routers`` (:59), an attribute that exists nowhere in the reference
    either; the two routers ``[net.Unet_router, net.vit_router]`` are used;
  * under torch.distributed the gradient all-reduce is the flat-bucket RCCL path of hdmoe_hip/dp.py.
"""
from __future__ import annotations

import collections
import math
import os
from typing import Any, Callable, Dict, Iterable, Optional, Union

import torch

from hdmoe_hip.dp import GradBuckets
from hdmoe_hip.optim import FusedAdamW
from .utils import EDM_LOSS, DeviceInputs, LatentDataset, MaskGenerator, ZetaScheduler, model_extras, null_text, sample_sigma_hybrid


def build_optimizer(model: torch.nn.Module, optim_config: Dict[str, Any]) -> FusedAdamW:
    """The reference's four AdamW groups (training.py:55-60): U-Net experts, ViT experts (boosted), fusion cross-attention,
    routers.  Like the reference, parameters outside these groups (stem, gates, text cross-attention, output conv,
    scaling_net, log-var head) are not optimised."""
    net = model.net
    routers = list(net.Unet_router.parameters()) + list(net.vit_router.parameters())
    opt = FusedAdamW([
        {"params": list(net.Unet_experts.parameters()), "lr": optim_config["lr_unet"]},
        {"params": list(net.VIT_experts.parameters()), "lr": optim_config["lr_vit"]},
        {"params": list(net.cross_attn.parameters()), "lr": optim_config["lr_attn"]},
        {"params": routers, "lr": optim_config["lr_router"]},
    ])
    # an expert without a sample in a step is left out of that step's update, as in the reference (its .grad stays None there:
    # models/model_config1.py:26-29, and torch.optim.AdamW skips grad-None tensors)
    opt.track_expert_usage([net.Unet_experts, net.VIT_experts])
    return opt


def build_scheduler(optimizer: torch.optim.Optimizer, optim_config: Dict[str, Any]):
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer=optimizer, T_max=optim_config["total_schedule_steps"],
                                                      eta_min=optim_config["eta_min"])


def save_checkpoint(model, optimizer, step, mse_score, configs, filename, ema=None, null_text_emb=None, balance=None) -> str:
    """Same dictionary and path rules as reference training.py:242-271 (keys step / model_state_dict /
    optimizer_state_dict / mse / config); tensors are written from host copies so the file loads on any device.
    With `ema` (hdmoe_hip.ema.WeightEMA) the file additionally carries "ema_state_dict", with `null_text_emb` (the null row of
    `Trainer(cond_dropout=...)`) "null_text_emb", which the sampler needs for guidance, with `balance` (hdmoe_hip.balance.RouterBalance,
    `Trainer(balance_rate=...).balance`) "router_balance", the routers' selection biases, which the model's state_dict does not hold;
    without them the dictionary is the reference's."""
    if "save_dir" in configs:
        save_path = configs["save_dir"]
    elif "model_configs" in configs and "save_dir" in configs["model_configs"]:
        save_path = configs["model_configs"]["save_dir"]
    else:
        save_path = "./checkpoints"
    os.makedirs(save_path, exist_ok=True)
    full_path = os.path.join(save_path, filename)
    model_state = model.module.state_dict() if hasattr(model, "module") else model.state_dict()
    checkpoint = {"step": step, "model_state_dict": model_state, "optimizer_state_dict": optimizer.state_dict(),
                  "mse": mse_score, "config": configs}
    if ema is not None:
        checkpoint["ema_state_dict"] = ema.state_dict()
    if null_text_emb is not None:
        checkpoint["null_text_emb"] = null_text_emb.detach().cpu()
    if balance is not None:
        checkpoint["router_balance"] = balance.state_dict()
    torch.save(checkpoint, str(full_path))
    print(f"   [Save] Checkpoint saved: {full_path}")
    return full_path


def load_checkpoint(path: str, model: torch.nn.Module, optimizer: Optional[torch.optim.Optimizer] = None, map_location=None, ema=None,
                    balance=None) -> dict:
    """Inverse of `save_checkpoint` (reference training.py:303-304 loads only the model; resuming also needs the
    optimizer moments).  Accepts files written by the reference's torch.optim.AdamW as well.  `ema` and `balance` (the routers' selection
    biases) are restored when the file has them; a saved "null_text_emb" comes back in the returned dictionary like every other key."""
    ck = torch.load(f=path, map_location=map_location, weights_only=False)
    model.load_state_dict(ck["model_state_dict"])
    if optimizer is not None and "optimizer_state_dict" in ck:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
    if ema is not None and "ema_state_dict" in ck:
        ema.load_state_dict(ck["ema_state_dict"])
    if balance is not None and "router_balance" in ck:
        balance.load_state_dict(ck["router_balance"])
    return ck


# The inputs of one step, whichever arm of `Trainer._batch` made them: x the noised latents, x0 the clean ones, keep the text-dropout
# decision (B,) float32 0/1 or None.
Batch = collections.namedtuple("Batch", "x x0 sigma text unet_mask vit_mask zeta keep")


def _is_count(val) -> bool:
    return not isinstance(val, bool) and isinstance(val, int) and val >= 1


def _due(every: Optional[int], step: int) -> bool:
    """Whether what runs behind every `every`-th update (None: never) runs behind the update of step `step`."""
    return every is not None and (step + 1) % every == 0


def _check_arguments(world, fuse_clip_into_step, ema, ema_snapshot_every, ema_snapshot_dir, cond_dropout, null_text_emb, dataset, batch_size,
                     evaluator, eval_every, skip_nonfinite, health_every, max_skips_in_a_row, balance_rate, balance_bias_max) -> None:
    """ValueError for every violated condition on `Trainer`'s keywords, in front of any use of the model."""
    if dataset is None:
        if batch_size is not None:
            raise ValueError("Trainer: batch_size is the dataset's batch size; without a dataset the caller's batches fix it")
    else:
        if not isinstance(dataset, LatentDataset):
            raise ValueError(f"Trainer: dataset is a Utils.utils.LatentDataset, got {type(dataset).__name__}")
        if dataset.text is None:
            raise ValueError("Trainer: the dataset needs text rows (LatentDataset(text=...)): the model is text-conditioned")
        if batch_size is None or int(batch_size) < 1:
            raise ValueError(f"Trainer: a dataset needs batch_size >= 1, got {batch_size}")
        if dataset.N < int(batch_size) * world:
            raise ValueError(f"Trainer: the dataset's N={dataset.N} items do not fill one step of batch_size * world = "
                             f"{int(batch_size)} * {world}")
    if ema_snapshot_every is not None:
        if ema is None:
            raise ValueError("Trainer: ema_snapshot_every needs an ema")
        if ema_snapshot_dir is None:
            raise ValueError("Trainer: ema_snapshot_every needs ema_snapshot_dir")
        if int(ema_snapshot_every) < 1:
            raise ValueError(f"Trainer: ema_snapshot_every must be >= 1, got {ema_snapshot_every}")
    if eval_every is not None:
        if evaluator is None:
            raise ValueError("Trainer: eval_every needs an evaluator")
        if not _is_count(eval_every):
            raise ValueError(f"Trainer: eval_every must be an int >= 1, got {eval_every}")
    elif evaluator is not None:
        raise ValueError("Trainer: an evaluator needs eval_every")
    if evaluator is not None and not callable(getattr(evaluator, "evaluate", None)):
        raise ValueError(f"Trainer: evaluator is a Utils.evaluation.Evaluator, got {type(evaluator).__name__}")
    if not isinstance(skip_nonfinite, bool):
        raise ValueError(f"Trainer: skip_nonfinite is a bool, got {skip_nonfinite!r}")
    if skip_nonfinite and not fuse_clip_into_step:
        raise ValueError("Trainer: skip_nonfinite needs fuse_clip_into_step (the verdict guards the fused clip + AdamW launch)")
    for key, val in (("health_every", health_every), ("max_skips_in_a_row", max_skips_in_a_row)):
        if val is not None and not _is_count(val):
            raise ValueError(f"Trainer: {key} must be an int >= 1, got {val!r}")
    if max_skips_in_a_row is not None and (not skip_nonfinite or health_every is None):
        raise ValueError("Trainer: max_skips_in_a_row needs skip_nonfinite and a health_every (the counters are only seen when read)")
    for key, val in (("balance_rate", balance_rate), ("balance_bias_max", balance_bias_max)):
        if val is None and key == "balance_rate":
            continue
        if isinstance(val, bool) or not isinstance(val, (int, float)) or not math.isfinite(val) or val <= 0:
            raise ValueError(f"Trainer: {key} must be a finite number > 0, got {val!r}")
    if not 0.0 <= float(cond_dropout) <= 1.0:                # NaN fails both comparisons
        raise ValueError(f"Trainer: cond_dropout must lie in [0, 1], got {cond_dropout}")
    if null_text_emb is not None and not torch.is_tensor(null_text_emb):
        raise ValueError(f"Trainer: null_text_emb is a tensor of one text row or None, got {type(null_text_emb).__name__}")


class Trainer:
    """One training iteration of reference training.py:110-197 as a reusable object (device-side sigma / mask / noise
    generation, fused loss, flat-bucket gradient all-reduce, fused clip + AdamW).

    ``device_inputs=True``: sigma, the noised latents, both router masks and zeta of a step come from one fused HIP call
    (`Utils.utils.DeviceInputs`), keyed by ``(seed, rank, step_idx)`` instead of torch's generator; zeta reaches the model as a device
    scalar.  ``seed=None`` takes ``hdmoe_hip.ops.next_seed()`` once, here.  ``step_idx`` is assignable: a run resumed at step k
    regenerates step k's inputs.

    ``graphed=True`` (implies ``device_inputs``): forward + loss + backward run as the replay of `hdmoe_hip.graph.StagedStep` -- what
    bench.py times -- over static buffers.  The first ``train_step`` fixes the latent and text shapes and captures; a capture failure
    raises (no eager fallback), and a later batch of another shape raises ValueError before any device work.  The tensors in the
    returned dictionary are then the static buffers of the captured step: valid until the next ``train_step`` overwrites them, so
    copy what has to live longer.

    With both keywords at their defaults nothing changes: the inputs come from torch's generator and the step is launched eagerly.

    ``cond_dropout=p`` > 0 trains the unconditional branch that classifier-free guidance extrapolates from: each step a sample's text is
    replaced with probability p by ``null_text_emb`` (one text row; None: zeros), and the result gains ``"text_keep"`` (B,) float32 0/1.
    With device inputs the decision is keyed by ``(seed, rank, step_idx)`` like every other input and made inside the one pass that
    copies the text into its static buffer (`DeviceInputs.drop_text`); otherwise it is drawn from torch's generator.  At 0 nothing is
    launched or drawn and the result has no new key.

    ``dataset=LatentDataset(...), batch_size=B`` (implies ``device_inputs``): the trainer draws its own batches.  ``train_step()`` then
    takes no arguments; the items of step k (a keyed epoch permutation, ``drop_last``, disjoint across the ranks of
    ``torch.distributed``), their VAE-posterior draw, horizontal flip and text rows are a function of ``(seed, world, rank, step_idx)``
    made inside the same fused input calls, and the result gains ``"item"`` (B,) int32 and ``"flip"`` (B,) float32 0/1.  Under
    ``graphed=True`` the captured step reads the generator's own buffers: no batch is copied.  Resuming at step k sees step k's data
    again.  With ``dataset=None`` every path is what it was.

    ``evaluator=Utils.evaluation.Evaluator(...), eval_every=n``: behind the update of every n-th step the trainer runs the held-out
    evaluation -- on the raw weights and, when the evaluator was built with this trainer's ``ema``, on each EMA profile -- keeps the
    numbers in ``last_eval`` and hands them to the logger's ``log_evaluation``.  The evaluation leaves the training state untouched.
    With both at their defaults nothing changes.

    ``skip_nonfinite=True`` (needs ``fuse_clip_into_step``): the guard every mixed-precision trainer has, without a host sync.  Behind
    the gradient all-reduce one statistics pass (`hdmoe_hip.optim.GradHealth`, in place of the clip's norm pass: the same number of
    launches) measures the gradients; clip + AdamW and the EMA then run behind its device verdict.  A step whose gradients hold a NaN or
    an Inf, or whose squared norm overflows, is skipped: parameters, both moments, the per-tensor step counts, every EMA profile and the
    EMA step stay bit for bit what they were.  ``step_idx``, the LR scheduler and the zeta and mask schedules still advance -- they follow
    the data, and a rejected batch must not be drawn again -- and an EMA snapshot or an evaluation due on that step still runs.  A step
    with a good verdict is the unguarded step bit for bit.  The result gains ``"step_ok"`` (device int32, 1 = applied) and
    ``"grad_norm"`` (device float32, over the finite elements); nobody reads them here, so nothing syncs.  Under data parallelism the
    gradients are all-reduced before they are measured, so every rank reaches the same verdict.

    ``health_every=n``: behind the update of every n-th step the parameters are measured as well and everything is read with one
    device-to-host copy into ``last_health`` (per-group norm / absmax / non-finite counts of gradients and weights, groups as in
    `hdmoe_hip.optim.health_groups`, and the skip counters) and handed to the logger's ``log_health``.  A non-finite parameter raises
    RuntimeError, and so does ``max_skips_in_a_row=m`` (needs both other keywords; the counters are only seen when they are read) once m
    steps in a row were skipped.  Without ``skip_nonfinite`` the gradients are measured on those steps only and the update is the plain
    one: this mode only observes.  ``health()`` does the same read on demand.  With all three at their defaults nothing changes.

    ``balance_rate=r`` (``balance_bias_max=m``): auxiliary-loss-free load balancing (`hdmoe_hip.balance.RouterBalance`, kept in
    ``balance``).  Both routers pick their top-k over logits + a per-expert bias that no gate weight and no loss term sees; every training
    forward counts its routing on the device, and behind the optimizer step one launch per router moves the bias by r towards the
    under-loaded experts, re-centres it and clamps it to +-m.  With ``skip_nonfinite`` the move runs behind the same verdict: a skipped
    step keeps the bias bit for bit (its counts are dropped).  Under ``graphed=True`` the captured heads read the bias by pointer, so the
    in-place update needs no recapture; under data parallelism the counts are summed over the ranks and every rank takes the same
    decision.  The result gains ``"router_balance"``: per router the device tensors "bias", "load" and "target" of the step (nobody reads
    them here, so nothing syncs); on steps where a health read or an evaluation syncs anyway they also go to the logger's
    ``log_balance``.  The loss's balance weights are the caller's: turn them down or off in ``loss_config``.  At None nothing changes:
    no buffer is registered and every path launches what it launched."""

    def __init__(self, model, model_config, optim_config, loss_config, mask_config, zeta_config, max_grad_norm: float = 1.0,
                 fuse_clip_into_step: bool = True, logger=None, ema=None, ema_snapshot_every: Optional[int] = None,
                 ema_snapshot_dir: Optional[str] = None, device_inputs: bool = False, graphed: bool = False, seed: Optional[int] = None,
                 cond_dropout: float = 0.0, null_text_emb: Optional[torch.Tensor] = None, dataset: Optional[LatentDataset] = None,
                 batch_size: Optional[int] = None, evaluator=None, eval_every: Optional[int] = None, skip_nonfinite: bool = False,
                 health_every: Optional[int] = None, max_skips_in_a_row: Optional[int] = None, balance_rate: Optional[float] = None,
                 balance_bias_max: float = 8.0):
        dist = torch.distributed.is_available() and torch.distributed.is_initialized()
        self.world, self.rank = (torch.distributed.get_world_size(), torch.distributed.get_rank()) if dist else (1, 0)
        _check_arguments(self.world, fuse_clip_into_step, ema, ema_snapshot_every, ema_snapshot_dir, cond_dropout, null_text_emb, dataset,
                         batch_size, evaluator, eval_every, skip_nonfinite, health_every, max_skips_in_a_row, balance_rate, balance_bias_max)
        self.dataset, self.batch_size = dataset, None if batch_size is None else int(batch_size)
        # every `eval_every` steps, behind the update: evaluator.evaluate() on the raw weights and, when the evaluator holds this
        # trainer's ema, on each of its profiles -> last_eval, and the logger's <run>_validation.jsonl
        self.evaluator, self.eval_every, self.last_eval = evaluator, eval_every, None
        # skip_nonfinite: every step's update runs behind the device verdict of one statistics pass over the gradients; health_every: that
        # pass's rows (and the parameters') are read every n-th step -> last_health, the logger's <run>_health.jsonl
        self.skip_nonfinite, self.health_every, self.max_skips_in_a_row = skip_nonfinite, health_every, max_skips_in_a_row
        self.last_health, self._health = None, None
        self.cond_dropout, self.null_text_emb = float(cond_dropout), null_text_emb
        self.model, self.cfg, self.mask_cfg = model, model_config, mask_config
        self.optimizer = build_optimizer(model, optim_config)
        self.scheduler = build_scheduler(self.optimizer, optim_config)
        self.zeta_sched = ZetaScheduler(total_steps=zeta_config["total_schedule_steps"], max_zeta=zeta_config["max_zeta"],
                                        min_zeta=zeta_config["min_zeta"], strategy=zeta_config["strategy"],
                                        warmup_ratio=zeta_config["warmup_ratio"])
        mk = lambda attr, rng: MaskGenerator(expert_attributes=mask_config[attr], p_mean=mask_config["p_mean"], p_std=mask_config["p_std"],
                                             total_steps=model_config["total_steps"], min_active=mask_config["min_active"],
                                             step_size=mask_config["step_size"], max_bandwidth=mask_config["max_BW"],
                                             bandwidth=mask_config["BW"], strat_band=mask_config["strat_band"], noise_range=mask_config[rng])
        self.unet_mask_gen, self.vit_mask_gen = mk("unet_attr", "unet_noise_range"), mk("vit_attr", "vit_noise_range")
        self.criterion = EDM_LOSS(num_experts=model_config["num_experts"], sigma_data=model_config["sigma_data"],
                                  Unet_bal=loss_config["unet_bal"], vit_bal=loss_config["vit_bal"], z_bal=loss_config["z_bal"],
                                  prior_bal=loss_config["prior_bal"])
        # balance_rate: the routers select over logits + a bias that one launch per router moves behind every optimizer step (built in front
        # of the buckets, which then all-reduce the routing counts next to the usage counters)
        self.balance = None
        if balance_rate is not None:
            from hdmoe_hip.balance import RouterBalance
            self.balance = RouterBalance(model, float(balance_rate), float(balance_bias_max))
        self.buckets = GradBuckets(model)                    # .grad become views of flat fp32 buckets (all-reduced when world > 1)
        self.max_grad_norm, self.fuse = float(max_grad_norm), fuse_clip_into_step
        self.logger = logger                                 # graphs.logger.Logger (sync-free) or None
        self.ema = ema                                       # hdmoe_hip.ema.WeightEMA or None: averaged right after every optimizer step
        # every `ema_snapshot_every` steps the averages go to <ema_snapshot_dir>/ema_<step>.pt: sources of hdmoe_hip.posthoc.reconstruct
        self.ema_snapshot_every = None if ema_snapshot_every is None else int(ema_snapshot_every)
        self.ema_snapshot_dir = ema_snapshot_dir
        self._clip_params = [p for p in model.parameters()]
        self.step_idx = 0
        self.graphed = bool(graphed)
        self.device_inputs = bool(device_inputs) or self.graphed or dataset is not None
        self.inputs = None
        if self.device_inputs:
            if seed is None:
                from hdmoe_hip import ops
                seed = ops.next_seed()
            self.seed = int(seed)
            self.inputs = DeviceInputs(model_config, mask_config, zeta_config, self.unet_mask_gen, self.vit_mask_gen, self.zeta_sched,
                                       seed=self.seed, rank=self.rank, cond_dropout=self.cond_dropout, null_text_emb=null_text_emb)
        self._model_extra = model_extras(model, mask_config)
        self._staged = None                                  # hdmoe_hip.graph.StagedStep, built by the first graphed train_step
        self._lat = self._text = None                        # its static latent / text buffers

    def _batch(self, latents: Optional[torch.Tensor], text: Optional[torch.Tensor], step: int, text_out: Optional[torch.Tensor] = None) -> Batch:
        """The inputs of step `step`: the one place where the input modes differ.  `text_out` is the captured step's static text buffer;
        with it the caller's batch is copied into the static buffers (the text substitution is that copy) and the dataset's text rows
        are gathered there -- its latents are made where the captured step reads them, nothing is copied."""
        if not self.device_inputs:                           # torch's generator, in this order: dropout, sigma, noise
            cfg, mc, keep = self.cfg, self.mask_cfg, None
            if self.cond_dropout > 0:                        # no key to be faithful to in this mode
                null = null_text(self.null_text_emb, text)
                kept = torch.rand(text.shape[0], device=text.device) >= self.cond_dropout
                text = torch.where(kept.view(-1, *([1] * (text.ndim - 1))), text, null)
                keep = kept.to(torch.float32)
            sigma = sample_sigma_hybrid(batch_size=latents.shape[0], sigma_max=cfg["sigma_max"], sigma_min=cfg["sigma_min"],
                                        p_mean=mc["p_mean"], p_std=mc["p_std"], extreme_prob=0.5, device=latents.device)
            return Batch(latents + torch.randn_like(latents) * sigma, latents, sigma, text, self.unet_mask_gen(sigma=sigma, step=step),
                         self.vit_mask_gen(sigma=sigma, step=step), self.zeta_sched.get_zeta(step=step), keep)
        if self.dataset is not None:                         # drawn by the generator into its own static buffers
            b = self.inputs.generate_from(self.dataset, step, self.batch_size, world=self.world, rank=self.rank)
            text, keep = self.inputs.text_from(self.dataset, step, out=text_out)
            return Batch(b["x"], b["x0"], b["sigma"], text, b["unet_mask"], b["vit_mask"], b["zeta"], keep if self.cond_dropout > 0 else None)
        keep = None
        if text_out is not None:
            latents = self._lat.copy_(latents)
        elif latents.dtype != torch.float32 or not latents.is_contiguous():
            latents = latents.to(torch.float32).contiguous()
        if self.cond_dropout > 0:
            text, keep = self.inputs.drop_text(text, step, out=text_out)
        elif text_out is not None:
            text = text_out.copy_(text)
        b = self.inputs.generate(latents, step)
        return Batch(b["x"], latents, b["sigma"], text, b["unet_mask"], b["vit_mask"], b["zeta"], keep)

    def _fwd_loss(self, b: Batch):
        out_model = self.model(x=b.x, sigma=b.sigma, text_emb=b.text, Unet_router_mask=b.unet_mask, Vit_router_mask=b.vit_mask, zeta=b.zeta,
                               return_log_var=True, **self._model_extra)
        return out_model, self.criterion(sigma_vec=b.sigma, x=b.x0, sigma=b.sigma, out_model=out_model)

    def _build_staged(self, latents: Optional[torch.Tensor], text: Optional[torch.Tensor]) -> None:
        """Fix the shapes, make the static buffers, fill them for `step_idx` and capture the staged step (bench.py's replay path).  With
        a dataset the latent buffer is the generator's own x0."""
        if self.dataset is not None:
            ds = self.dataset
            self._text = torch.empty((self.batch_size,) + tuple(ds.text.shape[1:]), dtype=ds.text.dtype, device=ds.device)
        else:
            if not latents.is_cuda:
                raise RuntimeError("hdmoe_hip: tensors must live on the GPU (no CPU fallback in the product path)")
            self._shapes = (tuple(latents.shape), tuple(text.shape))
            self._lat = torch.empty(latents.shape, dtype=torch.float32, device=latents.device)     # `_batch` fills both: a clone each
            self._text = torch.empty(text.shape, dtype=text.dtype, device=latents.device)
        batch = self._batch(latents, text, self.step_idx, text_out=self._text)
        self._lat = batch.x0
        self._capture(batch)

    def _capture(self, b: Batch) -> None:
        from hdmoe_hip import graph as hgraph

        def fwd_bwd():
            self.buckets.zero_grad()
            out_model, loss = self._fwd_loss(b)
            hgraph.backward(loss["loss"])
            return {"loss": loss, "out_model": out_model}

        self.buckets.enabled = False                         # no collectives from autograd hooks while capturing
        try:
            self._staged = hgraph.StagedStep(fwd_bwd, b.x0.device)
        finally:
            self.buckets.enabled = True
        if self.buckets.world > 1 or self.buckets.force:     # a branch's bucket goes out as soon as its backward section is launched
            self._staged.after = self.buckets.staged_hooks(self._staged)
        # the warm-up forwards accumulated into the routed-row counters: the first optimizer step must see only its own routing
        self.optimizer.clear_usage()
        if self.balance is not None:                         # ... and so must the first move of the selection bias
            self.balance.clear()

    def train_step(self, latent_images: Optional[torch.Tensor] = None, text_emb: Optional[torch.Tensor] = None) -> dict:
        """One iteration on (latents (B,C,H,W), text embeddings), or with a dataset on the batch the trainer draws for `step_idx` (no
        arguments).  Returns {"loss", "out_model", "sigma"}, "text_keep" when ``cond_dropout`` > 0 and "item" / "flip" with a dataset;
        with ``graphed=True`` their tensors are the captured step's static buffers, valid until the next call."""
        if self.dataset is not None and (latent_images is not None or text_emb is not None):
            raise ValueError("Trainer: with a dataset train_step() takes no batch; the trainer draws it")
        if self.dataset is None and (latent_images is None or text_emb is None):
            raise ValueError("Trainer: train_step(latents, text_emb) needs a batch (or build the Trainer with dataset=...)")
        step = self.step_idx
        if self.graphed:
            if self._staged is None:
                self._build_staged(latent_images, text_emb)
            elif self.dataset is None and (tuple(latent_images.shape), tuple(text_emb.shape)) != self._shapes:
                raise ValueError(f"Trainer(graphed=True): batch shapes {tuple(latent_images.shape)}, {tuple(text_emb.shape)} differ from the "
                                 f"captured step's {self._shapes[0]}, {self._shapes[1]}")
        batch = self._batch(latent_images, text_emb, step, text_out=self._text)
        if self.graphed:                                     # the replay reads the static buffers `batch` was written into
            res = self._staged()
            self.buckets.finish()
            out_model, loss = res["out_model"], res["loss"]
            self._log_forward(step, loss, out_model, batch.sigma)
        else:
            out_model, loss = self._fwd_loss(batch)
            self._log_forward(step, loss, out_model, batch.sigma)
            self.buckets.zero_grad()
            loss["loss"].backward()
            self.buckets.finish()
        return self._update(step, loss, out_model, batch.sigma, batch.keep)

    def _log_forward(self, step: int, loss: dict, out_model: dict, sigma: torch.Tensor) -> None:
        mc = self.mask_cfg
        lg = self.logger
        if lg is not None:                                   # same calls, same order as reference training.py:160-188
            lg.log_training_step(step=step, loss_dict=loss, zeta=self.zeta_sched.get_zeta(step=step),
                                 log_var=out_model["log_var"] if out_model["log_var"] is not None else 0.0,
                                 lr=self.optimizer.param_groups[0]["lr"], sigma=sigma, p_mean=mc["p_mean"], p_std=mc["p_std"])
            lg.log_router_statistics(step=step, unet_probs=out_model["Unet_router_loss"], vit_probs=out_model["vit_router_loss"],
                                     sigma=sigma, p_mean=mc["p_mean"], p_std=mc["p_std"])
            lg.log_scaling_gating(scaling_factors=out_model["scaling_net_out"], gate_weights=out_model["out_gate"], sigma=sigma)

    def _update(self, step: int, loss: dict, out_model: dict, sigma: torch.Tensor, keep: Optional[torch.Tensor] = None) -> dict:
        """Everything behind the backward, in the reference's order: gradient logs, clip + AdamW, EMA, scheduler."""
        lg = self.logger
        health_due, eval_due = _due(self.health_every, step), _due(self.eval_every, step)
        # guard: the statistics whose device verdict the update, the EMA and the bias move run behind; None: all three are the plain calls
        guard = self._grad_health() if self.skip_nonfinite else None
        ok = None if guard is None else guard.ok
        if guard is not None or health_due:                  # in place of the clip's norm pass when the update is guarded
            self._grad_health().measure(step, which="grad", verdict=guard is not None)
        if lg is not None:
            lg.log_gradients(step=step, model=self.model.net)
            lg.log_weight_statistics(step=step, model=self.model.net)
        if self.fuse:
            self.optimizer.step(clip=(self._clip_params, self.max_grad_norm), health=guard)
        else:
            from hdmoe_hip.optim import clip_grad_norm_
            clip_grad_norm_(self._clip_params, self.max_grad_norm)
            self.optimizer.step()
        if self.ema is not None:
            self.ema.update(ok=ok)
            if _due(self.ema_snapshot_every, step):
                self._save_ema_snapshot(step + 1)
        if self.balance is not None:                         # one launch per router; behind a bad verdict only the counts are cleared
            self.balance.step(ok=ok)
        self.scheduler.step()
        self.step_idx += 1
        if health_due:
            self._check_health(step, self._read_health())
        if eval_due:
            self._evaluate(step + 1)
        if self.balance is not None and (health_due or eval_due) and lg is not None and callable(getattr(lg, "log_balance", None)):
            lg.log_balance(step, self.balance.read())        # (these steps sync anyway)
        res = {"loss": loss, "out_model": out_model, "sigma": sigma}
        if guard is not None:                                # device values, read by nobody here: no sync
            res["step_ok"], res["grad_norm"] = guard.ok[0], torch.sqrt(guard.total_sumsq)[0]
        if self.balance is not None:
            res["router_balance"] = self.balance.last()
        if keep is not None:
            res["text_keep"] = keep
        if self.dataset is not None:
            res["item"], res["flip"] = self.inputs.data_buf["item"], self.inputs.data_buf["flip"]
        return res

    def _grad_health(self):
        """The statistics object over the clip's parameter list, built at the first use (the gradients exist by then)."""
        if self._health is None:
            from hdmoe_hip.optim import GradHealth, health_groups
            names, group_of = health_groups(self.model)
            self._health = GradHealth(self._clip_params, group_of, names)
        return self._health

    def _read_health(self) -> dict:
        """Measure the parameters (no verdict) and fetch every row and counter with one copy (it syncs) -> last_health."""
        h = self._grad_health()
        h.measure(self.step_idx, which="param", verdict=False)
        self.last_health = h.read()
        return self.last_health

    def health(self) -> dict:
        """`GradHealth.read()`'s dictionary on demand (it syncs): the gradient rows of the last measured step -- without
        ``skip_nonfinite`` they are measured now, from the gradients the last step left --, the parameter rows as of now, the last
        verdict and the skip counters.  Also kept in ``last_health``."""
        if not self.skip_nonfinite:
            self._grad_health().measure(max(self.step_idx - 1, 0), which="grad", verdict=False)
        return self._read_health()

    def _check_health(self, step: int, h: dict) -> None:
        if self.logger is not None and callable(getattr(self.logger, "log_health", None)):
            self.logger.log_health(step, h, h["groups"])
        if h["param"]["total"]["nonfinite"] > 0:
            bad = [n for n, c in zip(h["groups"], h["param"]["nonfinite"]) if c > 0]
            raise RuntimeError(f"Trainer: non-finite parameters behind step {step} in {bad} "
                               f"({h['param']['total']['nonfinite']} elements); the last good state is the last checkpoint")
        if self.max_skips_in_a_row is not None and h["skipped_in_a_row"] >= self.max_skips_in_a_row:
            raise RuntimeError(f"Trainer: {h['skipped_in_a_row']} steps in a row had non-finite gradients and were skipped "
                               f"(max_skips_in_a_row={self.max_skips_in_a_row}); the last one was step {h['last_skipped_step']}")

    def _evaluate(self, step: int) -> None:
        """The held-out numbers after `step` updates (it syncs: one host copy per evaluation): last_eval = {"step", "results": {tag:
        Evaluator.evaluate's dictionary}} with tag "raw" and, for the evaluator's ema when it is this trainer's, "ema<k>" per profile."""
        ev = self.evaluator
        results = {"raw": ev.evaluate()}
        if self.ema is not None and getattr(ev, "ema", None) is self.ema:
            for k in range(self.ema.nprofiles):
                results[f"ema{k}"] = ev.evaluate(profile=k)
        self.last_eval = {"step": step, "results": results}
        if self.logger is not None:
            for tag, r in results.items():
                self.logger.log_evaluation(step, r, tag=tag)

    def _save_ema_snapshot(self, step: int) -> None:
        """A host copy of every average (it syncs).  The averages are bit-identical across data-parallel ranks: rank 0 writes."""
        if self.rank != 0:
            return
        os.makedirs(self.ema_snapshot_dir, exist_ok=True)
        self.ema.save_snapshot(os.path.join(self.ema_snapshot_dir, f"ema_{step:08d}.pt"))


def train_steps(trainer: Trainer, batches: Union[Iterable, int], on_step: Optional[Callable[[int, dict], None]] = None) -> None:
    """Drive `trainer` over (latents, text_emb) batches, or -- a trainer with a dataset -- over `batches` steps of its own data;
    `on_step(step, result)` is where logging / checkpoints hook in."""
    trainer.model.train()
    if isinstance(batches, int):
        if trainer.dataset is None:
            raise ValueError("train_steps: a number of steps needs a Trainer with a dataset")
        batches = ((None, None) for _ in range(batches))
    for latents, text in batches:
        res = trainer.train_step(latents, text)
        if on_step is not None:
            on_step(trainer.step_idx - 1, res)
