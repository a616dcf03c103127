"""Training-side neighbours of the hot path -- drop-in for the names the reference's ``Utils/utils.py`` exports to
``Utils/training.py`` (``EDM_LOSS``, ``sample_sigma_hybrid``, ``ZetaScheduler``, ``MaskGenerator``).

``EDM_LOSS`` runs as one fused HIP forward + one fused backward with no ``.item()`` host syncs.  The input generators
produce a few (B,)/(B,E) values per step from torch's RNG before the timed path starts; they are kept as plain
torch device ops (data generation, not the denoiser's arithmetic).  ``DeviceInputs`` is their fused form: one HIP call per step
writes sigma, the noised latents, both masks and zeta into static buffers, keyed by (seed, rank, step) instead of a generator; its
``drop_text`` is the conditioning dropout that trains the unconditional branch of classifier-free guidance, under the same key.
``LatentDataset`` keeps the pre-encoded latents (and text rows) on the device; ``DeviceInputs.generate_from`` / ``text_from`` then make
the data of a step in the same fused calls -- epoch order, VAE-posterior draw, horizontal flip, text gather -- keyed by
(seed, world, rank, step), with no host loader.
"""
from __future__ import annotations

import inspect
import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from hdmoe_hip import ops


class EDM_LOSS(nn.Module):
    """log-var-weighted MSE + router load-balance + z-loss, all clamped at 50 (reference Utils/utils.py:105-172)."""

    def __init__(self, num_experts: int, sigma_data: float = 0.5, Unet_bal: float = 0.0005, vit_bal: float = 0.0005,
                 z_bal: float = 0.0001, prior_bal: float = 0.001, transition_sigma: float = 1.0, sharpness: float = 2.0):
        super().__init__()
        self.num_experts = num_experts
        self.sigma_data = sigma_data
        self.Unet_lambda = Unet_bal
        self.vit_lambda = vit_bal
        self.z_bal = z_bal
        self.prior_bal = prior_bal      # the reference computes no prior term (commented out at utils.py:143,145)

    def __call__(self, sigma_vec: torch.Tensor, x: torch.Tensor, sigma: torch.Tensor, out_model: dict) -> dict:
        loss, st = ops.edm_loss(out_model["denoised"], x, out_model["log_var"], out_model["Unet_router_loss"],
                                out_model["vit_router_loss"], out_model["Unet_raw"], out_model["vit_raw"],
                                self.Unet_lambda, self.vit_lambda, self.z_bal)
        return {"loss": loss, "denoising": st[1], "balance": st[2], "z_loss": st[3], "entropy": 0.0, "pure_loss": st[4]}


def sample_sigma_hybrid(batch_size, sigma_min=0.002, sigma_max=80.0, p_mean=-0.4, p_std=1.0, extreme_prob=0.2, device="cuda",
                        generator: Optional[torch.Generator] = None):
    """Log-normal core + log-uniform tail, shuffled (reference Utils/utils.py:26-61)."""
    n_ln = int(batch_size * (1 - extreme_prob))
    ln = (torch.randn([n_ln, 1, 1, 1], device=device, generator=generator) * p_std + p_mean).exp()
    u = torch.rand([batch_size - n_ln, 1, 1, 1], device=device, generator=generator)
    lu = (u * (math.log(sigma_max) - math.log(sigma_min)) + math.log(sigma_min)).exp()
    sigma = torch.cat([ln, lu], dim=0).clamp(sigma_min, sigma_max)
    return sigma[torch.randperm(batch_size, device=device, generator=generator)]


class ZetaScheduler:
    """Exploration-noise schedule (reference Utils/utils.py:175-225); pure host arithmetic."""

    def __init__(self, total_steps: int, max_zeta: float, min_zeta: float = 0.0, strategy: str = "cos", alpha: float = 4.0,
                 warmup_ratio: float = 0.05):
        self.total_steps, self.max_zeta, self.min_zeta = total_steps, max_zeta, min_zeta
        self.strategy, self.alpha = strategy, alpha
        self.warmup_steps = int(total_steps * warmup_ratio)

    def get_zeta(self, step: int) -> float:
        if step < self.warmup_steps:
            return self.max_zeta
        if step >= self.total_steps:
            return self.min_zeta
        cur, tot = step - self.warmup_steps, self.total_steps - self.warmup_steps
        if self.strategy == "cos":
            return float(self.min_zeta + (self.max_zeta - self.min_zeta) * 0.5 * (1 + np.cos(np.pi * cur / tot)))
        if self.strategy == "exp":
            term = max(min(-self.alpha * (cur - (self.max_zeta / tot)), 10), -10)
            z = (self.max_zeta - self.min_zeta) * np.exp(term) + self.min_zeta
            return float(max(min(z, self.max_zeta), self.min_zeta))
        raise ValueError(f"Unknown strategy: {self.strategy}")


class MaskGenerator(nn.Module):
    """Rank-based noise-band expert masks (reference Utils/utils.py:228-330)."""

    def __init__(self, expert_attributes: list, p_mean: float = -0.4, p_std: float = 1.0, bandwidth: float = 0.3,
                 max_bandwidth: float = 0.9, min_active: int = 1, total_steps: int = 5000, step_size: float = 0.1,
                 noise_range: tuple = (0.0, 1.0), strat_band: str = "step"):
        super().__init__()
        self.strat_band, self.total_steps, self.max_bw, self.step_size = strat_band, total_steps, max_bandwidth, step_size
        self.p_mean, self.p_std, self.bandwidth, self.min_active = p_mean, p_std, bandwidth, min_active
        attrs = torch.tensor(expert_attributes, dtype=torch.float32)
        order = torch.sort(attrs, stable=True).indices
        centers = torch.zeros_like(attrs)
        centers[order] = torch.linspace(noise_range[0], noise_range[1], steps=len(attrs))
        self.register_buffer("expert_centers", centers)

    @torch.no_grad()
    def __call__(self, sigma: torch.Tensor, step: int) -> torch.Tensor:
        s = sigma.flatten()
        pct = (0.5 * (1 + torch.erf((torch.log(s) - self.p_mean) / (self.p_std * np.sqrt(2))))).clamp(0, 1)
        dist = torch.abs(pct.view(-1, 1) - self.expert_centers.to(s.device).view(1, -1))
        mask = (dist <= self.bandwidth_scheduler(step)).float()
        mask.scatter_(1, torch.topk(-dist, k=self.min_active, dim=-1).indices, 1.0)
        return mask

    def bandwidth_scheduler(self, step: int) -> float:
        if step >= self.total_steps:
            return self.max_bw
        if self.strat_band == "linear":
            return self.bandwidth + (self.max_bw - self.bandwidth) * step / float(self.total_steps)
        if self.strat_band == "step":
            progress = min(int(step / (self.total_steps * self.step_size)) / int(1.0 / self.step_size), 1.0)
            return self.bandwidth + (self.max_bw - self.bandwidth) * progress
        raise ValueError(f"Unknown bandwidth strategy: {self.strat_band}")


class LatentDataset:
    """Pre-encoded latents, resident on the GPU, that `DeviceInputs.generate_from` / `Trainer(dataset=...)` draw their batches from
    (the reference's Flowers102 -> VAE -> DataLoader(shuffle=True, drop_last=True) chain, Utils/training.py:226-239, VAE_CLIP.py:58-66).

    ``mean`` (N,C,H,W) float32 or bfloat16 and optionally ``std`` of the same shape and dtype: a step's latent is
    ``scale * (mean + std * eps)`` with a fresh keyed draw per step (``std=None``: ``scale * mean``), mirrored along W with probability
    ``flip``.  ``text`` (K, ...) holds the text rows: K == 1 one prompt for every item, K == N one row per item, any K with
    ``text_index`` (N,) int32 naming each item's row.  ``text_index`` is range-checked here, once (one host sync): the kernels follow
    it unchecked.  Tensors are moved to ``device`` (default: the current GPU) unless they already live on a GPU; ValueError names the
    argument of every violated condition before any device work."""

    def __init__(self, mean: torch.Tensor, std: Optional[torch.Tensor] = None, *, scale: float = 1.0, flip: float = 0.0,
                 text: Optional[torch.Tensor] = None, text_index: Optional[torch.Tensor] = None, device=None):
        if not torch.is_tensor(mean) or mean.ndim != 4 or mean.shape[0] < 1 or mean.numel() == 0:
            raise ValueError(f"LatentDataset: mean is a (N, C, H, W) tensor with N >= 1, got {tuple(mean.shape) if torch.is_tensor(mean) else type(mean).__name__}")
        if mean.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"LatentDataset: mean must be float32 or bfloat16, got {mean.dtype}")
        N = mean.shape[0]
        if N >= 1 << 31:
            raise ValueError(f"LatentDataset: mean holds N={N} items, the keyed order needs N < 2^31")
        if std is not None and (not torch.is_tensor(std) or tuple(std.shape) != tuple(mean.shape) or std.dtype != mean.dtype):
            got = (tuple(std.shape), std.dtype) if torch.is_tensor(std) else type(std).__name__
            raise ValueError(f"LatentDataset: std must have mean's shape {tuple(mean.shape)} and dtype {mean.dtype}, got {got}")
        scale, flip = float(scale), float(flip)
        if not math.isfinite(scale):
            raise ValueError(f"LatentDataset: scale must be finite, got {scale}")
        if not 0.0 <= flip <= 1.0:
            raise ValueError(f"LatentDataset: flip is a probability in [0, 1], got {flip}")
        if text is None and text_index is not None:
            raise ValueError("LatentDataset: text_index without text")
        if text is not None:
            if not torch.is_tensor(text) or text.ndim < 2 or text.shape[0] < 1 or text.numel() == 0:
                raise ValueError("LatentDataset: text is a (K, ...) tensor with K >= 1 and a non-empty row")
            if text.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise ValueError(f"LatentDataset: text must be float32, bfloat16 or float16, got {text.dtype}")
            if text_index is None and text.shape[0] not in (1, N):
                raise ValueError(f"LatentDataset: text has K={text.shape[0]} rows for N={N} items: K must be 1 or N, or give a text_index")
        if text_index is not None:
            if not torch.is_tensor(text_index) or tuple(text_index.shape) != (N,) or text_index.dtype != torch.int32:
                raise ValueError(f"LatentDataset: text_index is a (N,) = ({N},) int32 tensor")
        tensors = [t for t in (mean, std, text, text_index) if t is not None]
        if device is None:
            on = [t.device for t in tensors if t.is_cuda]
            device = on[0] if on else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("hdmoe_hip: tensors must live on the GPU (no CPU fallback in the product path)")
        put = lambda t: None if t is None else t.detach().to(device).contiguous()
        self.mean, self.std, self.text, self.text_index = put(mean), put(std), put(text), put(text_index)
        self.scale, self.flip, self.N, self.device = scale, flip, N, device
        if self.text_index is not None:                        # the one sync: the only thing between a bad index and a device fault
            lo, hi = int(self.text_index.min()), int(self.text_index.max())
            if lo < 0 or hi >= self.text.shape[0]:
                raise ValueError(f"LatentDataset: text_index holds values in [{lo}, {hi}], text has rows 0 .. {self.text.shape[0] - 1}")

    def __len__(self) -> int:
        return self.N


class DeviceInputs:
    """The per-step training inputs from one fused HIP call (csrc/traingen.hip; RNG contract in include/hdmoe.h) instead of
    ``sample_sigma_hybrid`` + ``randn_like`` + two ``MaskGenerator`` calls on torch's generator.

    It owns the static output buffers: allocated by the first ``generate`` and fixed to that latent shape, so captured graphs can
    read them.  The outputs depend on ``(seed, rank, step)`` alone -- no generator state, no host sync -- so a resumed run regenerates
    the inputs of any step.  Bandwidths and zeta are the host schedulers' values for the step.

    ``cond_dropout`` > 0: ``drop_text`` replaces a sample's text by ``null_text_emb`` (one row; None: zeros) with that probability,
    in the one pass that copies the text into a static buffer (hdmoe_text_dropout), keyed like everything else here."""

    GOLDEN = 0x9E3779B97F4A7C15

    def __init__(self, model_config, mask_config, zeta_config, unet_mask_gen: "MaskGenerator", vit_mask_gen: "MaskGenerator",
                 zeta_sched: "ZetaScheduler", seed: int, rank: int = 0, extreme_prob: float = 0.5, cond_dropout: float = 0.0,
                 null_text_emb: Optional[torch.Tensor] = None):
        self.cfg, self.mask_cfg, self.zeta_cfg = model_config, mask_config, zeta_config
        self.unet_mask_gen, self.vit_mask_gen, self.zeta_sched = unet_mask_gen, vit_mask_gen, zeta_sched
        if unet_mask_gen.expert_centers.numel() != vit_mask_gen.expert_centers.numel() or unet_mask_gen.min_active != vit_mask_gen.min_active:
            raise ValueError("DeviceInputs: both mask generators need the same number of experts and the same min_active")
        self.data_seed = int(seed) & 0xFFFFFFFFFFFFFFFF        # rank-free: every rank walks the same epoch permutation (generate_from)
        self.seed = (int(seed) + int(rank) * self.GOLDEN) & 0xFFFFFFFFFFFFFFFF
        self.extreme_prob = float(extreme_prob)
        self.cond_dropout = float(cond_dropout)
        if not 0.0 <= self.cond_dropout <= 1.0:
            raise ValueError(f"DeviceInputs: cond_dropout must lie in [0, 1], got {cond_dropout}")
        if null_text_emb is not None and not torch.is_tensor(null_text_emb):
            raise ValueError(f"DeviceInputs: null_text_emb is a tensor of one text row or None, got {type(null_text_emb).__name__}")
        self.null_text_emb = null_text_emb
        self.shape = None
        self.buf = None
        self.keep = self.text = self._null = None             # drop_text's static buffers and the null row as the kernel reads it
        self._text_like = None
        self.data_buf = None                                  # generate_from's dictionary: buf plus "x0", "item", "flip"

    def _alloc(self, shape, dev) -> None:
        B = shape[0]
        self._ucen = self.unet_mask_gen.expert_centers.detach().to(device=dev, dtype=torch.float32).contiguous()
        self._vcen = self.vit_mask_gen.expert_centers.detach().to(device=dev, dtype=torch.float32).contiguous()
        E = self._ucen.numel()
        f32 = dict(dtype=torch.float32, device=dev)
        self.buf = {"sigma": torch.zeros(B, 1, 1, 1, **f32), "x": torch.zeros(shape, **f32), "unet_mask": torch.zeros(B, E, **f32),
                    "vit_mask": torch.zeros(B, E, **f32), "zeta": torch.zeros(1, **f32), "src": torch.zeros(B, dtype=torch.int32, device=dev)}
        self.shape = tuple(shape)

    def _schedule(self, step: int) -> dict:
        """The keywords `ops.train_inputs` and `ops.dataset_inputs` share: the sigma distribution and step `step`'s host schedules."""
        mc = self.mask_cfg
        return dict(sigma_min=self.cfg["sigma_min"], sigma_max=self.cfg["sigma_max"], p_mean=mc["p_mean"], p_std=mc["p_std"],
                    extreme_prob=self.extreme_prob, unet_bw=self.unet_mask_gen.bandwidth_scheduler(step),
                    vit_bw=self.vit_mask_gen.bandwidth_scheduler(step), min_active=self.unet_mask_gen.min_active,
                    zeta=self.zeta_sched.get_zeta(step=step))

    def _text_out(self, like: torch.Tensor, shape, out: Optional[torch.Tensor]) -> torch.Tensor:
        """Where `drop_text` / `text_from` write a step's text of `shape` (dtype and device of `like`): `out`, or the lazily made static
        ``text``.  The first call fixes shape and dtype and makes ``keep`` and the null row as the kernel reads it."""
        sig = (tuple(shape), like.dtype)
        if self._text_like is None:
            self._null = _null_row(self.null_text_emb, like)
            self.keep = torch.zeros(shape[0], dtype=torch.float32, device=like.device)
            self._text_like = sig
        elif sig != self._text_like:
            raise ValueError(f"DeviceInputs: text {sig} differs from the static buffers' {self._text_like}")
        if out is not None:
            return out
        if self.text is None:
            self.text = torch.empty(sig[0], dtype=sig[1], device=like.device)
        return self.text

    def generate(self, latents: torch.Tensor, step: int) -> dict:
        """{"sigma", "x", "unet_mask", "vit_mask", "zeta", "src"}: the static buffers, holding step `step`'s inputs for `latents`
        (B,C,H,W) float32 contiguous, until the next call."""
        if latents.ndim != 4:
            raise ValueError(f"DeviceInputs: latents are (B,C,H,W), got {tuple(latents.shape)}")
        if self.shape is not None and tuple(latents.shape) != self.shape:
            raise ValueError(f"DeviceInputs: latents {tuple(latents.shape)} differ from the static buffers' {self.shape}")
        if self.buf is None:
            if not latents.is_cuda:
                raise RuntimeError("hdmoe_hip: tensors must live on the GPU (no CPU fallback in the product path)")
            self._alloc(tuple(latents.shape), latents.device)
        b = self.buf
        ops.train_inputs(b["x"], b["sigma"], b["unet_mask"], b["vit_mask"], b["zeta"], b["src"], latents, self._ucen, self._vcen, self.seed,
                         int(step), **self._schedule(step))
        return b

    def generate_from(self, dataset: "LatentDataset", step: int, batch_size: int, world: int = 1, rank: int = 0) -> dict:
        """`generate`'s dictionary plus {"x0", "item", "flip"}, all static buffers: step `step`'s batch of `batch_size` items drawn from
        `dataset` for `rank` of `world` (item (B,) int32 dataset rows, flip (B,) float32 0/1, x0 the clean latents, x the noised ones),
        in the same two launches, until the next call.  The items follow the rank-free seed, everything else (seed, rank, step)."""
        if not isinstance(dataset, LatentDataset):
            raise ValueError(f"DeviceInputs: dataset is a LatentDataset, got {type(dataset).__name__}")
        B, world, rank = int(batch_size), int(world), int(rank)
        if B < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"DeviceInputs: batch_size >= 1, world >= 1 and rank in [0, world), got {batch_size}, {world}, {rank}")
        if dataset.N < B * world:
            raise ValueError(f"DeviceInputs: the dataset's N={dataset.N} items do not fill one step of batch_size * world = {B} * {world}")
        shape = (B,) + tuple(dataset.mean.shape[1:])
        if self.shape is not None and shape != self.shape:
            raise ValueError(f"DeviceInputs: batch {shape} differs from the static buffers' {self.shape}")
        if self.buf is None:
            self._alloc(shape, dataset.device)
        if self.data_buf is None:
            dev = dataset.device
            self.data_buf = dict(self.buf, x0=torch.zeros(shape, dtype=torch.float32, device=dev),
                                 item=torch.zeros(B, dtype=torch.int32, device=dev), flip=torch.zeros(B, dtype=torch.float32, device=dev))
        b = self.data_buf
        ops.dataset_inputs(b["x"], b["x0"], b["sigma"], b["unet_mask"], b["vit_mask"], b["zeta"], b["src"], b["item"], b["flip"], dataset.mean,
                           dataset.std, self._ucen, self._vcen, self.seed, self.data_seed, int(step), world=world, rank=rank, scale=dataset.scale,
                           p_flip=dataset.flip, **self._schedule(step))
        return b

    def text_from(self, dataset: "LatentDataset", step: int, out: Optional[torch.Tensor] = None):
        """(text_out, keep) of step `step`: the text rows of the items the last `generate_from` wrote (call it first, for the same step),
        with `drop_text`'s substitution under the same key folded into the gather; ``cond_dropout`` 0 is a pure gather and keep all ones.
        Static buffers like `drop_text`'s, `out` likewise."""
        if not isinstance(dataset, LatentDataset) or dataset.text is None:
            raise ValueError("DeviceInputs: text_from needs a LatentDataset with text")
        if self.data_buf is None:
            raise ValueError("DeviceInputs: text_from reads the items of generate_from: call that first")
        item = self.data_buf["item"]
        out = self._text_out(dataset.text, (item.shape[0],) + tuple(dataset.text.shape[1:]), out)
        ops.text_gather_dropout(out, self.keep, dataset.text, dataset.text_index, item, self._null, self.seed, int(step), self.cond_dropout,
                                dataset.N)
        return out, self.keep

    def drop_text(self, text: torch.Tensor, step: int, out: Optional[torch.Tensor] = None):
        """(text_out, keep) of step `step`: keep (B,) float32 0/1 under the key (seed, rank, step), text_out[i] = text[i] where
        keep[i] == 1 and the null row otherwise.  `keep` is a static buffer, and so is text_out unless the caller brings `out`
        (a captured step's own text buffer); both hold the step's values until the next call.  The first call fixes shape and dtype."""
        if not text.is_cuda:
            raise RuntimeError("hdmoe_hip: tensors must live on the GPU (no CPU fallback in the product path)")
        text = text.detach()
        if not text.is_contiguous():
            text = text.contiguous()
        out = self._text_out(text, text.shape, out)
        ops.text_dropout(out, self.keep, text, self._null, self.seed, int(step), self.cond_dropout)
        return out, self.keep


def model_extras(model: nn.Module, mask_config: dict) -> dict:
    """The forward keywords only some models take: model_config2 reads the soft-gate transition from the mask config, model_config1
    learns its scaling and has no such arguments."""
    if "transition_point" in inspect.signature(model.forward).parameters:
        return {"transition_point": mask_config["p_mean"], "softness": mask_config["p_std"]}
    return {}


def _null_row(null: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    """`null` as one contiguous row of `like` (its device and dtype); ValueError unless it has the shape of like[0]."""
    if null is None:
        return None
    if not torch.is_tensor(null) or tuple(null.shape) != tuple(like.shape[1:]):
        got = tuple(null.shape) if torch.is_tensor(null) else type(null).__name__
        raise ValueError(f"null text embedding: expected one row of shape {tuple(like.shape[1:])}, got {got}")
    return null.detach().to(device=like.device, dtype=like.dtype).contiguous()


def null_text(null: Optional[torch.Tensor], like: torch.Tensor) -> torch.Tensor:
    """The null row a model was trained with (`Trainer(null_text_emb=...)`; None: zeros) as a batch of `like`'s shape, dtype and device:
    what `EDM_Sampler.sample` and `forward_guided` take as `uncond_text_emb`."""
    row = _null_row(null, like)
    if row is None:
        return torch.zeros_like(like)
    return row.unsqueeze(0).expand(like.shape).contiguous()
