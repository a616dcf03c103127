"""Heun 2nd-order EDM sampler -- drop-in for the reference's ``Utils/EDM_sampler.py`` (row N1 of SURVEY.md section 8(f)).

Same constructor / ``denoise`` / ``sample`` signatures and semantics (Karras rho-schedule, optional churn, CFG lerp).  The
2N-1 model evaluations run through the HIP path; the per-step latent updates are fused launches (no torch arithmetic on the latents), and
the denoiser call is sync-free (device-side dispatch plan, no ``mask.any()``).  With ``use_graph=True`` (and no churn) a WHOLE Heun stage --
both evaluations, the Euler step and the 2nd-order correction, sigma taken from a device-side copy of the schedule -- is one captured
hipGraph replayed N - 1 times (plus one for the last, Euler-only stage): no host arithmetic between evaluations.  With churn the
evaluation alone is captured, as before.

``solver="dpmpp_2m"`` (extension) replaces Heun by the DPM-Solver++(2M) multistep solver: one evaluation per stage, the previous stage's
denoiser output standing in for the second one (N evaluations for N stages instead of 2N - 1).  Its fp32 stage is one evaluation plus the
fused ``hdmoe_dpm2m_step`` update; with ``use_graph`` ONE captured graph is replayed once per stage.  Other latent dtypes run a host-driven loop.

Stochastic sampling on the device (extensions, opt-in).  ``churn_on_device=True`` runs ``S_churn > 0`` through the fused Heun stage: the churn
(gamma, t_hat, x_hat = x + c eps) is one kernel in front of the first evaluation, and the Euler / correction kernels read t_hat from the
device.  ``solver="dpmpp_2m_sde"`` is DPM-Solver++(2M) SDE in its midpoint form (``eta`` scales the noise, 0 = ``dpmpp_2m``), one evaluation
per stage.  Both draw inside the stage kernels from a counter RNG keyed by (the call's seed, the stage index), both device-resident, so the
captured stages replay with fresh noise; ``sample(seed=...)`` fixes the draw, on the host loops too.

Extensions over the reference, all opt-in (``sample()`` keywords; with their defaults every path computes what it did without them):
image-to-image from ``init_latents`` part-way down the schedule (``strength``), inpainting (``inpaint_mask``: the known region is put back on
its probability-flow path ``x0 + sigma * noise`` by the epilogue of the update kernels), and expert steering (``Unet_router_mask`` /
``Vit_router_mask``, also on ``denoise()``).

``shared_guidance=True`` (extension, opt-in; needs ``Guide_net is model``): a guided evaluation (``guidance != 1``) is ONE pass through
``model.forward_guided`` instead of two: everything the text does not reach -- time embedding, stem, path scaling, both routers and both
dispatch plans -- is computed once, both text variants go through the expert banks and the fusion tail as one 2B-row batch, and the guided
D_x is formed by the egress kernel.  Every solver, ``use_graph`` and every ``sample()`` keyword work with it; ``uncond_text_emb=None``
then returns the plain D_x exactly (the unconditional branch IS the conditional one).

Guidance interval and per-sample scales (extensions, opt-in).  ``guidance_interval=(lo, hi)`` guides only the evaluations whose sigma lies in
[lo, hi] (limited-interval guidance); the others are the single plain conditional call, at 1x the cost.  The solver decides per evaluation
on the host (``guidance_plan``) and, with ``use_graph``, replays the stage variant captured for that decision.  ``sample(guidance=vector)`` /
``denoise(guidance=vector)`` take one scale per sample from a device buffer instead of the float baked into the capture.

Guidance rescale and adaptive projected guidance, APG (extensions, opt-in).  ``guidance_rescale`` > 0 pulls the per-sample standard
deviation of the guided output back to that of the conditional output (Lin et al. 2024, section 3.4); ``apg_eta`` (with
``apg_norm_threshold`` and ``apg_momentum``) splits the guidance update into its parts parallel and orthogonal to the conditional output,
weights the parallel part by eta, clamps the update's norm and gives it a momentum across evaluations (Sadat et al. 2024).  Either one turns
the blend of every guided evaluation into ONE launch of the combine kernel (``ops.guide_combine`` two-pass, the egress
``ops.nhwc_to_nchw_guide_combine`` with shared_guidance); the momentum lives in a device buffer of the stage state, so captured stages
replay it.  With the defaults no launch changes.

Composed guidance over several prompts (extension, opt-in; ``sample()`` / ``denoise()`` keywords ``compose_text``, ``compose_weights``,
``compose_masks``).  K conditions -- ``text_emb`` and the K - 1 of ``compose_text`` -- with per-sample weights a and optional spatial masks
m in [0, 1] over the latent positions stand in for the one conditional output (composable diffusion, Liu et al. 2022):
D_c = D_u + sum_k a_k m_k (D_k - D_u); prompt blending, negative prompts (a_k < 0) and regional prompts are its cases.  D_c then takes the
place of the conditional output in everything above: the scale, per-sample scales, the interval, rescale and APG.  With
``shared_guidance`` an evaluation is ONE ``model.forward_composed`` pass -- the routing once, the K + 1 text variants stacked through the
banks and the tail, D_c formed in the egress kernel; otherwise K passes of the model, one of the guide network and ONE launch of
``ops.guide_compose``.  D_c needs D_u, so an evaluation outside the guidance interval is the composed evaluation at scale 1 (out = D_c),
not one plain call.  Without the keywords nothing changes.

Tiled sampling (extension, opt-in; ``sample()`` keywords ``tile``, ``tile_overlap``, ``tile_window``, ``tile_batch``).  The model can only
be evaluated at the latent size it was built for; every solver update is pointwise, so a larger (B, C, H, W) latent runs through the
solvers unchanged and only the denoiser evaluation is tiled: ``den_big = blend(model(gather(x_big)))`` over overlapping model-sized windows
(``ops.tile_plan`` / ``ops.tile_gather`` / ``ops.tile_blend``, MultiDiffusion, Bar-Tal et al. 2023).  One method, ``_denoise_tiled``,
serves the fused and captured stages and the host loops; the text, the router masks and the per-sample scales are repeated per tile row.
"""
import collections
import math
import numbers

import numpy as np
import torch
import torch.nn as nn

from hdmoe_hip import graph as hgraph
from hdmoe_hip import ops

SOLVERS = ("heun", "dpmpp_2m", "dpmpp_2m_sde")


def _each(fn, *vs):
    """fn over matching fields of _Inputs records: a tensor, or the `known` triple entry by entry; None (and the floats) pass through."""
    if isinstance(vs[0], tuple):
        return tuple(fn(*e) for e in zip(*vs))
    return fn(*vs) if isinstance(vs[0], torch.Tensor) else vs[0]


class _Inputs(collections.namedtuple("_Inputs", "text unc um vm g texts cw cm known transition_mean softness")):
    """The operands of a denoiser evaluation, built once per sample() / denoise() call (EDM_Sampler._inputs) and handed down whole.  Per
    row (B rows, B T with tiling): text; unc, the unconditional text; um / vm, the (B, E) router masks; g, the (B,) guidance scales.
    Composed guidance: texts (K, B, ...) with text first, cw (B, K), cm (B, K, H, W).  known: the inpainting triple (x0, noise, mask) of
    the solver updates.  All but text may be None.  transition_mean, softness: floats.  Whatever has to list the inputs is a method here."""
    __slots__ = ()
    PER_ROW = ("text", "unc", "um", "vm", "g")

    def signature(self):                                      # what a capture bakes in: which fields exist, their shapes, the floats (last)
        return tuple(_each(lambda a: tuple(a.shape), v) for v in self[:-2]) + (float(self.transition_mean), float(self.softness))

    def empty_like(self):                                     # the static buffers of a capture
        return self._make(_each(torch.empty_like, v) for v in self)

    def copy_from(self, other):                               # refresh of the static buffers; a field they do not hold is skipped
        for dst, src in zip(self, other):
            _each(torch.Tensor.copy_, dst, src)

    def per_row(self, fn):                                    # fn over the per-row fields: the tile-row repeat, a chunk of tile rows
        return self._replace(**{k: _each(fn, getattr(self, k)) for k in self.PER_ROW})


class EDM_Sampler:
    def __init__(self, model: nn.Module, Guide_net: nn.Module, num_solve_steps: int = 32, sigma_min: float = 0.002,
                 sigma_max: float = 80, rho: int = 7, S_churn: float = 0.0, S_min: float = 0.0, S_max: float = float("inf"),
                 S_noise: float = 1.0, guidance: float = 1.0, dtype=torch.float32, use_graph: bool = False, solver: str = "heun",
                 churn_on_device: bool = False, eta: float = 1.0, shared_guidance: bool = False, guidance_interval=None,
                 guidance_rescale: float = 0.0, apg_eta: float = None, apg_norm_threshold: float = float("inf"),
                 apg_momentum: float = 0.0):
        if not isinstance(solver, str) or solver not in SOLVERS:
            raise ValueError(f"solver must be one of {', '.join(map(repr, SOLVERS))}, got {solver!r}")
        if solver != "heun" and S_churn > 0:
            raise ValueError(f"solver={solver!r} does not take S_churn > 0 (got {S_churn}): churn is defined for solver='heun' only")
        try:
            eta_f = float(eta)
        except (TypeError, ValueError):
            raise ValueError(f"eta must be a finite number >= 0, got {eta!r}") from None
        if not (math.isfinite(eta_f) and eta_f >= 0.0):
            raise ValueError(f"eta must be a finite number >= 0, got {eta!r}")
        if solver != "dpmpp_2m_sde" and eta_f != 1.0:
            raise ValueError(f"eta (got {eta!r}) is the noise scale of solver='dpmpp_2m_sde' only, not of solver={solver!r}")
        # guidance rescale / APG: checked here, launch scalars of the combine kernel from then on (part of every capture key)
        self.guidance_rescale = self._check_number(guidance_rescale, "guidance_rescale", "in [0, 1]", lambda v: 0.0 <= v <= 1.0)
        self.apg_eta = None if apg_eta is None else self._check_number(apg_eta, "apg_eta", "None or in [0, 1]", lambda v: 0.0 <= v <= 1.0)
        self.apg_norm_threshold = self._check_number(apg_norm_threshold, "apg_norm_threshold", "> 0 (inf: no clamp)", lambda v: v > 0.0)
        self.apg_momentum = self._check_number(apg_momentum, "apg_momentum", "in (-1, 1)", lambda v: -1.0 < v < 1.0)
        if self.apg_eta is None:
            for name, val, default in (("apg_norm_threshold", self.apg_norm_threshold, float("inf")), ("apg_momentum", self.apg_momentum, 0.0)):
                if val != default:
                    raise ValueError(f"{name}={val} belongs to projected guidance: it needs apg_eta (got apg_eta=None)")
        self.model = model
        self.gnet = Guide_net
        self.shared_guidance = bool(shared_guidance)     # extension: a guided evaluation is ONE shared-routing pass (model.forward_guided)
        self._check_shared()
        self.num_steps = num_solve_steps
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max
        self.rho = rho
        self.s_churn = S_churn
        self.s_min = S_min
        self.s_max = S_max
        self.s_noise = S_noise
        self.guide = guidance
        self.guidance_interval = guidance_interval       # extension: None, or (lo, hi): guide only the evaluations with lo <= sigma <= hi
        self.last_evaluations = None                     # {"guided": n, "plain": m} of the last sample() call
        self.dtype = dtype
        self.use_graph = use_graph          # extension over the reference: hipGraph replay of the denoiser evaluation
        self.solver = solver                # extension over the reference: "dpmpp_2m" = DPM-Solver++(2M), one evaluation per stage
        self.churn_on_device = bool(churn_on_device)     # extension: S_churn > 0 through the fused Heun stage (noise drawn in the kernel)
        self.eta = eta_f                    # solver="dpmpp_2m_sde": noise scale of DPM-Solver++(2M) SDE (S_noise multiplies the draw)
        # no churn (or churn_on_device), fp32 latents: a solver stage = both denoiser evaluations + the fused (churn /) Euler / Heun-correction
        # kernels with sigma read from a device-side schedule; with use_graph it is ONE captured graph, replayed N - 1 times, plus one graph
        # for the last (Euler-only) stage
        self.fused_heun = False
        # solver="dpmpp_2m" / "dpmpp_2m_sde", fp32 latents: a stage = one evaluation + the fused multistep update; with use_graph ONE
        # captured graph serves every stage, the last one and the first (no history) included: the kernel picks the order on the device
        self.fused_dpm = False
        # _stage_state() of the captured evaluation ("eval") and of the fused solver stage ("heun" / "dpm"): buffers, stage functions,
        # graphs and the key they were built for
        self._graph = None
        self._stage = None

    # reference Utils/EDM_sampler.py:35-70
    def denoise(self, x, sigma, text_emb, transition_mean, softness, uncond_text_emb=None, Unet_router_mask=None, Vit_router_mask=None,
                guidance=None, guided=True, momentum_state=None, compose_text=None, compose_weights=None, compose_masks=None):
        """One (guided) denoiser evaluation.  Router masks: (B, E) or (E,) with {0, 1} entries, None = every expert allowed (the reference).
        With shared_guidance a guided evaluation is one model.forward_guided pass (inference: call it under torch.no_grad()).
        guidance: None = the sampler's float scale, or a (B,) tensor of finite per-sample scales (any device).  guided=False: the single
        plain conditional evaluation, whatever the scale.  denoise() never reads sigma: whether an evaluation lies in guidance_interval is
        the solver's decision (sample()), handed down as `guided`.
        momentum_state: the APG momentum buffer, a contiguous (B, C, H, W) float32 tensor on x's device, updated in place by a guided
        evaluation (zero it before the first evaluation of a trajectory).  apg_momentum != 0 needs it; otherwise it is not used.
        compose_text / compose_weights / compose_masks: composed guidance, see sample(); guided=False is then D_c, the composed
        evaluation at scale 1."""
        if self.apg_momentum != 0.0:
            ms = momentum_state
            if not isinstance(ms, torch.Tensor):
                raise ValueError(f"apg_momentum={self.apg_momentum} needs momentum_state, a float32 tensor of shape {tuple(x.shape)} on "
                                 f"{x.device}, got {type(ms).__name__}")
            if ms.dtype != torch.float32 or tuple(ms.shape) != tuple(x.shape) or ms.device != x.device or not ms.is_contiguous():
                raise ValueError(f"momentum_state must be a contiguous float32 tensor of shape {tuple(x.shape)} on {x.device}, got "
                                 f"{tuple(ms.shape)} {ms.dtype} on {ms.device}")
        else:
            momentum_state = None
        inp, _ = self._inputs(x, text_emb, transition_mean, softness, uncond_text_emb, Unet_router_mask=Unet_router_mask,
                              Vit_router_mask=Vit_router_mask, guidance=guidance, compose_text=compose_text,
                              compose_weights=compose_weights, compose_masks=compose_masks)
        return self._denoise(x, sigma, inp, bool(guided), momentum_state)

    def _denoise(self, x, sigma, inp, guided=True, mom=None):
        """denoise() on the validated operands inp (_Inputs): no host read, so it can run under stream capture.  inp.g None: the scale
        is self.guide.  guided False, or a float scale of 1: one plain conditional call.
        With guidance rescale / APG (combine_params()) the blend of a guided evaluation is the combine kernel; mom: its momentum buffer
        (apg_momentum != 0), read and written by guided evaluations only.
        inp.texts: composed guidance; inp.text is then texts[0] and is not read."""
        um, vm = (torch.ones((x.shape[0], self.model.num_experts), device=x.device) if m is None else m for m in (inp.um, inp.vm))
        kw = dict(x=x, sigma=sigma, Unet_router_mask=um, Vit_router_mask=vm, zeta=0, transition_point=inp.transition_mean,
                  softness=inp.softness)
        # the guidance decision, once: the scale the kernels get and the combine record (eta, norm_threshold, momentum, rescale, state)
        # or None; the exits below only choose a callee
        active = guided and (inp.g is not None or self.guide != 1.0)
        scale = (self.guide if inp.g is None else inp.g) if active else 1.0
        comb = self.combine_params() if active else None
        rec = None if comb is None else comb + (mom,)
        # no record: the keyword defaults of ops.guide_* are the identity scalars
        ckw = {} if rec is None else dict(zip(("eta", "norm_threshold", "momentum", "rescale", "state"), rec))
        if inp.texts is not None:
            # composed guidance: D_c of the K conditions takes the conditional output's place.  Not active (the interval, guided=False,
            # a float scale of 1): the same evaluation at scale 1 with the identity scalars, out = D_c, the momentum untouched
            if self.shared_guidance:
                self._check_shared(composed=True)
                return self.model.forward_composed(text_embs=inp.texts, uncond_text_emb=inp.unc, weights=inp.cw, masks=inp.cm,
                                                   guidance=scale, guide_combine=rec, **kw)["denoised"].to(self.dtype)
            ds = [self.model(text_emb=inp.texts[k], **kw)["denoised"].to(self.dtype) for k in range(inp.texts.shape[0])]
            ref_D_x = self.gnet(text_emb=inp.unc, **kw)["denoised"].to(self.dtype)
            return ops.guide_compose(ref_D_x, ds, inp.cw, inp.cm, scale, **ckw)
        if self.shared_guidance and active:
            # one pass: routing (and so the router masks) once, both text variants through the banks and the tail, the lerp in the egress
            self._check_shared()
            if rec is not None:                               # the egress is the combine kernel
                kw["guide_combine"] = rec
            return self.model.forward_guided(text_emb=inp.text, uncond_text_emb=inp.unc, guidance=scale, **kw)["denoised"].to(self.dtype)
        D_x = self.model(text_emb=inp.text, **kw)["denoised"].to(self.dtype)
        if not active:
            return D_x
        ref_D_x = self.gnet(text_emb=inp.unc if inp.unc is not None else inp.text, **kw)["denoised"].to(self.dtype)
        if rec is not None:
            return ops.guide_combine(ref_D_x, D_x, scale, **ckw)
        # ref.lerp(D, g) = (1-g)*ref + g*D
        if inp.g is not None:
            return ops.lerp_rows(ref_D_x, D_x, scale)
        return ops.axpby(ref_D_x, D_x, 1.0 - scale, scale)

    def _inputs(self, x, text_emb, transition_mean, softness, uncond_text_emb=None, tile=None, *, Unet_router_mask=None,
                Vit_router_mask=None, guidance=None, compose_text=None, compose_weights=None, compose_masks=None):
        """The one constructor of _Inputs, from the public arguments of sample() / denoise() under their public names; tile: None, or
        sample()'s (tile, tile_overlap, tile_window, tile_batch).  Every check first (ValueError naming the argument, host work only),
        then the tile-row repeat and the device moves.  Returns (record, _check_tile's record or None)."""
        bs, dev = x.shape[0], x.device
        comp = self._check_compose(x, text_emb, uncond_text_emb, compose_text, compose_weights, compose_masks)
        g = self._check_guidance(guidance, bs)
        um = self._router_mask(Unet_router_mask, "Unet_router_mask", bs)
        vm = self._router_mask(Vit_router_mask, "Vit_router_mask", bs)
        tile = None if tile is None else self._check_tile(x, comp, *tile)
        put = lambda a: _each(lambda t: t.to(dev).contiguous(), a)
        extra, cw, cm = comp or (None, None, None)            # composed guidance: the further conditions go behind text_emb
        texts = None if comp is None else torch.cat([text_emb.detach()[None].to(dev), extra.to(device=dev, dtype=text_emb.dtype)])
        inp = _Inputs(text_emb, uncond_text_emb, um, vm, g, texts, put(cw), put(cm), None, transition_mean, softness)
        if tile is not None and tile["plan"].T > 1:           # everything below sample() sees a plain batch of B T rows
            inp = inp.per_row(lambda a: a.repeat_interleave(tile["plan"].T, 0))
        return inp._replace(um=put(inp.um), vm=put(inp.vm), g=put(inp.g)), tile

    # ---- argument checks of the extensions: ValueError naming the argument, before any device work ------------------------------------
    def _check_shared(self, composed=False):
        """shared_guidance shares the routing of ONE network between the two text variants: the guide network must be the model itself,
        and the model must have the shared pass (composed: the pass over K + 1 variants, forward_composed)."""
        if not self.shared_guidance:
            return
        if composed and not callable(getattr(self.model, "forward_composed", None)):
            raise ValueError(f"shared_guidance=True with compose_text / compose_weights / compose_masks needs a model with "
                             f"forward_composed(); {type(self.model).__name__} has none")
        if self.gnet is not self.model:
            raise ValueError("shared_guidance=True needs Guide_net to be the model itself (a different guide network takes two passes)")
        if not callable(getattr(self.model, "forward_guided", None)):
            raise ValueError(f"shared_guidance=True needs a model with forward_guided(); {type(self.model).__name__} has none")

    @staticmethod
    def _check_number(v, name, what, ok):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number {what}, got {v!r}") from None
        if isinstance(v, bool) or not ok(f):                  # NaN fails every comparison
            raise ValueError(f"{name} must be {what}, got {v!r}")
        return f

    def combine_params(self):
        """None when neither guidance rescale nor APG is on (guided evaluations then blend as before), else the launch scalars
        (eta, norm_threshold, momentum, rescale) of the combine kernel; apg_eta None is eta = 1, the plain update."""
        if self.guidance_rescale <= 0.0 and self.apg_eta is None:
            return None
        return (1.0 if self.apg_eta is None else self.apg_eta, self.apg_norm_threshold, self.apg_momentum, self.guidance_rescale)

    def _needs_momentum(self, gvec):
        """Does a guided evaluation of this configuration carry the APG momentum buffer?"""
        return self.combine_params() is not None and self.apg_momentum != 0.0 and (gvec is not None or self.guide != 1.0)

    @property
    def guidance_interval(self):
        """None (guide every evaluation) or (lo, hi), 0 <= lo < hi <= inf: an evaluation at sigma s is guided iff lo <= s <= hi."""
        return self._interval

    @guidance_interval.setter
    def guidance_interval(self, value):
        if value is not None:
            bad = ValueError(f"guidance_interval must be None or a pair (lo, hi) of numbers with 0 <= lo < hi, got {value!r}")
            if isinstance(value, (str, bytes)) or isinstance(value, torch.Tensor) and value.ndim != 1:
                raise bad
            try:
                lo, hi = (float(v) for v in value)
            except (TypeError, ValueError):
                raise bad from None
            if not (0.0 <= lo < hi):                          # NaN fails every comparison
                raise bad
            value = (lo, hi)
        self._interval = value

    @staticmethod
    def _check_guidance(g, bs):
        """sample() / denoise() keyword `guidance`: None, or the per-sample scales as a float32 (B,) CPU tensor."""
        if g is None:
            return None
        if not isinstance(g, torch.Tensor) or g.is_complex() or g.dtype == torch.bool:
            raise ValueError(f"guidance must be None or a real tensor of shape ({bs},), got {type(g).__name__}"
                             f"{' ' + str(g.dtype) if isinstance(g, torch.Tensor) else ''}")
        if tuple(g.shape) != (bs,):
            raise ValueError(f"guidance must have shape ({bs},), one scale per sample, got {tuple(g.shape)}")
        h = g.detach().to("cpu", torch.float32)
        if not bool(torch.isfinite(h).all()):
            raise ValueError("guidance entries must be finite")
        return h

    @staticmethod
    def _check_compose(x, text_emb, uncond_text_emb, compose_text, compose_weights, compose_masks):
        """The composed-guidance keywords of sample() / denoise(): None when none of the three is given, else (extra, weights, masks) --
        the (K - 1, B, ...) further conditions, the (B, K) float32 weights (default: ones) and the (B, K, H, W) float32 masks or None.
        The rule for K = 1: composition over text_emb alone is legal, but has to be asked for with an explicit EMPTY compose_text of shape
        (0,) + text_emb.shape; weights or masks with compose_text=None are refused (a forgotten compose_text is the likelier cause)."""
        if compose_text is None and compose_weights is None and compose_masks is None:
            return None
        if compose_text is None:
            raise ValueError("compose_text is missing: compose_weights / compose_masks need it (for K = 1, the weights or masks on text_emb "
                             f"alone, pass an empty compose_text of shape {(0,) + tuple(text_emb.shape)})")
        want = tuple(text_emb.shape)
        if not isinstance(compose_text, torch.Tensor) or not compose_text.is_floating_point() or tuple(compose_text.shape[1:]) != want \
                or compose_text.ndim != len(want) + 1:
            raise ValueError(f"compose_text must be a floating-point tensor of shape (K - 1,) + {want}, the further conditions stacked, got "
                             f"{tuple(getattr(compose_text, 'shape', ())) or type(compose_text).__name__}")
        K = compose_text.shape[0] + 1
        if K > ops.COMPOSE_MAX:
            raise ValueError(f"compose_text holds {K - 1} conditions: with text_emb that is K = {K}, above the limit of {ops.COMPOSE_MAX}")
        if not isinstance(uncond_text_emb, torch.Tensor) or tuple(uncond_text_emb.shape) != want:
            raise ValueError(f"uncond_text_emb of shape {want} is required with compose_text (D_c is built on the unconditional output), got "
                             f"{tuple(getattr(uncond_text_emb, 'shape', ())) or type(uncond_text_emb).__name__}")
        bs = x.shape[0]
        if compose_weights is None:
            w = torch.ones((bs, K), dtype=torch.float32)
        else:
            if not isinstance(compose_weights, torch.Tensor) or compose_weights.is_complex() or compose_weights.dtype == torch.bool \
                    or tuple(compose_weights.shape) not in ((bs, K), (K,)):
                raise ValueError(f"compose_weights must be a real tensor of shape ({bs}, {K}) or ({K},), one weight per condition, got "
                                 f"{tuple(getattr(compose_weights, 'shape', ())) or type(compose_weights).__name__}")
            w = compose_weights.detach().to("cpu", torch.float32).expand(bs, K).contiguous()
            if not bool(torch.isfinite(w).all()):
                raise ValueError("compose_weights entries must be finite")
        m = None
        if compose_masks is not None:
            hw = tuple(x.shape[2:])
            if not isinstance(compose_masks, torch.Tensor) or not compose_masks.is_floating_point() \
                    or compose_masks.ndim not in (3, 4) or tuple(compose_masks.shape[:-2]) not in ((bs, K), (K,)):
                raise ValueError(f"compose_masks must be a floating-point tensor of shape ({bs}, {K}, H, W) or ({K}, H, W), got "
                                 f"{tuple(getattr(compose_masks, 'shape', ())) or type(compose_masks).__name__}")
            if tuple(compose_masks.shape[-2:]) != hw:
                raise ValueError(f"compose_masks must have the latents' H, W = {hw}, got {tuple(compose_masks.shape[-2:])}")
            m = compose_masks.detach().to(torch.float32)
            lo, hi = (float(v) for v in torch.aminmax(m))
            if not (0.0 <= lo and hi <= 1.0):                 # NaN fails every comparison
                raise ValueError(f"compose_masks values must be finite and lie in [0, 1], got [{lo}, {hi}]")
            m = m.expand((bs, K) + hw)
        return compose_text.detach(), w, m

    def guidance_plan(self, t_steps, i0=0):
        """Which evaluations of sample() lie in guidance_interval: one tuple of bools per stage i = i0 ... N - 1, in the order the stage
        makes its evaluations -- Heun (first, second), its last, Euler-only stage (first,), DPM-Solver++(2M) (its one,).  Pure host
        arithmetic on the float64 schedule: the first evaluation of stage i is made at t[i], or with churn (on the device too: gamma is a
        function of t[i]) at t_hat = t[i] (1 + gamma); Heun's second at t[i+1].  No interval: every flag is True."""
        N = self.num_steps
        iv = self.guidance_interval
        inside = (lambda s: True) if iv is None else (lambda s: bool(iv[0] <= s <= iv[1]))
        plan = []
        for i in range(i0, N):
            t_cur = float(t_steps[i])
            gamma = min(self.s_churn / N, np.sqrt(2) - 1) if (self.s_churn > 0 and self.s_min <= t_cur <= self.s_max) else 0
            first = inside(t_cur + gamma * t_cur)
            if self.solver == "heun" and i < N - 1:
                plan.append((first, inside(float(t_steps[i + 1]))))
            else:
                plan.append((first,))
        return plan

    def _router_mask(self, m, name, bs):
        """Checked router mask as a float32 (B, E) tensor on m's device, or None.  A row without an allowed expert is refused: the gate
        would give NaN probabilities for it and silently drop the expert output."""
        if m is None:
            return None
        E = self.model.num_experts
        if not isinstance(m, torch.Tensor):
            raise ValueError(f"{name} must be a tensor of shape ({bs}, {E}) or ({E},)")
        if m.ndim not in (1, 2) or m.shape[-1] != E or (m.ndim == 2 and m.shape[0] != bs):
            raise ValueError(f"{name} must have shape ({bs}, {E}) or ({E},), got {tuple(m.shape)}")
        if m.is_complex():
            raise ValueError(f"{name} must be real with {{0, 1}} entries, got {m.dtype}")
        h = m.detach().to("cpu", torch.float64)
        if not bool(((h == 0) | (h == 1)).all()):
            raise ValueError(f"{name} entries must be 0 or 1")
        if bool((h.sum(-1) == 0).any()):
            raise ValueError(f"{name} has a row with no allowed expert")
        return m.detach().to(torch.float32).expand(bs, E)

    @staticmethod
    def _check_seed(seed):
        if seed is None:
            return None
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must be an int in [0, 2^64) or None, got {seed!r}")
        return int(seed)

    def _check_conditioning(self, noise, init_latents, strength, inpaint_mask):
        try:
            strength = float(strength)
        except (TypeError, ValueError):
            raise ValueError(f"strength must be a number in (0, 1], got {strength!r}") from None
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength must be in (0, 1], got {strength}")
        if init_latents is not None:
            if not isinstance(init_latents, torch.Tensor) or not init_latents.is_floating_point():
                raise ValueError("init_latents must be a floating-point tensor")
            if tuple(init_latents.shape) != tuple(noise.shape):
                raise ValueError(f"init_latents must have the shape of noise {tuple(noise.shape)}, got {tuple(init_latents.shape)}")
        elif strength < 1.0:
            raise ValueError(f"strength < 1 (got {strength}) needs init_latents")
        if inpaint_mask is not None:
            if init_latents is None:
                raise ValueError("inpaint_mask needs init_latents (the content of the known region)")
            if not isinstance(inpaint_mask, torch.Tensor) or inpaint_mask.dtype != torch.float32:
                raise ValueError(f"inpaint_mask must be a float32 tensor, got {getattr(inpaint_mask, 'dtype', type(inpaint_mask))}")
            if inpaint_mask.ndim != 4:
                raise ValueError(f"inpaint_mask must be 4-D, got shape {tuple(inpaint_mask.shape)}")
            try:
                ok = torch.broadcast_shapes(inpaint_mask.shape, noise.shape) == noise.shape
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError(f"inpaint_mask of shape {tuple(inpaint_mask.shape)} does not broadcast to noise {tuple(noise.shape)}")
            lo, hi = (float(v) for v in torch.aminmax(inpaint_mask.detach()))
            if not (0.0 <= lo and hi <= 1.0):
                raise ValueError(f"inpaint_mask values must lie in [0, 1], got [{lo}, {hi}]")
        return strength

    # ---- static state and hipGraph capture: fused solver stages (reference :90-107 without churn), the captured evaluation ----------------
    def _check_tile(self, noise, comp, tile, tile_overlap, tile_window, tile_batch):
        """The tiling keywords of sample(): None without `tile`, else the record {"plan": ops.TilePlan, "tb": tile rows per model call,
        "key": what a capture bakes in}.  Host arithmetic only."""
        if tile is None:
            return None
        try:
            h, w = (int(v) for v in tile)
        except (TypeError, ValueError):
            raise ValueError(f"tile must be None or a pair (h, w) of ints, the model's latent size, got {tile!r}") from None
        if noise.ndim != 4 or h < 1 or w < 1 or noise.shape[2] < h or noise.shape[3] < w:
            raise ValueError(f"tile=({h}, {w}) needs (B, C, H, W) latents with H >= {h} and W >= {w}, got noise of shape {tuple(noise.shape)}")
        if comp is not None:
            raise ValueError("tile does not combine with composed guidance (compose_text / compose_weights / compose_masks): the spatial "
                             "masks would have to be tiled too")
        if self.combine_params() is not None:
            raise ValueError("tile does not combine with guidance_rescale or apg_eta / apg_norm_threshold / apg_momentum: their per-sample "
                             "statistics and momentum would become per-tile ones")
        B, _, H, W = (int(v) for v in noise.shape)
        try:
            plan = ops.tile_plan(H, W, h, w, tile_overlap, tile_window)
        except ValueError as e:
            raise ValueError(f"tile / tile_overlap / tile_window: {e}") from None
        n = B * plan.T
        tb = n if tile_batch is None else tile_batch
        if isinstance(tb, bool) or not isinstance(tb, numbers.Integral) or tb < 1 or n % int(tb):
            raise ValueError(f"tile_batch must be a positive int dividing B * T = {B} * {plan.T} = {n}, got {tile_batch!r}")
        return dict(plan=plan, tb=int(tb), key=((h, w), plan.overlap, plan.window, int(tb), H, W))

    def _tile_bufs(self, tile, x):
        """The tile record with its device side: the plan's arrays on x's device, the gather target "xt" (tb, C, h, w) and, when an
        evaluation takes more than one model call, the tile buffer "buf" (B T, C, h, w) the chunks' outputs are collected in (fp32)."""
        plan, tb = tile["plan"], tile["tb"]
        plan.device(x.device)
        B, C = x.shape[:2]
        mk = lambda rows: torch.empty((rows, C, plan.h, plan.w), dtype=torch.float32, device=x.device)
        return dict(tile, xt=mk(tb), buf=mk(B * plan.T) if tb < B * plan.T else None)

    def _denoise_tiled(self, tile, x, sigma, inp, guided):
        """_denoise() of a latent larger than the model: den_big = blend(model(gather(x_big))).  x keeps its B rows; every per-row operand
        of inp (text, masks, scales) has B T rows, tile-batch order.  Per chunk of tb rows: ops.tile_gather, _denoise, and (more than one
        chunk) one copy_ into the tile buffer; then ONE ops.tile_blend.  The tile kernels are fp32: other latent dtypes are cast on the
        way in and out, as _denoise casts the model's output.  No host read: it runs under stream capture like _denoise."""
        plan, tb = tile["plan"], tile["tb"]
        n = x.shape[0] * plan.T
        xf = x.to(torch.float32).contiguous()
        for r0 in range(0, n, tb):
            sl = slice(r0, r0 + tb)
            xt = ops.tile_gather(xf, plan, r0, tb, out=tile["xt"])
            d = self._denoise(xt.to(self.dtype), sigma, inp if tb == n else inp.per_row(lambda a: a[sl]), guided)
            if tb == n:
                tiles = d.to(torch.float32).contiguous()      # one chunk: blended from where the model left it
            else:
                tiles = tile["buf"]
                tiles[sl].copy_(d)
        return ops.tile_blend(tiles, plan, x.shape[0]).to(self.dtype)

    def _stage_state(self, kind, x, inp, tile=None):
        """Static buffers, stage functions and (use_graph) captured graphs of one kind, for the latents x and the operands inp (_Inputs):
          "eval": one guided evaluation of x at sig into out (the host loops' evaluation with use_graph);
          "heun": a full Heun stage and the last, Euler-only stage; "dpm": one DPM-Solver++(2M) stage (den_prev: the previous stage's
                  denoiser output, read and overwritten element by element by the step kernel; i0: the first stage run).
        The stage kinds take sigma from the schedule t (float64, as the host computes it) at the device stage index idx, and the kernels pick
        the order on the device, so any strength shares one capture.  The SAME stage function runs eagerly and under capture: the two
        trajectories are bit-identical.  The key holds everything a capture bakes in -- shapes, which optional operands exist, and what
        _denoise reads on the host (guide, the two modules), the churn / SDE launch scalars -- never buffer values: every input, the seed of
        the stochastic stages included (device word "seed") and the operands (the record "inp"), is refreshed before each run.
        combine_params() -- launch scalars of the combine kernel -- are in the key; the APG momentum ("mom", float32, None without
        apg_momentum) is a buffer value: _refresh zeroes it at the start of a sample() call, every guided evaluation updates it in place.

        With a guidance interval (and guidance in effect) every stage function exists once per variant -- which of its evaluations are
        guided -- and with use_graph each variant is one graph, all in one pool over the same buffers: "sel" maps a stage's tuple of
        guidance_plan() to its index in "fns" / "g_<kind>", so the interval's bounds are a host selection and not in the key.  Without an
        interval the lists are the all-guided ones alone: two for "heun" (full, last), one for "dpm" and "eval".

        Composed guidance: its texts, weights and masks are static buffers refreshed like every input; K and whether there are masks
        are the key's second entry.  The "eval" kind reads no known region (the host loops blend it themselves): it drops inp.known.
        tile (tiled sampling, _check_tile's record): every evaluation of the state is _denoise_tiled.  x keeps its B rows, the per-row
        operands come with B T rows; the plan's device arrays and the tile buffers are part of the state ("tile"), and the tile spec --
        (h, w), the overlaps, the window, tile_batch, H, W -- is one more key entry, present only with tiling."""
        if kind == "eval":
            inp = inp._replace(known=None)
        variants = self.guidance_interval is not None and (inp.g is not None or self.guide != 1.0)
        key = (kind, None if inp.texts is None else (int(inp.texts.shape[0]), inp.cm is not None), self.solver, tuple(x.shape), x.dtype) \
            + (() if tile is None else (("tile",) + tile["key"],)) + (
               inp.signature(), self.num_steps, bool(self.use_graph), float(self.guide), id(self.model), id(self.gnet), float(self.s_churn),
               float(self.s_min), float(self.s_max), float(self.s_noise), float(self.eta), bool(self.churn_on_device), self.combine_params(),
               inp.g is not None, variants, bool(self.shared_guidance))
        slot = "_graph" if kind == "eval" else "_stage"          # one cached state for the evaluation, one for the solver stage
        st = getattr(self, slot)
        if st is not None and st["key"] == key:
            return st
        dev, static = x.device, inp.empty_like()
        # the record's fields under their own names too ("known": the stage functions read it).  mods: held so that their ids, in the
        # key, cannot be reused by other modules while this capture lives
        st = dict(static._asdict(), key=key, x=torch.empty_like(x), sig=torch.ones((), dtype=self.dtype, device=dev), inp=static,
                  variants=variants, mods=(self.model, self.gnet),
                  mom=torch.zeros(x.shape, dtype=torch.float32, device=dev) if self._needs_momentum(inp.g) else None,
                  tile=None if tile is None else self._tile_bufs(tile, x))
        self._refresh(st, x, inp)

        def den(x_, guided):
            return (self._denoise(x_, st["sig"], static, guided, st["mom"]) if st["tile"] is None else
                    self._denoise_tiled(st["tile"], x_, st["sig"], static, guided))

        def pick(j):                                          # sig = t[idx + j]
            ops.call("hdmoe_sched_pick", st["sig"], st["t"], st["idx"], j)

        churn = self.s_churn > 0                              # a fused Heun stage with churn: churn_on_device (sample() decides)
        gamma_cap = float(min(self.s_churn / self.num_steps, np.sqrt(2) - 1))

        def heun(last: bool, g1: bool = True, g2: bool = True):  # g1 / g2: is the first / second evaluation guided
            if churn:                                         # x <- x_hat in place, sig = t_hat; the updates then start from t_hat
                ops.heun_churn(st["x"], st["x"], st["sig"], st["t_hat"], st["t"], st["idx"], st["seed"], gamma_cap, self.s_min, self.s_max,
                               self.s_noise)
            else:
                pick(0)
            that = st["t_hat"] if churn else None
            d = den(st["x"], g1)
            if last:
                ops.heun_euler(st["x"], st["x"], d, st["t"], st["idx"], st["known"], that)
            else:
                ops.heun_euler(st["xn"], st["x"], d, st["t"], st["idx"], st["known"], that)
                pick(1)
                ops.heun_correct(st["x"], st["x"], d, st["xn"], den(st["xn"], g2), st["t"], st["idx"], st["known"], that)
            ops.call("hdmoe_idx_advance", st["idx"])

        def dpm(g1: bool = True):
            pick(0)
            if self.solver == "dpmpp_2m_sde":
                ops.dpm2m_sde_step(st["x"], st["x"], den(st["x"], g1), st["den_prev"], st["t"], st["idx"], st["i0"], self.eta, self.s_noise,
                                   st["seed"], st["known"])
            else:
                ops.dpm2m_step(st["x"], st["x"], den(st["x"], g1), st["den_prev"], st["t"], st["idx"], st["i0"], st["known"])
            ops.call("hdmoe_idx_advance", st["idx"])

        def evaluate(g1: bool = True):                        # each variant keeps its own output alive in the shared pool
            st["out" if g1 else "out_plain"] = den(st["x"], g1)

        if kind != "eval":
            st.update(t=torch.ones(self.num_steps + 1, dtype=torch.float64, device=dev), idx=torch.zeros(1, dtype=torch.int32, device=dev),
                      seed=torch.zeros(1, dtype=torch.int64, device=dev))      # the call's 64-bit seed (two's complement of the unsigned value)
        if kind == "heun":
            st["xn"] = torch.empty_like(x)                    # the Euler predictor
            st["t_hat"] = torch.ones(1, dtype=torch.float64, device=dev)       # the churned sigma of the current stage
        if kind == "dpm":
            st.update(den_prev=torch.zeros_like(x), i0=torch.zeros(1, dtype=torch.int32, device=dev))
        if not variants:
            st["fns"] = {"eval": [evaluate], "heun": [lambda: heun(False), lambda: heun(True)], "dpm": [dpm]}[kind]
            st["sel"] = {"heun": {(True, True): 0, (True,): 1}}.get(kind, {(True,): 0})
        else:                                                 # the all-guided variant first: the warm-up runs size the pool with it
            one = {"eval": evaluate, "heun": lambda a: heun(True, a), "dpm": dpm}[kind]
            keys = [(a, b) for a in (True, False) for b in (True, False)] if kind == "heun" else []
            keys += [(True,), (False,)]
            st["fns"] = [(lambda k=k: heun(False, *k)) if len(k) == 2 else (lambda k=k: one(*k)) for k in keys]
            st["sel"] = {k: n for n, k in enumerate(keys)}
        st["g_" + kind] = self._capture(st, warmup=3 if kind == "eval" else 2, warm_all=variants) if self.use_graph else []
        setattr(self, slot, st)
        return st

    @staticmethod
    def _capture(st, warmup, warm_all=False):
        """One graph per stage function of st, all in one memory pool, after `warmup` runs of the first on a side stream (they register the
        weight bank and size the allocator pool) and, with warm_all (the guidance-interval variants), one run of each of the others: a
        variant may be the first to make the plain model call.  The device stage indices restart at 0 before every run."""
        def restart():
            for k in ("idx", "i0"):
                if k in st:
                    st[k].zero_()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for fn in [st["fns"][0]] * warmup + (st["fns"][1:] if warm_all else []):
                restart()
                fn()
        torch.cuda.current_stream().wait_stream(side)
        restart()
        graphs = []
        with hgraph.no_gc():
            for fn in st["fns"]:
                graphs.append(torch.cuda.CUDAGraph())
                with torch.cuda.graph(graphs[-1], pool=graphs[0].pool() if len(graphs) > 1 else None):
                    fn()
        return graphs

    @staticmethod
    def _refresh(st, x, inp, seed=None, reset_momentum=True):
        """Every input into the static buffers: a later sample() with another prompt of the same shape must not see the captured one.
        seed: the 64-bit seed of this call's stochastic stages (a buffer value like the others, never part of the capture key).
        reset_momentum: zero the APG momentum -- the start of a sample() call (the warm-up runs of a capture have written it too); the
        captured evaluation of the host loops keeps it from one evaluation of a call to the next."""
        if reset_momentum and st["mom"] is not None:
            st["mom"].zero_()
        if seed is not None:
            st["seed"].fill_(seed - (1 << 64) if seed >= 1 << 63 else seed)
        st["x"].copy_(x)
        st["inp"].copy_from(inp)

    @staticmethod
    def _eps(x, seed, stage):
        """The stage's standard normals in x's dtype: keyed by (seed, stage) like the fused stages, or from the library's stream (seed None)."""
        eps = ops.randn_like(x, 1.0) if seed is None else ops.randn_keyed(x, seed, stage)
        return eps.to(x.dtype)

    def _dpm_host_loop(self, x, t_steps, inp, seed, plan, mom, tile):
        """solver="dpmpp_2m" / "dpmpp_2m_sde" for latents the fused stage does not take (non-fp32 dtype): the rule of sample() with host
        coefficients.  plan: guidance_plan() of the stages run, i0 ... N - 1."""
        N, known, i0 = self.num_steps, inp.known, self.num_steps - len(plan)
        sde = self.solver == "dpmpp_2m_sde"
        den_prev = None
        for i in range(i0, N):
            t_cur, t_next = float(t_steps[i]), float(t_steps[i + 1])
            den = self._eval(x, t_cur, inp, plan[i - i0][0], mom, i == i0, tile)
            e = math.exp(-self.eta * math.log(t_cur / t_next)) if sde and t_next > 0 else 1.0
            a = t_next / t_cur * e
            if t_next == 0:
                x = den.clone()
            elif i == i0:
                x = ops.axpby(x, den, a, 1.0 - a)
            else:
                hr = 0.5 * math.log(t_cur / t_next) / math.log(float(t_steps[i - 1]) / t_cur)      # 1 / (2 r)
                x = ops.axpby(x, ops.axpby(den, den_prev, 1.0 + hr, -hr), a, 1.0 - a)
            if sde and self.eta > 0 and t_next > 0:
                x = ops.axpby(x, self._eps(x, seed, i), 1.0, t_next * math.sqrt(1.0 - e * e) * self.s_noise)
            if known is not None:
                ops.known_blend_(x, *known, t_next)
            den_prev = den
        return x

    def _heun_host_loop(self, x_next, t_steps, inp, seed, plan, mom, tile):
        """solver="heun" for what the fused stage does not take (host churn, non-fp32 latents): the reference's loop (:90-107), every
        latent update a fused launch.  plan: guidance_plan() of the stages run, i0 ... N - 1."""
        N, known, i0 = self.num_steps, inp.known, self.num_steps - len(plan)
        for i in range(i0, N):
            t_cur, t_next = float(t_steps[i]), float(t_steps[i + 1])
            gamma = min(self.s_churn / self.num_steps, np.sqrt(2) - 1) if (self.s_churn > 0 and self.s_min <= t_cur <= self.s_max) else 0
            t_hat = t_cur + gamma * t_cur
            x_hat = x_next
            if gamma > 0:
                x_hat = ops.axpby(x_next, self._eps(x_next, seed, i), 1.0, float(np.sqrt(t_hat ** 2 - t_cur ** 2) * self.s_noise))
            denoised = self._eval(x_hat, t_hat, inp, plan[i - i0][0], mom, i == i0, tile)
            # d_cur = (x_hat - denoised)/t_hat ; x_next = x_hat + (t_next - t_hat) * d_cur
            h = (t_next - t_hat)
            x_next = ops.axpby(x_hat, denoised, 1.0 + h / t_hat, -h / t_hat)
            if known is not None:
                ops.known_blend_(x_next, *known, t_next)
            if i < self.num_steps - 1:
                den2 = self._eval(x_next, t_next, inp, plan[i - i0][1], mom, False, tile)
                # x_next = x_hat + h * (0.5*d_cur + 0.5*d_prime),  d_prime = (x_next - den2)/t_next
                d_cur_term = ops.axpby(x_hat, denoised, 1.0 + 0.5 * h / t_hat, -0.5 * h / t_hat)     # x_hat + 0.5 h d_cur
                d_pr = ops.axpby(x_next, den2, 0.5 * h / t_next, -0.5 * h / t_next)                  # 0.5 h d_prime
                x_next = ops.axpby(d_cur_term, d_pr, 1.0, 1.0)
                if known is not None:
                    ops.known_blend_(x_next, *known, t_next)
        return x_next

    def _eval(self, x, t, inp, guided, mom, first, tile):
        """One evaluation at sigma t of the host loops; guided: the solver's guidance-interval decision for it.  mom: the call's APG
        momentum buffer (eager); the captured evaluation carries its own, zeroed on the first evaluation of a call.  tile: the tile
        record of a tiled call (eager: with this call's buffers, _tile_bufs); the evaluation is then _denoise_tiled."""
        if not self.use_graph:
            sig = torch.tensor(t, dtype=self.dtype, device=x.device)
            return self._denoise(x, sig, inp, guided, mom) if tile is None else self._denoise_tiled(tile, x, sig, inp, guided)
        st = self._stage_state("eval", x, inp, tile)
        self._refresh(st, x, inp, reset_momentum=first)
        st["sig"].fill_(float(t))
        guided = bool(guided) or not st["variants"]
        st["g_eval"][st["sel"][(guided,)]].replay()
        return st["out" if guided else "out_plain"].clone()

    def t_schedule(self, device):
        """Karras rho schedule with the appended 0 (reference :80-87), computed on the host in float64."""
        i = np.arange(self.num_steps, dtype=np.float64)
        t = (self.sigma_max ** (1 / self.rho) + i / (self.num_steps - 1) *
             (self.sigma_min ** (1 / self.rho) - self.sigma_max ** (1 / self.rho))) ** self.rho
        return np.concatenate([t, [0.0]])

    @torch.no_grad()
    def sample(self, noise: torch.Tensor, text_emb: torch.Tensor, transition_mean: float, softness: float,
               uncond_text_emb: torch.Tensor = None, *, init_latents: torch.Tensor = None, strength: float = 1.0,
               inpaint_mask: torch.Tensor = None, Unet_router_mask: torch.Tensor = None, Vit_router_mask: torch.Tensor = None,
               seed: int = None, guidance: torch.Tensor = None, compose_text: torch.Tensor = None, compose_weights: torch.Tensor = None,
               compose_masks: torch.Tensor = None, tile=None, tile_overlap=0, tile_window: str = "feather",
               tile_batch: int = None) -> torch.Tensor:
        """Solve of the probability-flow ODE over t = t_schedule() (N = num_solve_steps, t[N] = 0): Heun (solver="heun", the reference),
        or DPM-Solver++(2M) (solver="dpmpp_2m", one evaluation per stage).

        solver="dpmpp_2m" runs, for i = i0 ... N - 1, with D_i the (guided) denoiser output at t[i] and a = t[i+1] / t[i]:
            t[i+1] == 0:  x = D_i                                       (last stage)
            i == i0:      x = a x + (1 - a) D_i                         (no history yet: first order)
            otherwise:    x = a x + (1 - a) ((1 + 1/(2r)) D_i - 1/(2r) D_{i-1}),   r = log(t[i-1] / t[i]) / log(t[i] / t[i+1])
        then the inpainting blend below at sigma = t[i+1], and D_{i-1} <- D_i: n_run evaluations per network.  It takes every keyword below.

        solver="dpmpp_2m_sde" (DPM-Solver++(2M) SDE, midpoint form) is the same with e = exp(-eta log(t[i] / t[i+1])): a = (t[i+1] / t[i]) e
        in place of a above, and, except on the last stage and when eta == 0, x += t[i+1] sqrt(1 - e^2) S_noise eps_i before the blend.
        eta = 0 is solver="dpmpp_2m" bit-for-bit.

        Churn (S_churn > 0, solver="heun", reference :90-97): stage i starts from t_hat = t[i] (1 + gamma), x_hat = x + sqrt(t_hat^2 - t[i]^2)
        S_noise eps_i, gamma = min(S_churn / N, sqrt(2) - 1) where S_min <= t[i] <= S_max, else 0.  It runs on the host-driven loop unless
        churn_on_device=True (fp32 latents on the GPU), which runs it inside the fused stage.

        eps_i, one standard normal per latent element, is what hdmoe_randn draws under the key (seed, i) -- ops.randn_keyed(x, seed, i).

        Keywords beyond the reference (every default reproduces the plain sampler):
          strength:       in (0, 1]; the solver runs the last n_run = ceil(strength * N) stages, i0 = N - n_run ... N - 1, i.e. 2 n_run - 1
                          evaluations per network with Heun, n_run with DPM-Solver++(2M).  Below 1 it needs init_latents.
          init_latents:   x0, the shape of noise.  Start x = x0 + t[i0] * noise (image-to-image); without it x = t[i0] * noise.  This holds
                          under the inpainting mask too: whatever x0 holds in the hole enters at 1 / t[i0] of the noise scale (zero the hole
                          to avoid that).
          inpaint_mask:   m, float32 in [0, 1] (1 = keep), any 4-D shape broadcasting to noise; needs init_latents.  Wherever a stage
                          produces latents at sigma = t[i+1] (the Euler predictor, the Heun-corrected output, the last Euler-only output, each
                          DPM-Solver++(2M) update):
                          x <- m (x0 + sigma noise) + (1 - m) x, so where m = 1 the output is x0 exactly.  Soft masks blend.
          seed:           int in [0, 2^64) or None.  The fused stochastic stages draw from it; None takes the next value of the library's
                          seed stream (ops.manual_seed), once per call.  The host loops draw under the same (seed, stage) key when it is
                          given -- so they see the eps of the fused path -- and from the library's stream per stage, as before, when it is
                          None.  A configuration that draws nothing ignores it.
          Unet_router_mask / Vit_router_mask:  (B, E) or (E,) with {0, 1} entries, passed to the model and the guide network; None = all
                          experts.  A row with no allowed expert is refused.
          guidance:       None = the sampler's float scale (baked into a capture, as before), or a (B,) tensor of finite per-sample
                          scales on any device.  It is copied into a static device buffer like every other input and read there by the
                          blend (ops.lerp_rows, two-pass) or the egress (shared_guidance): one batch can carry a sweep of scales, and
                          another vector of the same shape replays the same capture.

        guidance_interval = (lo, hi) (constructor argument / attribute; None = guide everywhere): an evaluation made at sigma s is guided iff
        lo <= s <= hi, otherwise it is the ONE plain conditional call that guidance == 1 makes.  s is t[i] for a stage's first evaluation
        (t_hat with churn), t[i+1] for Heun's second; guidance_plan() lists the decisions and last_evaluations counts them after each call.
        With DPM-Solver++(2M) the history term D_{i-1} is whatever stage i - 1 evaluated: across an interval boundary the extrapolation
        mixes a guided and a plain output -- that is the formula applied to the gated denoiser, not an error.  With use_graph every stage
        variant is captured once; calls that differ in the bounds replay the same graphs.

        guidance_rescale / apg_eta / apg_norm_threshold / apg_momentum (constructor arguments): with w the scale, D_c / D_u the two
        denoiser outputs of a guided evaluation and all sums over one sample, the guided output is
            M = (D_c - D_u) + apg_momentum M_prev;   s = min(1, apg_norm_threshold / |M|);   c = <M, D_c> / |D_c|^2
            O = D_c + (w - 1) s (M - (1 - apg_eta) c D_c);   out = (guidance_rescale std(D_c) / std(O) + 1 - guidance_rescale) O
        (apg_eta None: eta = 1, no clamp, no momentum, i.e. O = (1 - w) D_u + w D_c).  M_prev is zero at the start of every call and is
        updated by the guided evaluations in the order the solver makes them; evaluations outside guidance_interval leave it alone.

        compose_text / compose_weights / compose_masks (composed guidance; all None: off).  The K conditions are text_emb and the K - 1
        rows of compose_text, (K - 1, B, S, D), K <= 8; uncond_text_emb is required.  compose_weights: (B, K) or (K,), finite, any sign,
        default ones; compose_masks: (B, K, H, W) or (K, H, W) in [0, 1] at the latents' H, W, default none.  Per element, in fp32,
            c_k = weights[n, k] masks[n, k, p];   c_0 = 1 - sum_k c_k;   D_c = c_0 D_u + sum_k c_k D_k
        and D_c replaces the conditional output D_c in the formulas above (scale, per-sample scales, rescale, APG).  An evaluation outside
        guidance_interval is out = D_c (the same evaluation at scale 1, momentum untouched): guidance_plan and last_evaluations keep their
        meaning, but a "plain" evaluation costs what a guided one does.  K = 1 (weights or masks on text_emb alone) has to be asked for
        with an empty compose_text of shape (0, B, S, D); weights or masks without compose_text are refused.  With use_graph the extra
        text, the weights and the masks are static buffers: other values of the same K replay the same capture.

        tile / tile_overlap / tile_window / tile_batch (tiled sampling of latents larger than the model's resolution, MultiDiffusion
        style; tile=None: off, nothing changes).  tile = (h, w) is the model's own latent size; noise, init_latents, inpaint_mask and the
        result are (B, C, H, W) with H >= h, W >= w.  The solver updates are pointwise and run on the large latent unchanged; every
        denoiser evaluation is den_big = blend(model(gather(x_big))) over the T = Ty Tx windows of ops.tile_plan(H, W, h, w, tile_overlap,
        tile_window): along an axis of length L with tile length n and overlap o (an int, or (oy, ox) in tile_overlap; 0 <= o < n) the
        stride is n - o, there are 1 + ceil((L - n) / (n - o)) tiles (at most 32) and the last is clamped to the edge.  tile_window:
        "uniform" (plain average over the covering tiles) or "feather" (1-D weight min(i + 1, n - i, r) / r, r = max(o, 1), normalised
        over the covering tiles).  A position under one tile takes that tile's output bit for bit.  text_emb, uncond_text_emb, the router
        masks and the per-sample guidance vector are repeated T times per sample, so guidance, the interval, per-sample scales and the
        masks apply per tile row.  tile_batch: tile rows per model call, a divisor of B T (default B T, one call per evaluation).
        Every solver, churn_on_device, use_graph, image-to-image, strength, inpainting, seed and non-fp32 dtype (host loops; the tile
        kernels run in fp32) work with it; with use_graph the tile spec is part of the capture key, and a second call of the same shapes
        replays the same graphs.  Refused (ValueError naming tile): composed guidance (its spatial masks would have to be tiled too),
        guidance_rescale and apg_* (their per-sample statistics and momentum would become per-tile ones).
        Argument errors raise ValueError (naming the argument) before any device work."""
        strength = self._check_conditioning(noise, init_latents, strength, inpaint_mask)
        seed = self._check_seed(seed)
        inp, tile = self._inputs(noise, text_emb, transition_mean, softness, uncond_text_emb, (tile, tile_overlap, tile_window, tile_batch),
                                 Unet_router_mask=Unet_router_mask, Vit_router_mask=Vit_router_mask, guidance=guidance,
                                 compose_text=compose_text, compose_weights=compose_weights, compose_masks=compose_masks)
        device = noise.device
        if self.use_graph:
            # the captured evaluation holds no weight-prepare launch when the images were current at capture time: refresh them here,
            # eagerly, in case the parameters changed since (new checkpoint, an optimizer step)
            from hdmoe_hip import bank as wbank
            for m_ in {id(self.model): self.model, id(self.gnet): self.gnet}.values():
                if isinstance(m_, nn.Module) and getattr(m_, "_hdmoe_bank", None) is not None:
                    m_._hdmoe_bank.refresh_eval()
        i0 = self.num_steps - math.ceil(strength * self.num_steps)
        t_steps = self.t_schedule(device)
        # the guidance-interval decision of every evaluation, taken here, on the host, from the float64 sigmas: denoise() never reads sigma
        plan = self.guidance_plan(t_steps, i0)
        n_guided = sum(map(sum, plan)) if (inp.g is not None or self.guide != 1.0) else 0
        self.last_evaluations = {"guided": n_guided, "plain": sum(map(len, plan)) - n_guided}
        if init_latents is None:
            x_next = ops.axpby(noise.to(self.dtype), None, float(t_steps[i0]), 0.0)
        else:
            lat = noise.to(self.dtype).contiguous()
            x0 = init_latents.to(device=device, dtype=self.dtype).contiguous()
            x_next = ops.axpby(x0, lat, 1.0, float(t_steps[i0]))
            if inpaint_mask is not None:                      # expanded once per call: the kernels read a mask of the latents' size
                inp = inp._replace(known=(x0, lat, inpaint_mask.to(device).expand(noise.shape).contiguous()))
        fused = bool((self.s_churn <= 0 or self.churn_on_device) and self.dtype == torch.float32 and noise.is_cuda and self.num_steps >= 2)
        self.fused_heun = fused and self.solver == "heun"
        self.fused_dpm = fused and self.solver != "heun"
        if fused:
            # the whole solver runs from a device-side schedule (fused churn / Euler / Heun-correction kernels, or the DPM-Solver++(2M) step
            # kernel, no host arithmetic between the evaluations); with use_graph each stage is one hipGraph replay
            kind = "heun" if self.fused_heun else "dpm"
            if seed is None and (self.s_churn > 0 or (self.solver == "dpmpp_2m_sde" and self.eta > 0)):
                seed = ops.next_seed()                        # a stochastic stage: one value of the library's stream per call
            st = self._stage_state(kind, x_next, inp, tile)
            self._refresh(st, x_next, inp, seed)
            st["t"].copy_(torch.from_numpy(t_steps))
            st["idx"].fill_(i0)
            if self.fused_dpm:
                st["i0"].fill_(i0)
            runs = [g.replay for g in st["g_" + kind]] or st["fns"]
            for flags in plan:                                # Heun: the Euler-only stage last; DPM: its one stage throughout
                runs[st["sel"][flags if st["variants"] else (True,) * len(flags)]]()
            return st["x"].clone()
        # host loops: this call's APG momentum (the captured evaluation of use_graph holds its own and zeroes it on the first evaluation)
        mom = torch.zeros(x_next.shape, dtype=torch.float32, device=device) if self._needs_momentum(inp.g) and not self.use_graph else None
        if tile is not None and not self.use_graph:           # this call's tile buffers (the captured evaluation holds its own)
            tile = self._tile_bufs(tile, x_next)
        loop = self._heun_host_loop if self.solver == "heun" else self._dpm_host_loop
        return loop(x_next, t_steps, inp, seed, plan, mom, tile)
