"""EDM_Sampler extensions: image-to-image (init_latents + strength), inpainting (inpaint_mask) and router masks at sampling time.

CPU tests: every argument check raises ValueError naming the argument before any device work.  GPU tests: the trajectory against a
float64 restatement of the rules (Utils/EDM_sampler.py, sample() docstring), the known region exact, eager vs hipGraph replay on the
real model (including three different conditionings through one capture), and router masks passed through to the model."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils"))

from EDM_sampler import EDM_Sampler  # noqa: E402

DEV = "cuda"
gpu = pytest.mark.gpu


class _MockDenoiser(torch.nn.Module):
    """Linear mock denoiser (the role of the reference's tests/test_utilities/test_sampler.py mock); counts its calls and records the
    router masks it was given."""

    def __init__(self, scale, num_experts=4):
        super().__init__()
        self.num_experts = num_experts
        self.scale = scale
        self.calls = 0
        self.masks = []

    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, transition_point, softness, return_log_var=False):
        self.calls += 1
        assert sigma.ndim == 0 and Unet_router_mask.shape == (x.shape[0], self.num_experts) and zeta == 0
        self.masks.append((Unet_router_mask, Vit_router_mask))
        return {"denoised": x * self.scale}


def close_scaled(a, b, rel, msg="", atol=1e-6):
    """max|a-b| <= rel * max|b| + atol (the sampler tests' tolerance form)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{msg}: non-finite output"
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= rel * scale + atol, f"{msg}: max err {err:.3e} > {rel:.1e} * {scale:.3e} + {atol:.0e}"


def schedule(N, sigma_min=0.002, sigma_max=80.0, rho=7):
    i = torch.arange(N, dtype=torch.float64)
    t = (sigma_max ** (1 / rho) + i / (N - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros(1, dtype=torch.float64)])


def restate(noise, N, guide, strength, x0=None, m=None, s_model=0.9, s_gnet=0.5):
    """float64 CPU restatement: start at i0 = N - ceil(strength N) from x0 + t[i0] noise, blend m (x0 + sigma noise) + (1 - m) x wherever a
    stage produces latents at sigma = t[i+1]."""
    t = schedule(N)
    i0 = N - math.ceil(strength * N)
    noise = noise.cpu().double()
    x0 = None if x0 is None else x0.cpu().double()
    m = None if m is None else m.cpu().double()
    den = (lambda x: (s_gnet * x).lerp(s_model * x, guide)) if guide != 1.0 else (lambda x: s_model * x)
    blend = (lambda x, s: x) if m is None else (lambda x, s: m * (x0 + s * noise) + (1 - m) * x)
    x = t[i0] * noise if x0 is None else x0 + t[i0] * noise
    for k in range(i0, N):
        d = (x - den(x)) / t[k]
        xn = blend(x + (t[k + 1] - t[k]) * d, t[k + 1])
        if k < N - 1:
            dp = (xn - den(xn)) / t[k + 1]
            xn = blend(x + (t[k + 1] - t[k]) * (0.5 * d + 0.5 * dp), t[k + 1])
        x = xn
    return x


# ----------------------------------------------------------------------------------------------- CPU: argument checks
def _cpu_args(B=2):
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 5, 16, generator=g)


def _raises(name, **kw):
    noise, text = _cpu_args()
    s = EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4)
    with pytest.raises(ValueError, match=name):
        s.sample(noise, text, -1.2, 1.6, **kw)
    assert s._stage is None and s._graph is None


@pytest.mark.parametrize("strength", [0.0, -0.5, 1.5, float("nan")])
def test_strength_out_of_range(strength):
    _raises("strength", init_latents=torch.zeros(2, 4, 8, 8), strength=strength)


def test_strength_below_one_needs_init_latents():
    _raises("init_latents", strength=0.5)


def test_inpaint_mask_needs_init_latents():
    _raises("inpaint_mask", inpaint_mask=torch.ones(2, 1, 8, 8))


@pytest.mark.parametrize("shape", [(2, 1, 4, 8), (3, 1, 8, 8), (2, 4, 8), (1, 2, 1, 8, 8)])
def test_inpaint_mask_must_broadcast(shape):
    _raises("inpaint_mask", init_latents=torch.zeros(2, 4, 8, 8), inpaint_mask=torch.ones(shape))


def test_inpaint_mask_dtype_and_range():
    _raises("inpaint_mask", init_latents=torch.zeros(2, 4, 8, 8), inpaint_mask=torch.ones(2, 1, 8, 8, dtype=torch.float64))
    _raises("inpaint_mask", init_latents=torch.zeros(2, 4, 8, 8), inpaint_mask=torch.full((2, 1, 8, 8), 1.5))


@pytest.mark.parametrize("shape", [(2, 4, 8, 4), (1, 4, 8, 8), (2, 4, 64)])
def test_init_latents_shape(shape):
    _raises("init_latents", init_latents=torch.zeros(shape))


@pytest.mark.parametrize("name", ["Unet_router_mask", "Vit_router_mask"])
def test_router_mask_rows_and_shape(name):
    _raises(name, **{name: torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])})    # second row allows no expert
    _raises(name, **{name: torch.zeros(4)})
    _raises(name, **{name: torch.ones(2, 3)})                                                # E = 4
    _raises(name, **{name: torch.ones(3, 4)})                                                # B = 2
    _raises(name, **{name: torch.full((2, 4), 0.5)})                                         # {0, 1} entries


def test_denoise_rejects_empty_router_row():
    noise, text = _cpu_args()
    s = EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4)
    with pytest.raises(ValueError, match="Vit_router_mask"):
        s.denoise(noise, torch.tensor(1.0), text, -1.2, 1.6, Vit_router_mask=torch.tensor([[1.0, 1, 0, 0], [0, 0, 0, 0]]))


# ----------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    hdmoe_hip.set_compute_dtype(torch.float32)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


def _masks(B, H, W, gen):
    binary = (torch.rand(B, 1, H, W, generator=gen, device=DEV) > 0.5).float()
    soft = torch.rand(B, 1, H, W, generator=gen, device=DEV)
    soft[0, 0, :2] = 1.0
    soft[1, 0, -2:] = 0.0
    bcast = torch.zeros(1, 1, H, W, device=DEV)
    bcast[..., : W // 2] = 1.0
    return {"none": None, "binary": binary, "soft": soft, "broadcast": bcast}


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("guide", [1.0, 2.5])
def test_trajectory_matches_restatement(_gpu, use_graph, guide):
    N, B = 6, 3
    gen = torch.Generator(device=DEV).manual_seed(1)
    noise = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(B, 5, 16, device=DEV, generator=gen)
    x0 = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    m, gnet = _MockDenoiser(0.9).to(DEV), _MockDenoiser(0.5).to(DEV)
    s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=guide, use_graph=use_graph)
    for mname, mask in _masks(B, 8, 8, gen).items():
        for strength in (1.0, 0.5, 1.0 / N):
            for init in ((None, x0) if strength == 1.0 and mask is None else (x0,)):
                n_run = math.ceil(strength * N)
                m.calls = gnet.calls = 0
                out = s.sample(noise, text, -1.2, 1.6, init_latents=init, strength=strength, inpaint_mask=mask)
                ref = restate(noise, N, guide, strength, init, mask)
                tag = f"mask={mname} strength={strength:.3f} init={init is not None} guide={guide} graph={use_graph}"
                close_scaled(out, ref.float(), 1e-4, msg=tag)
                if not use_graph:                         # replays do not call the modules
                    assert m.calls == 2 * n_run - 1, tag
                    assert gnet.calls == (0 if guide == 1.0 else 2 * n_run - 1), tag
    assert s.fused_heun


def _known_exact(out, x0, mask, msg):
    keep = mask.expand_as(out) == 1
    assert bool(keep.any()) and bool((~keep).any())
    assert torch.equal(out[keep], x0[keep]), f"{msg}: known region is not init_latents bit-for-bit"


@gpu
def test_known_region_exact_on_every_path(_gpu):
    N, B = 5, 2
    gen = torch.Generator(device=DEV).manual_seed(2)
    noise = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(B, 5, 16, device=DEV, generator=gen)
    x0 = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    mask = (torch.rand(B, 1, 8, 8, generator=gen, device=DEV) > 0.5).float()
    for use_graph in (False, True):
        s = EDM_Sampler(_MockDenoiser(0.9).to(DEV), _MockDenoiser(0.5).to(DEV), num_solve_steps=N, guidance=2.0, use_graph=use_graph)
        for strength in (1.0, 0.4):
            out = s.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=strength, inpaint_mask=mask)
            assert s.fused_heun
            _known_exact(out, x0, mask, f"fused graph={use_graph} strength={strength}")
    for use_graph in (False, True):                       # host-driven loop (churn), with and without the captured evaluation
        m = _MockDenoiser(0.9).to(DEV)
        s = EDM_Sampler(m, _MockDenoiser(0.5).to(DEV), num_solve_steps=N, S_churn=10.0, use_graph=use_graph)
        out = s.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=0.6, inpaint_mask=mask)
        assert not s.fused_heun and torch.isfinite(out).all()
        _known_exact(out, x0, mask, f"churn graph={use_graph}")
        if not use_graph:
            assert m.calls == 2 * math.ceil(0.6 * N) - 1


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_host_loop_matches_restatement(_gpu, use_graph):
    """The host-driven loop (host-scalar blend) on the same rules: S_churn > 0 selects it, S_max = 0 keeps every gamma at 0."""
    N, B = 5, 2
    gen = torch.Generator(device=DEV).manual_seed(3)
    noise = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(B, 5, 16, device=DEV, generator=gen)
    x0 = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    m, gnet = _MockDenoiser(0.9).to(DEV), _MockDenoiser(0.5).to(DEV)
    s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.5, S_churn=1.0, S_max=0.0, use_graph=use_graph)
    for mname, mask in _masks(B, 8, 8, gen).items():
        for strength in (1.0, 0.6):
            m.calls = 0
            out = s.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=strength, inpaint_mask=mask)
            assert not s.fused_heun
            close_scaled(out, restate(noise, N, 2.5, strength, x0, mask).float(), 1e-4, msg=f"host loop mask={mname} strength={strength}")
            if not use_graph:
                assert m.calls == 2 * math.ceil(strength * N) - 1


@gpu
def test_host_loop_bf16_known_region(_gpu):
    """bf16 latents take the host loop too: the known region is init_latents (in bf16) exactly."""
    gen = torch.Generator(device=DEV).manual_seed(7)
    noise = torch.randn(2, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(2, 5, 16, device=DEV, generator=gen)
    x0 = torch.randn(2, 4, 8, 8, device=DEV, generator=gen)
    mask = (torch.rand(2, 1, 8, 8, generator=gen, device=DEV) > 0.5).float()
    s = EDM_Sampler(_MockDenoiser(0.9).to(DEV), _MockDenoiser(0.5).to(DEV), num_solve_steps=4, dtype=torch.bfloat16)
    out = s.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=0.75, inpaint_mask=mask)
    assert not s.fused_heun and out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    _known_exact(out, x0.to(torch.bfloat16), mask, "bf16 host loop")


# ---- real model (config-2 golden weights)
@pytest.fixture(scope="module")
def real_model(_gpu):
    from models import model_config2
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    model = model_config2.preconditioned_HDMOEM(**g["cfg"])
    model.load_state_dict(g["state"])
    return model.to(DEV).eval(), g


@gpu
def test_real_model_inpaint_eager_vs_graph(real_model):
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(4)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    x0 = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    mask = torch.zeros(2, 1, 16, 16, device=DEV)
    mask[0, :, :, :8] = 1.0
    mask[1, :, 4:12, 4:12] = 1.0
    EDM_Sampler(model, model, num_solve_steps=2).sample(noise, text, -1.2, 1.6)       # registers the weight bank (see test_hip_parity)
    eager = EDM_Sampler(model, model, num_solve_steps=4).sample(noise, text, -1.2, 1.6, init_latents=x0, strength=0.5, inpaint_mask=mask)
    graphed = EDM_Sampler(model, model, num_solve_steps=4, use_graph=True).sample(noise, text, -1.2, 1.6, init_latents=x0, strength=0.5,
                                                                                  inpaint_mask=mask)
    assert torch.isfinite(eager).all()
    close_scaled(graphed, eager, 1e-5, msg="inpaint + strength 0.5: graph replay vs eager")
    _known_exact(eager, x0, mask, "eager")
    _known_exact(graphed, x0, mask, "graph")


@gpu
def test_real_model_one_capture_follows_every_conditioning(real_model):
    """Three sample() calls with different init_latents, masks and strengths through ONE graphed sampler each equal a fresh eager sampler:
    no static buffer and no capture is stale."""
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(5)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    cases = []
    for strength in (1.0, 0.5, 0.75):
        x0 = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
        mask = (torch.rand(2, 1, 16, 16, device=DEV, generator=gen) > 0.5).float()
        cases.append((x0, mask, strength))
    EDM_Sampler(model, model, num_solve_steps=2).sample(noise, text, -1.2, 1.6)
    graphed = EDM_Sampler(model, model, num_solve_steps=4, use_graph=True)
    outs = []
    for x0, mask, strength in cases:
        eager = EDM_Sampler(model, model, num_solve_steps=4).sample(noise, text, -1.2, 1.6, init_latents=x0, strength=strength,
                                                                    inpaint_mask=mask)
        out = graphed.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=strength, inpaint_mask=mask)
        close_scaled(out, eager, 1e-5, msg=f"strength {strength} through the shared capture")
        _known_exact(out, x0, mask, f"strength {strength}")
        outs.append(out)
    for a in range(3):
        for b in range(a + 1, 3):
            assert float((outs[a] - outs[b]).abs().max()) > 1e-3


@gpu
def test_router_mask_reaches_the_model(real_model):
    model, g = real_model
    B = 4
    x = g["x"][:B].to(DEV)
    sig = torch.tensor(1.7, device=DEV)
    text = g["text"][:B].to(DEV)
    s = EDM_Sampler(model, model, num_solve_steps=4)
    ones = torch.ones(B, model.num_experts, device=DEV)
    ref = model(x=x, sigma=sig, text_emb=text, Unet_router_mask=ones, Vit_router_mask=ones, zeta=0, transition_point=-1.2, softness=1.6)
    # keep for every sample only an expert the all-ones routing did not pick for sample 0
    used = set(torch.topk(ref["Unet_raw"][0], g["cfg"]["top_k"]).indices.tolist())
    e = next(k for k in range(model.num_experts) if k not in used)
    um = torch.zeros(B, model.num_experts, device=DEV)
    um[:, e] = 1.0
    out = s.denoise(x, sig, text, -1.2, 1.6, Unet_router_mask=um)
    direct = model(x=x, sigma=sig, text_emb=text, Unet_router_mask=um, Vit_router_mask=ones, zeta=0, transition_point=-1.2, softness=1.6)
    assert torch.equal(out, direct["denoised"]), "denoise() with a router mask differs from the direct model call"
    assert float((out - ref["denoised"]).abs().max()) > 1e-4, "excluding the experts the routing used changed nothing"
    assert torch.equal(s.denoise(x, sig, text, -1.2, 1.6), ref["denoised"])
    vm = torch.tensor([1.0, 0.0, 1.0, 0.0], device=DEV)                 # (E,) form
    direct = model(x=x, sigma=sig, text_emb=text, Unet_router_mask=ones, Vit_router_mask=vm.expand(B, -1).contiguous(), zeta=0,
                   transition_point=-1.2, softness=1.6)
    assert torch.equal(s.denoise(x, sig, text, -1.2, 1.6, Vit_router_mask=vm), direct["denoised"])


@gpu
def test_router_mask_sampling_eager_vs_graph(real_model):
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(6)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    um = torch.tensor([0.0, 0.0, 1.0, 0.0], device=DEV)                 # one U-Net expert
    EDM_Sampler(model, model, num_solve_steps=2).sample(noise, text, -1.2, 1.6)
    eager = EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0).sample(noise, text, -1.2, 1.6, Unet_router_mask=um)
    graphed = EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0, use_graph=True)
    out = graphed.sample(noise, text, -1.2, 1.6, Unet_router_mask=um)
    assert torch.isfinite(eager).all()
    close_scaled(out, eager, 1e-5, msg="one-expert U-Net mask: graph replay vs eager")
    plain = EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0).sample(noise, text, -1.2, 1.6)
    assert float((plain - eager).abs().max()) > 1e-4
    # the mock sees the mask on both networks, on the fused and on the churn path
    for churn in (0.0, 5.0):
        m, gn = _MockDenoiser(0.9).to(DEV), _MockDenoiser(0.5).to(DEV)
        EDM_Sampler(m, gn, num_solve_steps=3, guidance=2.0, S_churn=churn).sample(noise, text, -1.2, 1.6, Unet_router_mask=um)
        for net in (m, gn):
            assert net.masks and all(torch.equal(u, um.expand(2, -1)) and bool((v == 1).all()) for u, v in net.masks)


@gpu
@pytest.mark.parametrize("solver,churn", [("heun", 0.0), ("dpmpp_2m", 0.0), ("heun", 1.0)], ids=["heun", "dpmpp_2m", "churn_eval"])
def test_capture_follows_guide_and_model(_gpu, solver, churn):
    """A captured sampler recaptures when guide or the model changes between sample() calls: each output equals a fresh eager sampler's.
    churn_eval: S_churn > 0 with S_max = 0 takes the host loop through the captured evaluation, without noise."""
    gen = torch.Generator(device=DEV).manual_seed(8)
    noise = torch.randn(2, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(2, 5, 16, device=DEV, generator=gen)
    gnet = _MockDenoiser(0.5).to(DEV)
    kw = dict(num_solve_steps=4, S_churn=churn, S_max=0.0, solver=solver)
    graphed = EDM_Sampler(_MockDenoiser(0.9).to(DEV), gnet, use_graph=True, **kw)

    def check(tag):
        out = graphed.sample(noise, text, -1.2, 1.6)
        eager = EDM_Sampler(graphed.model, gnet, guidance=graphed.guide, **kw).sample(noise, text, -1.2, 1.6)
        assert (graphed.fused_heun or graphed.fused_dpm) == (churn == 0.0), tag
        assert torch.equal(out, eager), f"{tag}: the replay differs from eager sampling"

    check("first capture")
    for guide in (2.5, 1.0):
        graphed.guide = guide
        check(f"guide {guide}")
    graphed.model = _MockDenoiser(0.7).to(DEV)
    check("new model")
