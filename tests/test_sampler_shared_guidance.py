"""Classifier-free guidance in one shared-routing evaluation: EDM_Sampler(shared_guidance=True) / preconditioned_HDMOEM.forward_guided.

Layout: "pair-stacked" = [conditional rows 0..B-1 ; unconditional rows B..2B-1].

CPU tests: the argument checks.  GPU tests: hdmoe_gather_rows_paired against src[perm % B]; hdmoe_nhwc_to_nchw_guided against float64;
one guided evaluation against the CPU oracle (two evaluations + cfg_lerp) on both model variants; a short trajectory against the oracle's;
eager against hipGraph replay; launch counts of one evaluation; a mock model's call pattern; uncond_text_emb=None.

Tolerances.  close_scaled is the sampler tests' form, max|a - b| <= rel * max|b| + 1e-6.
  guided egress: per element 4 eps_fp32 (|sx x| + |sf| (|1-g| |F_u| + |g| |F_c|)) -- three multiply-adds in fp32, bf16 F converts exactly;
  one evaluation: (|g| + |1 - g|) times the single-evaluation bounds of tests/test_hip_parity.py (1e-3 fp32, 2e-2 bf16 compute mode): the
      factor is how far the lerp can amplify the per-pass error;
  trajectory: 4 x the measured error of the two-pass path against the same oracle trajectory (TWO_PASS_ERR below);
  eager vs replay 1e-5, mock trajectory vs its float64 restatement 1e-4: the existing sampler tests' bounds."""
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
EPS32 = 2.0 ** -23
TP, SOFT = -1.2, 1.6


class _MockDenoiser(torch.nn.Module):
    """Closed-form mock D(x; text) = scale x + 0.3 mean(text), with the shared pass forward_guided = (1 - g) D(x; unc) + g D(x; text)
    + guided_bias (a marker that tells the two modes apart where a test needs it).  Counts and records its calls."""

    def __init__(self, scale, num_experts=4, guided_bias=0.0):
        super().__init__()
        self.num_experts = num_experts
        self.scale = scale
        self.guided_bias = guided_bias
        self.calls = 0
        self.guided = []                                  # (guidance, a copy of uncond_text_emb or None) per forward_guided call

    def _d(self, x, text):
        return x * self.scale + 0.3 * text.float().mean(dim=(1, 2)).view(-1, 1, 1, 1)

    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, transition_point, softness, return_log_var=False):
        self.calls += 1
        return {"denoised": self._d(x, text_emb)}

    def forward_guided(self, x, sigma, text_emb, uncond_text_emb, guidance, Unet_router_mask, Vit_router_mask, zeta, transition_point,
                       softness):
        assert sigma.ndim == 0 and Unet_router_mask.shape == (x.shape[0], self.num_experts) and zeta == 0
        self.guided.append((guidance, None if uncond_text_emb is None else uncond_text_emb.clone()))
        if uncond_text_emb is None:
            return {"denoised": self._d(x, text_emb)}
        return {"denoised": (1.0 - guidance) * self._d(x, uncond_text_emb) + guidance * self._d(x, text_emb) + self.guided_bias}


class _PlainMock(torch.nn.Module):
    """A model without forward_guided."""
    num_experts = 4

    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, transition_point, softness, return_log_var=False):
        return {"denoised": x * 0.9}


def close_scaled(a, b, rel, msg="", atol=1e-6):
    """max|a-b| <= rel * max|b| + atol (the sampler tests' tolerance form)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{msg}: non-finite output"
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print(f"{msg}: max err {err:.3e}, bound {rel * scale + atol:.3e}")
    assert err <= rel * scale + atol, f"{msg}: max err {err:.3e} > {rel:.1e} * {scale:.3e} + {atol:.0e}"


def close_logits(a, b, rel, msg=""):
    """close_scaled for router logits: masked experts hold -inf, which must coincide; the finite entries within the bound."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin) and torch.equal(a[~fin], b[~fin]), f"{msg}: masked entries differ"
    close_scaled(a[fin], b[fin], rel, msg=msg)


def schedule(N, sigma_min=0.002, sigma_max=80.0, rho=7):
    i = torch.arange(N, dtype=torch.float64)
    t = (sigma_max ** (1 / rho) + i / (N - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros(1, dtype=torch.float64)])


def dpm_update(t, i, i0, x, d, dp):
    """The DPM-Solver++(2M) update of stage i (tests/test_sampler_dpm_solver.py), in the dtype of its operands."""
    a = t[i + 1] / t[i]
    if t[i + 1] == 0:
        return d.clone()
    if i == i0:
        return a * x + (1 - a) * d
    r = torch.log(t[i - 1] / t[i]) / torch.log(t[i] / t[i + 1])
    return a * x + (1 - a) * ((1 + 1 / (2 * r)) * d - (1 / (2 * r)) * dp)


def restate64(solver, den, noise, N):
    """float64 restatement of sample() without churn / conditioning: den(x) -> the guided D in float64."""
    t = schedule(N)
    x = t[0] * noise.cpu().double()
    dp = None
    for i in range(N):
        d = den(x, t[i])
        if solver == "heun":
            h = t[i + 1] - t[i]
            xn = x + h * (x - d) / t[i]
            x = xn if i == N - 1 else x + h * (0.5 * (x - d) / t[i] + 0.5 * (xn - den(xn, t[i + 1])) / t[i + 1])
        else:
            x = dpm_update(t, i, 0, x, d, dp)
            dp = d
    return x


# ----------------------------------------------------------------------------------------------- 1. argument checks (CPU)
def test_shared_guidance_needs_the_model_as_guide():
    m = _MockDenoiser(0.9)
    with pytest.raises(ValueError, match="shared_guidance"):
        EDM_Sampler(m, _MockDenoiser(0.5), num_solve_steps=4, guidance=2.0, shared_guidance=True)
    s = EDM_Sampler(m, m, num_solve_steps=4, guidance=2.0, shared_guidance=True)
    assert s.shared_guidance is True and s._stage is None and s._graph is None
    assert EDM_Sampler(m, _MockDenoiser(0.5), num_solve_steps=4).shared_guidance is False       # the default takes any guide network


def test_shared_guidance_needs_forward_guided():
    m = _PlainMock()
    with pytest.raises(ValueError, match="shared_guidance"):
        EDM_Sampler(m, m, num_solve_steps=4, guidance=2.0, shared_guidance=True)
    EDM_Sampler(m, m, num_solve_steps=4, guidance=2.0)


def test_uncond_of_another_shape_raises(golden_full):
    """CPU tensors: any device work would raise RuntimeError (no CPU fallback) instead of the ValueError."""
    from models import model_config1, model_config2
    g = golden_full
    cls = (model_config1 if g["variant"] == 1 else model_config2).preconditioned_HDMOEM
    model = cls(**g["cfg"]).eval()
    B = 2
    kw = dict(x=g["x"][:B], sigma=g["sigma"][:B], text_emb=g["text"][:B], guidance=2.5, Unet_router_mask=g["unet_mask"][:B],
              Vit_router_mask=g["vit_mask"][:B], zeta=0.0, **g["extra"])
    with torch.no_grad():
        for bad in (g["text"][:B, :-1], g["text"][:1], g["text"][:B, 0]):
            with pytest.raises(ValueError, match="uncond_text_emb"):
                model.forward_guided(uncond_text_emb=bad, **kw)
    with pytest.raises(RuntimeError, match="inference only"):                                   # grad mode on, parameters require grad
        model.forward_guided(uncond_text_emb=g["text"][:B].flip(0), **kw)
    if g["variant"] == 2:                                 # through the sampler (its model call carries transition_point / softness)
        s = EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0, shared_guidance=True)
        with torch.no_grad(), pytest.raises(ValueError, match="uncond_text_emb"):
            s.denoise(g["x"][:B], torch.tensor(1.0), g["text"][:B], TP, SOFT, uncond_text_emb=g["text"][:1])


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


# ---- 2. paired gather
@gpu
def test_paired_gather_matches_indexing(_gpu):
    """hdmoe_gather_rows_paired against src[perm % B], exactly: 16-byte and scalar paths in both dtypes, unused rows (a sample routed to
    fewer than k experts) zero as in gather_rows, one expert without rows.  And the property the shared pass relies on: the plan of
    [w ; w] keeps, inside each expert's segment, the conditional rows first and the same samples' unconditional rows behind them."""
    from hdmoe_hip import ops
    B, E, k = 5, 4, 2
    w = torch.zeros(B, E, device=DEV)
    for b, (e0, e1) in enumerate([(0, 1), (2, 0), (1, 2), (0, 2), (1, 0)]):                     # expert 3 gets no row
        w[b, e0], w[b, e1] = 0.6, 0.4
    w[1] = 0.0
    w[1, 2] = 1.0                                                                               # one sample on a single expert
    plan1 = ops.DispatchPlan(w, k)
    plan = ops.DispatchPlan(torch.cat([w, w]), k)
    perm, seg = plan.perm.cpu().long(), plan.seg.cpu()
    assert torch.equal(seg, 2 * plan1.seg.cpu()) and int(seg[4] - seg[3]) == 0
    assert int((perm < 0).sum()) == 2 and plan.R == 2 * B * k                                  # the unused rows of sample 1, twice
    p1 = plan1.perm.cpu().long()
    for e in range(E):
        a, b, n = int(seg[e]), int(seg[e + 1]), int(plan1.seg[e + 1] - plan1.seg[e])
        own = p1[int(plan1.seg[e]):int(plan1.seg[e + 1])]
        assert torch.equal(perm[a:a + n], own) and torch.equal(perm[a + n:b], own + B), f"expert {e}: segment is not [cond ; uncond]"
    gen = torch.Generator(device=DEV).manual_seed(3)
    for dtype, shape in ((torch.float32, (3, 8)), (torch.float32, (7,)), (torch.bfloat16, (2, 8)), (torch.bfloat16, (5,)),
                         (torch.bfloat16, (3, 4, 6))):
        src = torch.randn(B, *shape, device=DEV, generator=gen).to(dtype)
        L = src[0].numel()
        vec = (L * src.element_size()) % 16 == 0
        out = ops.gather_rows_paired(src, plan, B)
        ref = src[(perm % B).to(DEV)].clone()
        ref[(perm < 0).to(DEV)] = 0
        assert out.shape == (plan.R, *shape) and out.dtype == dtype
        assert torch.equal(out, ref), f"{dtype} L={L} ({'16-byte' if vec else 'scalar'} path)"
        # the same rows as the plain gather of the materialised stack
        assert torch.equal(out, ops.gather_rows(torch.cat([src, src]), plan))
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("hdmoe_gather_rows_paired", out, src, plan.perm, plan.R, L, 0, 1)
    with pytest.raises(ValueError, match="gather_rows_paired"):
        ops.gather_rows_paired(src[:3], plan, 3)                                                # 10 plan rows are no stack of 3
    torch.cuda.synchronize()


# ---- 3. guided egress
@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("guide", [0.0, 1.0, 2.5, -0.5])
def test_guided_egress_matches_float64(_gpu, dtype, guide):
    """out[n] = sx[n] x[n] + sf[n] ((1 - g) F[N + n] + g F[n]) against float64, per element within
    4 eps_fp32 (|sx x| + |sf| (|1-g| |F_u| + |g| |F_c|)).  HW = 63 and C = 5 are multiples of nothing the launch uses (256-thread blocks).
    g = 1 against hdmoe_nhwc_to_nchw on the conditional half: asserted within the same bound; the kernel is written to reduce to that
    kernel's operations at g = 1 (the lerp then returns F_c exactly), the equality is printed but whether the compiler contracts the two
    kernels' multiply-adds alike is its choice, so the bound is what is pinned."""
    from hdmoe_hip import ops
    gen = torch.Generator(device=DEV).manual_seed(5)
    N, C, H, W = 3, 5, 7, 9
    F = (3.0 * torch.randn(2 * N, H, W, C, device=DEV, generator=gen)).to(dtype)
    x = torch.randn(N, C, H, W, device=DEV, generator=gen)
    sf = torch.rand(N, device=DEV, generator=gen) + 0.1
    sx = torch.rand(N, device=DEV, generator=gen) - 0.5
    out = ops.nhwc_to_nchw_guided(F, sf, x, sx, guide)
    assert out.shape == (N, C, H, W) and out.dtype == torch.float32
    F64 = F.double().permute(0, 3, 1, 2).cpu()
    fc, fu = F64[:N], F64[N:]
    sf64, sx64, x64 = sf.double().cpu().view(-1, 1, 1, 1), sx.double().cpu().view(-1, 1, 1, 1), x.double().cpu()
    ref = sx64 * x64 + sf64 * ((1.0 - guide) * fu + guide * fc)
    bound = 4 * EPS32 * ((sx64 * x64).abs() + sf64.abs() * (abs(1.0 - guide) * fu.abs() + abs(guide) * fc.abs()))
    err = (out.double().cpu() - ref).abs()
    print(f"guided egress g={guide} {dtype}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"g={guide} {dtype}: max err / bound = {float((err / bound).max()):.3f}"
    if guide == 1.0:
        plain = ops.nhwc_to_nchw_f32(F[:N].contiguous(), sf, x, sx)
        print(f"g = 1 equals hdmoe_nhwc_to_nchw bit-for-bit: {torch.equal(out, plain)}")
        assert bool(((out.double().cpu() - plain.double().cpu()).abs() <= bound).all())
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("hdmoe_nhwc_to_nchw_guided", out, F, sf, x, sx, float("nan"), N, C, H * W, 0 if dtype == torch.float32 else 1)
    with pytest.raises(ValueError, match="pair-stacked"):
        ops.nhwc_to_nchw_guided(F[:5], sf, x, sx, guide)
    torch.cuda.synchronize()


# ---- 4. one evaluation against the reference, both variants
def _load(g):
    from models import model_config1, model_config2
    cls = (model_config1 if g["variant"] == 1 else model_config2).preconditioned_HDMOEM
    model = cls(**g["cfg"])
    model.load_state_dict(g["state"])
    return model.to(DEV).eval()


@gpu
@pytest.mark.parametrize("mode,unc_kind", [("fp32", "flip"), ("bf16", "flip"), ("fp32", "zeros")])
def test_one_guided_evaluation_matches_oracle(_gpu, golden_full, mode, unc_kind):
    import hdmoe_hip
    from oracle import hdmoe_oracle as O
    g = golden_full
    guide = 2.5
    unc = g["text"].flip(0) if unc_kind == "flip" else torch.zeros_like(g["text"])
    with torch.no_grad():
        ref_c, ref_u = (O.preconditioned_hdmoem(g["state"], g["cfg"], g["variant"], g["x"], g["sigma"], t, g["unet_mask"], g["vit_mask"],
                                                **g["extra"])["denoised"] for t in (g["text"], unc))
    ref = O.cfg_lerp(ref_c, ref_u, guide)
    assert float((ref_c - ref_u).abs().max()) > 1e-3 * float(ref_c.abs().max())                 # the unconditional branch matters here
    hdmoe_hip.set_compute_dtype(torch.float32 if mode == "fp32" else torch.bfloat16)
    try:
        model = _load(g)
        with torch.no_grad():
            out = model.forward_guided(x=g["x"].to(DEV), sigma=g["sigma"].to(DEV), text_emb=g["text"].to(DEV),
                                       uncond_text_emb=unc.to(DEV), guidance=guide, Unet_router_mask=g["unet_mask"].to(DEV),
                                       Vit_router_mask=g["vit_mask"].to(DEV), zeta=0.0, **g["extra"])
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)
    k = g["cfg"]["top_k"]
    B = g["x"].shape[0]
    for key in ("Unet_raw", "vit_raw"):                   # the shared routing: per sample (B rows), indices bit-exact vs the reference
        assert out[key].shape[0] == B
        assert torch.equal(torch.topk(out[key].cpu(), k, dim=-1).indices, g["topk_idx"][key]), key
        close_logits(out[key], g["out"][key], 1e-3, msg=key)
    for key in ("Unet_router_loss", "vit_router_loss", "scaling_net_out"):
        close_scaled(out[key], g["out"][key], 1e-3, msg=key)
    assert out["denoised"].shape == g["x"].shape
    rel = (abs(guide) + abs(1.0 - guide)) * (1e-3 if mode == "fp32" else 2e-2)
    close_scaled(out["denoised"], ref, rel, msg=f"guided denoised, variant {g['variant']} {mode} unc={unc_kind}")


# ---- real model (config-2 golden weights) for the sampler tests
@pytest.fixture(scope="module")
def real_model(_gpu):
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    model = _load(g)
    gen = torch.Generator(device=DEV).manual_seed(0)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    EDM_Sampler(model, model, num_solve_steps=2).sample(noise, g["text"][:2].to(DEV), TP, SOFT)     # registers the weight bank
    return model, g


# ---- 5. shared against two-pass on a short trajectory
# Measured on an MI355X: max|two-pass - oracle trajectory| / max|oracle trajectory| of the EXISTING two-pass path for the inputs below
# (fp32 compute mode, B = 2, N = 4, g = 2.0, TRAJ_SEED).  The shared path is allowed 4x it: the same kernels' rounding, but possibly other
# kernel selections at 2B rows, over up to seven chained evaluations.
TWO_PASS_ERR = {"heun": 2.808e-06, "dpmpp_2m": 2.627e-06}       # (the shared path measured 2.553e-06 / 2.249e-06 in the same run)
TRAJ_SEED = 0


def trajectory_case(model, g, solver, seed, N=4, B=2, guide=2.0):
    """Oracle trajectory (CPU) with the oracle's guided denoiser, the two-pass and the shared GPU trajectories, and whether the GPU model
    reproduces the oracle's top-k on every state the oracle evaluates."""
    from oracle import hdmoe_oracle as O
    gen = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, 4, 16, 16, generator=gen)
    text = g["text"][:B]
    unc = torch.randn(text.shape, generator=gen)
    E, k = g["cfg"]["num_experts"], g["cfg"]["top_k"]
    ones = torch.ones(B, E)
    seen = []

    def oracle_den(x, t):
        with torch.no_grad():
            outs = [O.preconditioned_hdmoem(g["state"], g["cfg"], 2, x.float(), t.float(), tx, ones, ones, transition_point=TP, softness=SOFT)
                    for tx in (text, unc)]
        seen.append((x.float(), t.float(), [torch.topk(outs[0][key], k, dim=-1) for key in ("Unet_raw", "vit_raw")]))
        return O.cfg_lerp(outs[0]["denoised"], outs[1]["denoised"], guide).to(x.dtype)

    if solver == "heun":
        ref = O.edm_sampler(oracle_den, noise, N)
    else:
        ref = restate64(solver, oracle_den, noise, N)
    ties_free, margin = True, float("inf")
    with torch.no_grad():
        for x, t, tops in seen:
            out = model(x=x.to(DEV), sigma=t.to(DEV), text_emb=text.to(DEV), Unet_router_mask=ones.to(DEV), Vit_router_mask=ones.to(DEV),
                        zeta=0, transition_point=TP, softness=SOFT)
            for key, top in zip(("Unet_raw", "vit_raw"), tops):
                ties_free &= torch.equal(torch.topk(out[key].cpu(), k, dim=-1).indices, top.indices)
    outs = {}
    for name, shared in (("two_pass", False), ("shared", True)):
        s = EDM_Sampler(model, model, num_solve_steps=N, guidance=guide, solver=solver, shared_guidance=shared)
        outs[name] = s.sample(noise.to(DEV), text.to(DEV), TP, SOFT, unc.to(DEV)).cpu()
    scale = float(ref.abs().max())
    err = {name: float((o.double() - ref.double()).abs().max()) / scale for name, o in outs.items()}
    return dict(ref=ref, outs=outs, err=err, routing_exact=ties_free, evaluations=len(seen))


@gpu
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_shared_trajectory_against_oracle(real_model, solver):
    model, g = real_model
    c = trajectory_case(model, g, solver, TRAJ_SEED)
    print(f"{solver}: two-pass err {c['err']['two_pass']:.3e}, shared err {c['err']['shared']:.3e} (relative to max|oracle trajectory|), "
          f"{c['evaluations']} oracle evaluations, routing exact: {c['routing_exact']}")
    assert c["evaluations"] == (7 if solver == "heun" else 4)
    assert c["routing_exact"], "the GPU routing differs from the oracle's on this seed (a near-tie): pick another TRAJ_SEED"
    assert torch.isfinite(c["outs"]["shared"]).all()
    assert c["err"]["shared"] <= 4 * TWO_PASS_ERR[solver], f"{solver}: shared err {c['err']['shared']:.3e} > 4 x {TWO_PASS_ERR[solver]:.3e}"


# ---- 6. eager = graph
def _known_exact(out, x0, mask, msg):
    keep = mask.expand_as(out) == 1
    assert bool(keep.any()) and bool((~keep).any())
    assert torch.equal(out[keep], x0[keep]), f"{msg}: known region is not init_latents bit-for-bit"


GRAPH_CASES = {
    "heun": dict(),
    "dpmpp_2m": dict(solver="dpmpp_2m"),
    "dpmpp_2m_sde": dict(solver="dpmpp_2m_sde", eta=0.5),
    "churn_on_device": dict(S_churn=3.0, S_min=0.05, S_max=50.0, churn_on_device=True),
    "conditioned": dict(),
}


@gpu
@pytest.mark.parametrize("case", list(GRAPH_CASES))
def test_shared_eager_vs_graph(real_model, case):
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(11)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    x0 = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    unc = torch.randn(text.shape, device=DEV, generator=gen)
    kw = dict(seed=12345) if case in ("dpmpp_2m_sde", "churn_on_device") else {}
    mask = None
    if case == "conditioned":
        mask = torch.zeros(2, 1, 16, 16, device=DEV)
        mask[0, :, :, :8] = 1.0
        mask[1, :, 4:12, 4:12] = 1.0
        kw = dict(init_latents=x0, strength=0.75, inpaint_mask=mask, Unet_router_mask=torch.tensor([1.0, 0.0, 1.0, 1.0], device=DEV))
    mk = lambda **o: EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0, shared_guidance=True, **GRAPH_CASES[case], **o)  # noqa: E731
    eager_s, graph_s = mk(), mk(use_graph=True)
    eager = eager_s.sample(noise, text, TP, SOFT, unc, **kw)
    graphed = graph_s.sample(noise, text, TP, SOFT, unc, **kw)
    assert torch.isfinite(eager).all()
    assert (graph_s.fused_heun or graph_s.fused_dpm) and graph_s._stage is not None
    close_scaled(graphed, eager, 1e-5, msg=f"{case}: graph replay vs eager")
    if mask is not None:
        _known_exact(eager, x0, mask, "eager")
        _known_exact(graphed, x0, mask, "replay")
    plain = EDM_Sampler(model, model, num_solve_steps=4, guidance=1.0, **GRAPH_CASES[case]).sample(noise, text, TP, SOFT, unc, **kw)
    assert float((plain - eager).abs().max()) > 1e-4                      # the guidance is in effect
    # another prompt and another unconditional embedding through the SAME capture: no stale buffer
    stage = graph_s._stage
    text2, unc2 = g["text"][2:4].to(DEV), torch.randn(text.shape, device=DEV, generator=gen)
    again = graph_s.sample(noise, text2, TP, SOFT, unc2, **kw)
    assert graph_s._stage is stage, "same shapes must not recapture"
    close_scaled(again, mk().sample(noise, text2, TP, SOFT, unc2, **kw), 1e-5, msg=f"{case}: second prompt through the same capture")
    assert float((again - graphed).abs().max()) > 1e-4


@gpu
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_capture_follows_shared_guidance(_gpu, solver):
    """Flipping shared_guidance on a live captured sampler recaptures (the key test of test_capture_follows_guide_and_model for the new
    key member).  The mock's shared pass carries a marker bias, so a stale capture of the other mode shows in the output."""
    gen = torch.Generator(device=DEV).manual_seed(8)
    noise = torch.randn(2, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(2, 5, 16, device=DEV, generator=gen)
    unc = torch.randn(2, 5, 16, device=DEV, generator=gen)
    m = _MockDenoiser(0.9, guided_bias=0.25).to(DEV)
    kw = dict(num_solve_steps=4, guidance=2.0, solver=solver)
    graphed = EDM_Sampler(m, m, use_graph=True, **kw)
    outs = {}
    for shared in (False, True, False):
        graphed.shared_guidance = shared
        before = graphed._stage
        out = graphed.sample(noise, text, TP, SOFT, unc)
        assert graphed._stage is not before, f"shared_guidance={shared}: no recapture"
        assert graphed._stage["key"][-1] is shared
        eager = EDM_Sampler(m, m, shared_guidance=shared, **kw).sample(noise, text, TP, SOFT, unc)
        assert torch.equal(out, eager), f"shared_guidance={shared}: the replay differs from eager sampling"
        outs[shared] = out
    assert float((outs[True] - outs[False]).abs().max()) > 1e-2            # the marker: the two modes ran different code


# ---- 7. it really is one pass
@gpu
def test_launch_counts_of_one_guided_evaluation(real_model):
    """Routers and plans once instead of twice, one guided egress, no blend.  The blend is an hdmoe_axpby call behind the two evaluations;
    the model itself goes through hdmoe_axpby as well (its mp_sum is that entry point), so "no blend" is pinned as: a shared evaluation
    makes exactly the hdmoe_axpby calls of ONE plain evaluation, the two-pass one twice as many plus the blend, and the guided egress is
    the last call of a shared evaluation (the blend would follow it)."""
    from hdmoe_hip import _lib
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    unc = torch.randn(text.shape, device=DEV, generator=gen)
    sig = torch.tensor(1.3, device=DEV)
    counts = {}
    for shared in (True, False, None):                   # None: one plain evaluation (guidance 1)
        s = EDM_Sampler(model, model, num_solve_steps=4, guidance=1.0 if shared is None else 2.0, shared_guidance=bool(shared))
        with torch.no_grad():
            s.denoise(x, sig, text, TP, SOFT, unc)                          # warm: nothing one-off in the log
            _lib.CALL_LOG = []
            try:
                out = s.denoise(x, sig, text, TP, SOFT, unc)
                log = [name for name, _ in _lib.CALL_LOG]
            finally:
                _lib.CALL_LOG = None
        counts[shared] = {n: log.count(n) for n in ("hdmoe_router_head_fwd", "hdmoe_dispatch_plan", "hdmoe_nhwc_to_nchw_guided",
                                                     "hdmoe_nhwc_to_nchw", "hdmoe_axpby", "hdmoe_gather_rows_paired")}
        counts[shared]["total"] = len(log)
        counts[shared]["last"] = log[-1]
        counts[shared]["out"] = out
    print({k: {n: v for n, v in c.items() if n != "out"} for k, c in counts.items()})
    sh, tp, one = counts[True], counts[False], counts[None]
    assert sh["hdmoe_router_head_fwd"] == 2 and tp["hdmoe_router_head_fwd"] == 4
    assert sh["hdmoe_dispatch_plan"] == 2 and tp["hdmoe_dispatch_plan"] == 4
    assert sh["hdmoe_nhwc_to_nchw_guided"] == 1 and sh["hdmoe_nhwc_to_nchw"] == 0 and sh["last"] == "hdmoe_nhwc_to_nchw_guided"
    assert sh["hdmoe_axpby"] == one["hdmoe_axpby"] and tp["hdmoe_axpby"] == 2 * one["hdmoe_axpby"] + 1 and tp["last"] == "hdmoe_axpby"
    assert tp["hdmoe_nhwc_to_nchw_guided"] == 0 and tp["hdmoe_nhwc_to_nchw"] == 2
    assert sh["hdmoe_gather_rows_paired"] == 4                              # features and time embedding, for each bank
    assert sh["total"] < tp["total"]
    # both modes are within (|g| + |1 - g|) 1e-3 of the same exact value (the one-evaluation bound above): twice that between them
    close_scaled(sh["out"], tp["out"], 2 * 3 * 1e-3, msg="one evaluation: shared vs two-pass")


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_mock_sees_one_guided_call_per_evaluation(_gpu, solver, use_graph):
    N, B, guide = 5, 3, 2.5
    gen = torch.Generator(device=DEV).manual_seed(1)
    noise = torch.randn(B, 4, 8, 8, device=DEV, generator=gen)
    text = torch.randn(B, 5, 16, device=DEV, generator=gen)
    unc = torch.randn(B, 5, 16, device=DEV, generator=gen)
    m = _MockDenoiser(0.9).to(DEV)
    s = EDM_Sampler(m, m, num_solve_steps=N, guidance=guide, solver=solver, use_graph=use_graph, shared_guidance=True)
    out = s.sample(noise, text, TP, SOFT, unc)
    t64, u64 = text.cpu().double(), unc.cpu().double()
    d64 = lambda x, tx: 0.9 * x + 0.3 * tx.mean(dim=(1, 2)).view(-1, 1, 1, 1)         # noqa: E731
    ref = restate64(solver, lambda x, t: (1.0 - guide) * d64(x, u64) + guide * d64(x, t64), noise, N)
    close_scaled(out, ref.float(), 1e-4, msg=f"{solver} graph={use_graph}: shared mode vs the float64 restatement")
    assert m.calls == 0, "shared mode must not call forward()"
    if not use_graph:                                     # replays do not call the module
        assert len(m.guided) == (2 * N - 1 if solver == "heun" else N)
    assert m.guided and all(gd == guide and torch.equal(u, unc) for gd, u in m.guided)
    # guidance 1: the single plain evaluation, no guided call
    m.guided.clear()
    EDM_Sampler(m, m, num_solve_steps=N, guidance=1.0, solver=solver, shared_guidance=True).sample(noise, text, TP, SOFT, unc)
    assert not m.guided and m.calls == (2 * N - 1 if solver == "heun" else N)


# ---- 8. uncond_text_emb=None
@gpu
def test_no_uncond_embedding_is_the_plain_evaluation(real_model):
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(14)
    x = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    sig = torch.tensor(0.7, device=DEV)
    with torch.no_grad():
        shared = EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0, shared_guidance=True).denoise(x, sig, text, TP, SOFT)
        plain = EDM_Sampler(model, model, num_solve_steps=4, guidance=1.0).denoise(x, sig, text, TP, SOFT)
    assert torch.equal(shared, plain)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    a = EDM_Sampler(model, model, num_solve_steps=3, guidance=2.0, shared_guidance=True).sample(noise, text, TP, SOFT)
    b = EDM_Sampler(model, model, num_solve_steps=3, guidance=1.0).sample(noise, text, TP, SOFT)
    assert torch.equal(a, b)
