"""Guidance interval and per-sample guidance scales: EDM_Sampler(guidance_interval=(lo, hi)), sample(guidance=vector) / denoise(guidance=vector,
guided=...), forward_guided with a (B,) scale, and the two kernels behind them (hdmoe_nhwc_to_nchw_guided_rows, hdmoe_lerp_rows).

CPU tests: the argument checks and the host-side plan (guidance_plan) on the Karras schedules
  N = 5: t = [80, 17.528, 2.5152, 0.1698, 0.002, 0],   N = 6: t = [80, 24.408, 5.8389, 0.9654, 0.0851, 0.002, 0].
GPU tests: the kernels against float64 and, for a constant vector, bit for bit against the scalar entry points; the sampler on a closed-form
mock (interval runs against a float64 restatement, replay against eager, no recapture, per-sample vectors); the real model (bit-exact ends,
one evaluation per row, a trajectory against the CPU oracle, the launch log of an unguided evaluation).

Tolerances.  close_scaled is the sampler tests' form, max|a - b| <= rel * max|b| + 1e-6.
  per-row egress: per element 4 eps_fp32 (|sx x| + |sf| (|1-g| |F_u| + |g| |F_c|)), the bound of the scalar egress test;
  lerp_rows: per element 4 eps_fp32 (|1-g| |ref| + |g| |d|) -- the rounding of 1 - g, two multiply-adds -- and in bf16 one rounding of the
      output more: bf16 keeps 8 significant bits, so half an ulp is at most 2^-8 of the magnitude the fp32 value can have;
  mock trajectory vs its float64 restatement 1e-4, the existing sampler tests' bound; replay vs eager on the mock: torch.equal;
  real-model trajectory: 4 x the measured error of the always-guided two-pass path of the parent commit at N = 5 (TWO_PASS_ERR_N5)."""
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
INF = float("inf")


class _MockDenoiser(torch.nn.Module):
    """Closed-form mock D(x; text) = scale x + 0.3 mean(text), with the shared pass forward_guided = (1 - g) D(x; unc) + g D(x; text)
    + guided_bias (a marker that tells the two modes apart where a test needs it).  Counts and records its calls.  (The mock of
    tests/test_sampler_shared_guidance.py; a (B,) guidance tensor is applied per row.)"""

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
        if isinstance(guidance, torch.Tensor):
            assert guidance.shape == (x.shape[0],) and guidance.dtype == torch.float32 and guidance.device == x.device
            guidance = guidance.view(-1, 1, 1, 1)
        return {"denoised": (1.0 - guidance) * self._d(x, uncond_text_emb) + guidance * self._d(x, text_emb) + self.guided_bias}


class _RaisingMock(_MockDenoiser):
    """Any model call is a failure of "before any device work"."""

    def forward(self, *a, **k):
        raise RuntimeError("the model was called")

    forward_guided = forward


def close_scaled(a, b, rel, msg="", atol=1e-6):
    """max|a-b| <= rel * max|b| + atol (the sampler tests' tolerance form)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{msg}: non-finite output"
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print(f"{msg}: max err {err:.3e}, bound {rel * scale + atol:.3e}")
    assert err <= rel * scale + atol, f"{msg}: max err {err:.3e} > {rel:.1e} * {scale:.3e} + {atol:.0e}"


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


def restate64(solver, den, noise, N, i0=0, x_start=None):
    """float64 restatement of sample() without churn: den(x, t) -> the denoiser output in float64, gated by the caller on t."""
    t = schedule(N)
    x = t[i0] * noise.cpu().double() if x_start is None else x_start
    dp = None
    for i in range(i0, N):
        d = den(x, t[i])
        if solver == "heun":
            h = t[i + 1] - t[i]
            xn = x + h * (x - d) / t[i]
            x = xn if i == N - 1 else x + h * (0.5 * (x - d) / t[i] + 0.5 * (xn - den(xn, t[i + 1])) / t[i + 1])
        else:
            x = dpm_update(t, i, i0, x, d, dp)
            dp = d
    return x


def gated64(text, unc, g, interval, scale=0.9, bias=0.0):
    """The mock's denoiser in float64: guided (per-row scales g, plus the shared pass's marker bias) iff lo <= t <= hi, else plain."""
    t64, u64 = text.cpu().double(), unc.cpu().double()
    g64 = torch.as_tensor(g, dtype=torch.float64).cpu().reshape(-1, 1, 1, 1)
    d64 = lambda x, tx: scale * x + 0.3 * tx.mean(dim=(1, 2)).view(-1, 1, 1, 1)          # noqa: E731

    def den(x, t):
        if interval is None or interval[0] <= float(t) <= interval[1]:
            return (1.0 - g64) * d64(x, u64) + g64 * d64(x, t64) + bias
        return d64(x, t64)
    return den


def mock_inputs(seed, B=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(B, 4, 8, 8, device=DEV, generator=gen), torch.randn(B, 5, 16, device=DEV, generator=gen),
            torch.randn(B, 5, 16, device=DEV, generator=gen))


# ----------------------------------------------------------------------------------------------- 1. argument checks (CPU)
@pytest.mark.parametrize("bad", [(float("nan"), 1.0), (1.0, float("nan")), (-1.0, 2.0), (2.0, 2.0), (3.0, 1.0), (1.0,), 1.0, "1,2",
                                 (1.0, 2.0, 3.0), (INF, INF)])
def test_interval_argument_is_checked(bad):
    m = _RaisingMock(0.9)
    with pytest.raises(ValueError, match="guidance_interval"):
        EDM_Sampler(m, m, num_solve_steps=5, guidance=2.0, guidance_interval=bad)
    s = EDM_Sampler(m, m, num_solve_steps=5, guidance=2.0, guidance_interval=(0, INF))
    assert s.guidance_interval == (0.0, INF)
    with pytest.raises(ValueError, match="guidance_interval"):
        s.guidance_interval = bad
    assert s.guidance_interval == (0.0, INF)
    assert EDM_Sampler(m, m, num_solve_steps=5).guidance_interval is None


@pytest.mark.parametrize("shared", [False, True])
def test_guidance_vector_is_checked_before_any_device_work(shared):
    """CPU tensors and a model that raises RuntimeError when called: the ValueError comes first."""
    m = _RaisingMock(0.9)
    s = EDM_Sampler(m, m, num_solve_steps=5, guidance=2.0, shared_guidance=shared, guidance_interval=(1, 20))
    noise, text = torch.randn(3, 4, 8, 8), torch.randn(3, 5, 16)
    for bad in (torch.ones(2), torch.ones(3, 1), torch.ones(()), torch.tensor([1.0, float("nan"), 2.0]),
                torch.tensor([1.0, INF, 2.0]), [1.0, 2.0, 3.0], 2.0):
        with pytest.raises(ValueError, match="guidance"):
            s.sample(noise, text, TP, SOFT, text.flip(0), guidance=bad)
        with pytest.raises(ValueError, match="guidance"):
            s.denoise(noise, torch.tensor(1.0), text, TP, SOFT, text.flip(0), guidance=bad)
    assert s.last_evaluations is None and s._stage is None


def test_forward_guided_refuses_a_vector_of_another_shape(golden_full):
    from models import model_config1, model_config2
    g = golden_full
    cls = (model_config1 if g["variant"] == 1 else model_config2).preconditioned_HDMOEM
    model = cls(**g["cfg"]).eval()
    B = 2
    kw = dict(x=g["x"][:B], sigma=g["sigma"][:B], text_emb=g["text"][:B], uncond_text_emb=g["text"][:B].flip(0),
              Unet_router_mask=g["unet_mask"][:B], Vit_router_mask=g["vit_mask"][:B], zeta=0.0, **g["extra"])
    with torch.no_grad():
        for bad in (torch.ones(3), torch.ones(B, 1), torch.ones(()), torch.ones(B, dtype=torch.int64)):
            with pytest.raises(ValueError, match="guidance"):
                model.forward_guided(guidance=bad, **kw)


# ----------------------------------------------------------------------------------------------- 2. the plan (CPU)
def _plan(N, interval, i0=0, **kw):
    m = _RaisingMock(0.9)
    s = EDM_Sampler(m, m, num_solve_steps=N, guidance=2.0, guidance_interval=interval, **kw)
    t = s.t_schedule(None)
    assert torch.allclose(torch.from_numpy(t), schedule(N), rtol=1e-12, atol=0)
    return s.guidance_plan(t, i0)


def test_plan_heun():
    T, F = True, False
    plan = _plan(5, (1, 20))
    assert plan == [(F, T), (T, T), (T, F), (F, F), (F,)]
    assert {p for p in plan if len(p) == 2} == {(a, b) for a in (T, F) for b in (T, F)}          # all four full-stage variants
    assert sum(map(sum, plan)) == 4 and sum(map(len, plan)) == 9


def test_plan_heun_with_churn():
    """gamma = min(3 / 5, sqrt 2 - 1) where 0.05 <= t[i] <= 50: stage 0 (t = 80) is not churned, its second evaluation at 17.53 is
    guided; stage 1 starts at t_hat = 17.528 sqrt 2 = 24.79 (not guided); stage 2 at 2.5152 sqrt 2 = 3.557 (guided)."""
    T, F = True, False
    for dev in (False, True):
        plan = _plan(5, (1, 20), S_churn=3, S_min=0.05, S_max=50, churn_on_device=dev)
        assert plan[0] == (F, T) and plan[1] == (F, T) and plan[2] == (T, F) and plan[3] == (F, F) and plan[4] == (F,)
    assert math.isclose(17.528 * math.sqrt(2), 24.79, rel_tol=1e-3) and math.isclose(2.5152 * math.sqrt(2), 3.557, rel_tol=1e-3)
    # an interval that tells t[1] from t_hat[1]: (17, 18) holds 17.528 only
    assert _plan(5, (17, 18), S_churn=3, S_min=0.05, S_max=50)[:2] == [(F, T), (F, F)]
    assert _plan(5, (17, 18))[:2] == [(F, T), (T, F)]


@pytest.mark.parametrize("solver", ["dpmpp_2m", "dpmpp_2m_sde"])
def test_plan_dpm(solver):
    plan = _plan(6, (0.5, 10), solver=solver)
    assert plan == [(False,), (False,), (True,), (True,), (False,), (False,)]
    assert _plan(5, (1, 20), solver=solver) == [(False,), (True,), (True,), (False,), (False,)]


def test_plan_strength_and_full_interval():
    T, F = True, False
    N, strength = 5, 0.5
    i0 = N - math.ceil(strength * N)
    assert i0 == 2
    assert _plan(N, (1, 20), i0) == [(T, F), (F, F), (F,)]
    assert _plan(N, (1, 20), i0, solver="dpmpp_2m") == [(T,), (F,), (F,)]
    for interval in ((0, INF), None):
        assert _plan(N, interval) == [(T, T)] * 4 + [(T,)]
        assert _plan(6, interval, solver="dpmpp_2m") == [(T,)] * 6
    assert _plan(N, (1e3, 1e4)) == [(F, F)] * 4 + [(F,)]
    m = _RaisingMock(0.9)                                 # the bounds belong to the interval: [t[2], t[1]] as the schedule holds them
    s = EDM_Sampler(m, m, num_solve_steps=N, guidance=2.0)
    t = s.t_schedule(None)
    s.guidance_interval = (float(t[2]), float(t[1]))
    assert s.guidance_plan(t, 0) == [(F, T), (T, T), (T, F), (F, F), (F,)]


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


# ---- 3. per-row egress
EGRESS_SHAPES = {"1x3x5": (1, 3, 1, 5, [1.75]), "3x4x16": (3, 4, 4, 4, [0.0, 1.0, -0.5]), "5x4x64": (5, 4, 8, 8, [2.5, -0.5, 0.3, 7.0, 1.1])}


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(EGRESS_SHAPES))
def test_rows_egress_matches_float64(_gpu, dtype, shape):
    """out[n] = sx[n] x[n] + sf[n] ((1 - g[n]) F[N + n] + g[n] F[n]) against float64 within the scalar egress test's bound, and a constant
    vector against the scalar entry point, bit for bit."""
    from hdmoe_hip import ops
    N, C, H, W, gs = EGRESS_SHAPES[shape]
    gen = torch.Generator(device=DEV).manual_seed(5)
    F = (3.0 * torch.randn(2 * N, H, W, C, device=DEV, generator=gen)).to(dtype)
    x = torch.randn(N, C, H, W, device=DEV, generator=gen)
    sf = torch.rand(N, device=DEV, generator=gen) + 0.1
    sx = torch.rand(N, device=DEV, generator=gen) - 0.5
    g = torch.tensor(gs, device=DEV)
    out = ops.nhwc_to_nchw_guided(F, sf, x, sx, g)
    assert out.shape == (N, C, H, W) and out.dtype == torch.float32
    F64 = F.double().permute(0, 3, 1, 2).cpu()
    fc, fu = F64[:N], F64[N:]
    col = lambda v: v.double().cpu().view(-1, 1, 1, 1)                                           # noqa: E731
    sf64, sx64, g64, x64 = col(sf), col(sx), col(g), x.double().cpu()
    ref = sx64 * x64 + sf64 * ((1.0 - g64) * fu + g64 * fc)
    bound = 4 * EPS32 * ((sx64 * x64).abs() + sf64.abs() * ((1.0 - g64).abs() * fu.abs() + g64.abs() * fc.abs()))
    err = (out.double().cpu() - ref).abs()
    print(f"rows egress {shape} {dtype}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"{shape} {dtype}: max err / bound = {float((err / bound).max()):.3f}"
    for const in (0.0, 1.0, 2.5, -0.5):
        rows = ops.nhwc_to_nchw_guided(F, sf, x, sx, torch.full((N,), const, device=DEV))
        assert torch.equal(rows, ops.nhwc_to_nchw_guided(F, sf, x, sx, const)), f"constant vector {const} differs from the scalar kernel"
    for bad in (torch.ones(N + 1, device=DEV), torch.ones(N, device=DEV, dtype=torch.float64), torch.ones(N)):
        with pytest.raises(ValueError, match="guidance"):
            ops.nhwc_to_nchw_guided(F, sf, x, sx, bad)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("hdmoe_nhwc_to_nchw_guided_rows", out, F, sf, x, sx, None, N, C, H * W, 0 if dtype == torch.float32 else 1)
    torch.cuda.synchronize()


# ---- 4. lerp_rows
@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("per,offset", [(1, 0), (3, 0), (4, 0), (1024, 0), (4, 1), (1024, 1)])
def test_lerp_rows_matches_float64(_gpu, dtype, per, offset):
    """(1 - g[n]) ref[n] + g[n] d[n] against float64, rows = 5.  per = 3: a 16-byte vector would hold elements of two rows (the scalar
    path must run); offset = 1: the operands start one element into their buffers, so no 16-byte access is aligned (scalar path again);
    per = 4 / 1024 without offset: the 16-byte path in fp32 (4 only there) / both dtypes."""
    from hdmoe_hip import ops
    rows = 5
    gen = torch.Generator(device=DEV).manual_seed(7 + per)
    mk = lambda: (2.0 * torch.randn(rows * per + offset, device=DEV, generator=gen)).to(dtype)[offset:].view(rows, per)   # noqa: E731
    ref, d = mk(), mk()
    assert ref.data_ptr() % 16 == (offset * ref.element_size()) % 16
    g = torch.tensor([2.5, -0.5, 0.0, 1.0, 0.3], device=DEV)
    out = ops.lerp_rows(ref, d, g)
    assert out.shape == ref.shape and out.dtype == dtype
    g64, r64, d64 = g.double().cpu().view(-1, 1), ref.double().cpu(), d.double().cpu()
    exact = (1.0 - g64) * r64 + g64 * d64
    bound = 4 * EPS32 * ((1.0 - g64).abs() * r64.abs() + g64.abs() * d64.abs())
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (exact.abs() + bound)
    err = (out.double().cpu() - exact).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"lerp_rows per={per} offset={offset} {dtype}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), f"per={per} offset={offset} {dtype}: max err / bound = {ratio:.3f}"
    for const in (0.0, 2.0, 2.5, -0.5):                   # 1 - g exact in fp32
        vec = ops.lerp_rows(ref, d, torch.full((rows,), const, device=DEV))
        assert torch.equal(vec, ops.axpby(ref, d, 1.0 - const, const)), f"constant vector {const} differs from hdmoe_axpby"
        assert torch.equal(vec, ops.lerp_rows(ref, d, const))
    with pytest.raises(ValueError, match="guidance"):
        ops.lerp_rows(ref, d, torch.ones(rows + 1, device=DEV))
    with pytest.raises(ValueError, match="lerp_rows"):
        ops.lerp_rows(ref, d[:, :-1] if per > 1 else d[:-1], g)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("hdmoe_lerp_rows", out, ref, d, g, rows, 0, 0 if dtype == torch.float32 else 1)
    torch.cuda.synchronize()


# ---- 5. interval runs on the mock
SOLVERS = {"heun": dict(), "dpmpp_2m": dict(solver="dpmpp_2m"), "dpmpp_2m_sde": dict(solver="dpmpp_2m_sde", eta=0.0)}


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("solver", list(SOLVERS))
def test_interval_run_matches_restatement(_gpu, solver, use_graph, shared):
    """N = 5, interval (1, 20): guided at 17.528 and 2.5152 only (Heun: t[1] twice, t[2] twice; dpm: stages 1 and 2).  The shared pass
    carries a marker bias of 0.25 that the restatement adds to the guided evaluations alone: a stage replayed with the wrong variant is
    off by about the marker.  (dpmpp_2m_sde with eta = 0 draws nothing: the restatement is dpmpp_2m's.)"""
    N, guide, interval = 5, 2.5, (1.0, 20.0)
    noise, text, unc = mock_inputs(1)
    bias = 0.25 if shared else 0.0
    m = _MockDenoiser(0.9, guided_bias=bias).to(DEV)
    s = EDM_Sampler(m, m, num_solve_steps=N, guidance=guide, use_graph=use_graph, shared_guidance=shared, guidance_interval=interval,
                    **SOLVERS[solver])
    out = s.sample(noise, text, TP, SOFT, unc)
    ref = restate64("heun" if solver == "heun" else "dpm", gated64(text, unc, [guide] * 3, interval, bias=bias), noise, N)
    close_scaled(out, ref.float(), 1e-4, msg=f"{solver} graph={use_graph} shared={shared}: interval run vs the float64 restatement")
    n_g, n_p = (4, 5) if solver == "heun" else (2, 3)
    assert s.last_evaluations == {"guided": n_g, "plain": n_p}
    if use_graph:
        assert len(s._stage["g_heun" if solver == "heun" else "g_dpm"]) == (6 if solver == "heun" else 2)
    else:                                                 # replays do not call the module
        if shared:
            assert len(m.guided) == n_g and m.calls == n_p, "forward_guided for the guided evaluations only, forward for the rest"
            assert all(gd == guide for gd, _ in m.guided)
        else:
            assert not m.guided and m.calls == 2 * n_g + n_p, "two passes per guided evaluation, ONE per plain evaluation"
    # the interval is in effect: neither the always-guided nor the plain trajectory
    for other in (None, (1e3, 1e4)):
        o = EDM_Sampler(m, m, num_solve_steps=N, guidance=guide, shared_guidance=shared, guidance_interval=other,
                        **SOLVERS[solver]).sample(noise, text, TP, SOFT, unc)
        assert float((o - out).abs().max()) > 1e-2


@gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_interval_host_loops(_gpu, use_graph):
    """The host-driven loops consult the same plan: bf16 latents (no fused stage) through _eval, with use_graph the captured evaluation
    in its two variants.  Counts only (bf16 latents against float64 would need a bound of their own), plus eager == replay."""
    N, interval = 5, (1.0, 20.0)
    noise, text, unc = mock_inputs(2)
    for solver, (n_g, n_p) in (("heun", (4, 5)), ("dpmpp_2m", (2, 3))):
        m = _MockDenoiser(0.9, guided_bias=0.25).to(DEV)
        s = EDM_Sampler(m, m, num_solve_steps=N, guidance=2.0, dtype=torch.bfloat16, use_graph=use_graph, shared_guidance=True,
                        guidance_interval=interval, solver=solver)
        out = s.sample(noise, text, TP, SOFT, unc)
        assert not (s.fused_heun or s.fused_dpm) and s.last_evaluations == {"guided": n_g, "plain": n_p}
        if use_graph:
            assert len(s._graph["g_eval"]) == 2
            eager = EDM_Sampler(m, m, num_solve_steps=N, guidance=2.0, dtype=torch.bfloat16, shared_guidance=True,
                                guidance_interval=interval, solver=solver).sample(noise, text, TP, SOFT, unc)
            assert torch.equal(out, eager)
        else:
            assert len(m.guided) == n_g and m.calls == n_p


# ---- 6. replay against eager, bit for bit
REPLAY_CASES = {
    "heun": dict(),
    "dpmpp_2m": dict(solver="dpmpp_2m"),
    "dpmpp_2m_sde": dict(solver="dpmpp_2m_sde", eta=0.5),
    "churn_on_device": dict(S_churn=3.0, S_min=0.05, S_max=50.0, churn_on_device=True),
}


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("case", list(REPLAY_CASES))
def test_interval_replay_equals_eager(_gpu, case, shared):
    """N = 6, interval (0.5, 10): the mock's elementwise arithmetic and the same stage function, so the replay of the per-stage variants
    is the eager trajectory bit for bit (a wrong variant would be off by the marker)."""
    noise, text, unc = mock_inputs(3)
    m = _MockDenoiser(0.9, guided_bias=0.25).to(DEV)
    kw = dict(seed=12345) if case in ("dpmpp_2m_sde", "churn_on_device") else {}
    mk = lambda **o: EDM_Sampler(m, m, num_solve_steps=6, guidance=2.0, shared_guidance=shared, guidance_interval=(0.5, 10.0),  # noqa: E731
                                 **REPLAY_CASES[case], **o)
    eager_s, graph_s = mk(), mk(use_graph=True)
    eager = eager_s.sample(noise, text, TP, SOFT, unc, **kw)
    graphed = graph_s.sample(noise, text, TP, SOFT, unc, **kw)
    assert torch.isfinite(eager).all() and (graph_s.fused_heun or graph_s.fused_dpm)
    assert eager_s.last_evaluations == graph_s.last_evaluations
    assert 0 < eager_s.last_evaluations["guided"] and 0 < eager_s.last_evaluations["plain"]
    assert torch.equal(graphed, eager), f"{case}: max diff {float((graphed - eager).abs().max()):.3e}"
    assert torch.equal(graph_s.sample(noise, text, TP, SOFT, unc, **kw), eager)                 # and again


# ---- 7. no recapture
@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_no_recapture_for_bounds_scales_prompt_strength(_gpu, solver, shared):
    noise, text, unc = mock_inputs(4)
    _, text2, unc2 = mock_inputs(5)
    x0 = mock_inputs(6)[0]
    m = _MockDenoiser(0.9, guided_bias=0.25).to(DEV)
    kw = dict(num_solve_steps=6, guidance=2.0, solver=solver, shared_guidance=shared)
    graphed = EDM_Sampler(m, m, use_graph=True, guidance_interval=(1.0, 20.0), **kw)
    g1 = torch.tensor([2.0, 0.0, 3.5])
    g2 = torch.tensor([-0.5, 1.0, 7.0], device=DEV)
    out0 = graphed.sample(noise, text, TP, SOFT, unc, guidance=g1)
    stage = graphed._stage
    name = "g_heun" if solver == "heun" else "g_dpm"
    assert len(stage[name]) == (6 if solver == "heun" else 2)
    assert stage["key"][-1] is shared and stage["key"][-2] is True
    graphs = list(stage[name])
    steps = [((0.5, 10.0), g1, text, unc, {}), ((0.5, 10.0), g2, text, unc, {}), ((0.5, 10.0), g2, text2, unc2, {}),
             ((0.0, INF), g2, text2, unc2, dict(init_latents=x0, strength=0.5)), ((1.0, 20.0), g1, text, unc, {})]
    prev = out0
    for interval, g, tx, uc, extra in steps:
        graphed.guidance_interval = interval
        out = graphed.sample(noise, tx, TP, SOFT, uc, guidance=g, **extra)
        assert graphed._stage is stage and list(stage[name]) == graphs, f"recaptured at {interval} {extra}"
        eager = EDM_Sampler(m, m, guidance_interval=interval, **kw).sample(noise, tx, TP, SOFT, uc, guidance=g, **extra)
        assert torch.equal(out, eager), f"{interval} {extra}: the replay differs from a fresh eager sampler"
        assert float((out - prev).abs().max()) > 1e-3     # every step changed something that matters
        prev = out
    assert torch.equal(prev, out0)                        # the last step is the first call again
    # no interval: today's capture, two graphs for Heun (full, last), one for dpm
    graphed.guidance_interval = None
    out = graphed.sample(noise, text, TP, SOFT, unc, guidance=g1)
    assert graphed._stage is not stage and len(graphed._stage[name]) == (2 if solver == "heun" else 1)
    assert graphed._stage["key"][-1] is shared and graphed._stage["key"][-2] is False
    assert torch.equal(out, EDM_Sampler(m, m, **kw).sample(noise, text, TP, SOFT, unc, guidance=g1))
    # a float scale: still part of the key
    stage = graphed._stage
    graphed.sample(noise, text, TP, SOFT, unc)
    float_stage = graphed._stage
    assert float_stage is not stage
    graphed.guide = 3.0
    graphed.sample(noise, text, TP, SOFT, unc)
    assert graphed._stage is not float_stage


# ---- 8. per-sample vector
@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_per_sample_vector(_gpu, solver, use_graph, shared):
    N = 5
    noise, text, unc = mock_inputs(9)
    m = _MockDenoiser(0.9).to(DEV)
    kw = dict(num_solve_steps=N, solver=solver, use_graph=use_graph, shared_guidance=shared)
    gs = [2.0, 0.0, 3.5]
    for interval in (None, (1.0, 20.0)):
        s = EDM_Sampler(m, m, guidance=1.0, guidance_interval=interval, **kw)      # the float is not used: the vector is the scale
        out = s.sample(noise, text, TP, SOFT, unc, guidance=torch.tensor(gs, dtype=torch.float64))
        ref = restate64("heun" if solver == "heun" else "dpm", gated64(text, unc, gs, interval), noise, N)
        close_scaled(out, ref.float(), 1e-4, msg=f"{solver} graph={use_graph} shared={shared} interval={interval}: per-sample scales")
        n_eval = 2 * N - 1 if solver == "heun" else N
        assert s.last_evaluations["guided"] == (n_eval if interval is None else (4 if solver == "heun" else 2))
        # rows differ by their scale: row 1 (g = 0) is the unconditional trajectory, not the conditional one
        plain = EDM_Sampler(m, m, guidance=1.0, **kw).sample(noise, text, TP, SOFT, unc)
        assert float((out[1] - plain[1]).abs().max()) > 1e-3
        const = s.sample(noise, text, TP, SOFT, unc, guidance=torch.full((3,), 2.0))
        flt = EDM_Sampler(m, m, guidance=2.0, guidance_interval=interval, **kw).sample(noise, text, TP, SOFT, unc)
        assert torch.equal(const, flt), "a vector filled with 2.0 differs from guidance=2.0"


# ---- real model (config-2 golden weights)
def _load(g):
    from models import model_config1, model_config2
    cls = (model_config1 if g["variant"] == 1 else model_config2).preconditioned_HDMOEM
    model = cls(**g["cfg"])
    model.load_state_dict(g["state"])
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def real_model(_gpu):
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    model = _load(g)
    gen = torch.Generator(device=DEV).manual_seed(0)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    EDM_Sampler(model, model, num_solve_steps=2).sample(noise, g["text"][:2].to(DEV), TP, SOFT)     # registers the weight bank
    return model, g


def _real_inputs(g, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    return noise, text, torch.randn(text.shape, device=DEV, generator=gen)


# ---- 9. bit-exact ends
@gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_interval_ends_are_bit_exact(real_model, solver, shared, use_graph):
    """Interval (0, inf) is guidance_interval=None, and an interval that holds no sigma of the schedule is guidance = 1: no tolerance."""
    model, g = real_model
    noise, text, unc = _real_inputs(g, 21)
    kw = dict(num_solve_steps=3, solver=solver, shared_guidance=shared, use_graph=use_graph)
    run = lambda **o: EDM_Sampler(model, model, **kw, **o).sample(noise, text, TP, SOFT, unc)    # noqa: E731
    always, full = run(guidance=2.0), run(guidance=2.0, guidance_interval=(0.0, INF))
    assert torch.isfinite(always).all() and torch.equal(full, always)
    plain, never = run(guidance=1.0), run(guidance=2.0, guidance_interval=(1e3, 1e4))
    assert torch.equal(never, plain)
    assert float((always - plain).abs().max()) > 1e-4


# ---- 10. one evaluation with a per-sample vector
@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
def test_one_evaluation_with_per_sample_scales(real_model, shared):
    """Row n of denoise(guidance=[2.5, -0.5]) is row n of the float run with g_n, bit for bit: the two passes / F do not depend on the
    scale, and the per-row kernels reproduce the scalar ones.  guided=False is the guidance = 1 evaluation."""
    model, g = real_model
    x, text, unc = _real_inputs(g, 22)
    sig = torch.tensor(1.3, device=DEV)
    gs = [2.5, -0.5]
    with torch.no_grad():
        vec = EDM_Sampler(model, model, num_solve_steps=4, shared_guidance=shared).denoise(x, sig, text, TP, SOFT, unc,
                                                                                          guidance=torch.tensor(gs))
        for n, gn in enumerate(gs):
            flt = EDM_Sampler(model, model, num_solve_steps=4, guidance=gn, shared_guidance=shared).denoise(x, sig, text, TP, SOFT, unc)
            assert torch.equal(vec[n], flt[n]), f"row {n} (g = {gn}): max diff {float((vec[n] - flt[n]).abs().max()):.3e}"
        assert float((vec[0] - vec[1]).abs().max()) > 1e-4
        plain = EDM_Sampler(model, model, num_solve_steps=4, guidance=1.0).denoise(x, sig, text, TP, SOFT, unc)
        off = EDM_Sampler(model, model, num_solve_steps=4, guidance=2.0, shared_guidance=shared).denoise(
            x, sig, text, TP, SOFT, unc, guidance=torch.tensor(gs), guided=False)
        assert torch.equal(off, plain)
        if shared:                                        # forward_guided itself, with a vector on the host
            out = model.forward_guided(x=x, sigma=sig, text_emb=text, uncond_text_emb=unc, guidance=torch.tensor(gs, dtype=torch.float64),
                                       Unet_router_mask=torch.ones(2, model.num_experts, device=DEV),
                                       Vit_router_mask=torch.ones(2, model.num_experts, device=DEV), zeta=0, transition_point=TP,
                                       softness=SOFT)["denoised"]
            assert torch.equal(out, vec)


# ---- 11. a short trajectory against the CPU oracle
# Measured on an MI355X with the PARENT commit's tree: max|two-pass - oracle trajectory| / max|oracle trajectory| of the always-guided
# two-pass path (fp32 compute mode, B = 2, N = 5, g = 2.0, TRAJ_SEED, the inputs of trajectory_case in tests/test_sampler_shared_guidance.py).
# The interval run is allowed 4x it, the existing test's allowance: the same kernels, chained evaluations, fewer of them amplified.
TWO_PASS_ERR_N5 = {"heun": 5.381e-06, "dpmpp_2m": 3.484e-06}     # (its shared path: 5.440e-06 / 4.057e-06 in the same run)
TRAJ_SEED = 0
TRAJ_INTERVAL = (1.0, 20.0)


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_interval_trajectory_against_oracle(real_model, solver, shared):
    from oracle import hdmoe_oracle as O
    model, g = real_model
    N, B, guide = 5, 2, 2.0
    lo, hi = TRAJ_INTERVAL
    gen = torch.Generator().manual_seed(TRAJ_SEED)
    noise = torch.randn(B, 4, 16, 16, generator=gen)
    text = g["text"][:B]
    unc = torch.randn(text.shape, generator=gen)
    E, k = g["cfg"]["num_experts"], g["cfg"]["top_k"]
    ones = torch.ones(B, E)
    seen = []

    def oracle_den(x, t):
        guided = lo <= float(t) <= hi
        with torch.no_grad():
            outs = [O.preconditioned_hdmoem(g["state"], g["cfg"], 2, x.float(), t.float(), tx, ones, ones, transition_point=TP, softness=SOFT)
                    for tx in ((text, unc) if guided else (text,))]
        seen.append((x.float(), t.float(), guided, [torch.topk(outs[0][key], k, dim=-1) for key in ("Unet_raw", "vit_raw")]))
        return (O.cfg_lerp(outs[0]["denoised"], outs[1]["denoised"], guide) if guided else outs[0]["denoised"]).to(x.dtype)

    ref = O.edm_sampler(oracle_den, noise, N) if solver == "heun" else restate64("dpm", oracle_den, noise, N)
    n_g, n_p = (4, 5) if solver == "heun" else (2, 3)
    assert [s[2] for s in seen].count(True) == n_g and len(seen) == n_g + n_p
    exact = True
    with torch.no_grad():
        for x, t, _, tops in seen:
            out = model(x=x.to(DEV), sigma=t.to(DEV), text_emb=text.to(DEV), Unet_router_mask=ones.to(DEV), Vit_router_mask=ones.to(DEV),
                        zeta=0, transition_point=TP, softness=SOFT)
            for key, top in zip(("Unet_raw", "vit_raw"), tops):
                exact &= torch.equal(torch.topk(out[key].cpu(), k, dim=-1).indices, top.indices)
    run = lambda **o: EDM_Sampler(model, model, num_solve_steps=N, solver=solver, shared_guidance=shared, **o).sample(  # noqa: E731
        noise.to(DEV), text.to(DEV), TP, SOFT, unc.to(DEV)).cpu()
    s = EDM_Sampler(model, model, num_solve_steps=N, guidance=guide, solver=solver, shared_guidance=shared, guidance_interval=TRAJ_INTERVAL)
    out = s.sample(noise.to(DEV), text.to(DEV), TP, SOFT, unc.to(DEV)).cpu()
    err = float((out.double() - ref.double()).abs().max()) / float(ref.abs().max())
    print(f"{solver} shared={shared}: interval err {err:.3e} (relative to max|oracle trajectory|), bound 4 x {TWO_PASS_ERR_N5[solver]}, "
          f"routing exact: {exact}")
    assert s.last_evaluations == {"guided": n_g, "plain": n_p}
    assert exact, "the GPU routing differs from the oracle's on this seed (a near-tie): pick another TRAJ_SEED"
    assert torch.isfinite(out).all()
    assert err <= 4 * TWO_PASS_ERR_N5[solver], f"{solver}: interval err {err:.3e} > 4 x {TWO_PASS_ERR_N5[solver]:.3e}"
    assert float((out - run(guidance=guide)).abs().max()) > 1e-4, "the interval run is the always-guided run"
    assert float((out - run(guidance=1.0)).abs().max()) > 1e-4, "the interval run is the plain run"


# ---- 12. an unguided evaluation really is one pass
@gpu
def test_launch_log_of_an_unguided_evaluation(real_model):
    from hdmoe_hip import _lib
    model, g = real_model
    x, text, unc = _real_inputs(g, 23)
    sig = torch.tensor(1.3, device=DEV)
    logs = {}
    for name, kw, call_kw in (("unguided", dict(guidance=2.0, shared_guidance=True, guidance_interval=(1e3, 1e4)), dict(guided=False)),
                              ("unguided_vec", dict(guidance=2.0, shared_guidance=True), dict(guided=False, guidance=torch.ones(2) * 3)),
                              ("one", dict(guidance=1.0), {}), ("guided", dict(guidance=2.0, shared_guidance=True), {})):
        s = EDM_Sampler(model, model, num_solve_steps=4, **kw)
        with torch.no_grad():
            s.denoise(x, sig, text, TP, SOFT, unc, **call_kw)               # warm: nothing one-off in the log
            _lib.CALL_LOG = []
            try:
                s.denoise(x, sig, text, TP, SOFT, unc, **call_kw)
                logs[name] = [n for n, _ in _lib.CALL_LOG]
            finally:
                _lib.CALL_LOG = None
    print({k: len(v) for k, v in logs.items()})
    for name in ("unguided", "unguided_vec"):
        assert not [n for n in logs[name] if n.startswith("hdmoe_nhwc_to_nchw_guided") or n == "hdmoe_gather_rows_paired"]
        assert logs[name] == logs["one"], "an unguided evaluation makes the library calls of a guidance = 1 evaluation"
    assert logs["guided"].count("hdmoe_nhwc_to_nchw_guided") == 1 and logs["guided"].count("hdmoe_gather_rows_paired") > 0
