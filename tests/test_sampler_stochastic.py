"""Stochastic sampling on the device: EDM_Sampler(churn_on_device=True) (churned Heun) and solver="dpmpp_2m_sde" (DPM-Solver++(2M) SDE).

The RNG contract: stage i of a sample() call with seed S draws, for latent element j, the value hdmoe_randn(out, seed=S, seed_dev=&c,
scale=1, n) writes to out[j] with c == i.  Every reference below regenerates eps through hdmoe_randn in exactly that form.

CPU tests: constructor / seed checks.  GPU tests: hdmoe_heun_churn, the t_hat forms of the Heun updates and hdmoe_dpm2m_sde_step against
float64; the moments of the draws; trajectories against a float64 restatement with every conditioning keyword; eager vs hipGraph replay;
seeding rules; evaluation counts; recapture; the bf16 host loops.

Tolerances (close_scaled, the form and values of tests/test_sampler_dpm_solver.py): a kernel against float64 2e-6, a sampled trajectory or
a host loop against the float64 restatement 1e-4.  Draw statistics over n = 2^20 elements: six standard errors of the estimator, i.e.
|mean| <= 6 / sqrt(n), |var - 1| <= 6 sqrt(2 / n), |corr| <= 6 / sqrt(n); the 24-bit uniforms and the fp32 Box-Muller bias the variance by
about 1e-6, far inside 8.3e-3."""
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
SDE = "dpmpp_2m_sde"
SEED_A, SEED_B = 0xDEADBEEFCAFEF00D, 12345               # one above 2^63 (the device word holds its two's complement)
GAMMA_MAX = math.sqrt(2) - 1


class _MockDenoiser(torch.nn.Module):
    """Linear mock denoiser D = scale * x; counts its calls."""

    def __init__(self, scale, num_experts=4):
        super().__init__()
        self.num_experts = num_experts
        self.scale = scale
        self.calls = 0

    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, transition_point, softness, return_log_var=False):
        self.calls += 1
        assert sigma.ndim == 0 and Unet_router_mask.shape == (x.shape[0], self.num_experts) and zeta == 0
        return {"denoised": x * self.scale}


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


def mocks():
    return _MockDenoiser(0.9).to(DEV), _MockDenoiser(0.5).to(DEV)


# ----------------------------------------------------------------------------------------------- CPU: argument checks
def test_sde_with_churn_raises():
    with pytest.raises(ValueError, match="solver"):
        EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4, S_churn=1.0, solver=SDE)


@pytest.mark.parametrize("bad", [-0.5, float("inf"), float("-inf"), float("nan"), "much", None])
def test_bad_eta_raises(bad):
    with pytest.raises(ValueError, match="eta"):
        EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4, solver=SDE, eta=bad)


@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_eta_with_other_solver_raises(solver):
    with pytest.raises(ValueError, match="eta"):
        EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4, solver=solver, eta=0.5)
    EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4, solver=solver, eta=1.0)        # the default is accepted


def test_new_options_build_nothing():
    for kw in (dict(S_churn=2.0, churn_on_device=True), dict(churn_on_device=True), dict(solver=SDE), dict(solver=SDE, eta=0.0)):
        s = EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4, use_graph=True, **kw)
        assert not s.fused_heun and not s.fused_dpm and s._stage is None and s._graph is None
    s = EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4)
    assert s.churn_on_device is False and s.eta == 1.0


@pytest.mark.parametrize("bad", [-1, 1 << 64, 1.5, "7", True, float("nan")])
def test_bad_seed_raises_before_device_work(bad):
    """CPU tensors: any device work would raise RuntimeError (no CPU fallback) instead of the ValueError."""
    for kw in (dict(S_churn=2.0, churn_on_device=True), dict(solver=SDE), {}):
        s = EDM_Sampler(_MockDenoiser(0.9), _MockDenoiser(0.5), num_solve_steps=4, **kw)
        with pytest.raises(ValueError, match="seed"):
            s.sample(torch.randn(1, 4, 8, 8), torch.randn(1, 5, 16), -1.2, 1.6, seed=bad)
        assert s._stage is None and s._graph is None


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


def seed_word(S):
    return torch.tensor([S - (1 << 64) if S >= 1 << 63 else S], dtype=torch.int64, device=DEV)


def contract_eps(n, S, i):
    """The contract itself: hdmoe_randn with seed = S and a device counter holding i, scale 1."""
    from hdmoe_hip import ops
    out = torch.empty(n, device=DEV)
    ops.call("hdmoe_randn", out, S, torch.tensor([i], dtype=torch.int64, device=DEV), 1.0, n)
    return out


def _views(n, k, misaligned, gen):
    """k fp32 device vectors of n elements, each 4 bytes past a 16-byte boundary when misaligned (the scalar path)."""
    off = 1 if misaligned else 0
    out = []
    for _ in range(k):
        buf = torch.randn(n + 4, device=DEV, generator=gen)
        v = buf[off:off + n]
        assert (v.data_ptr() % 16 != 0) == misaligned
        out.append(v)
    return out


@gpu
def test_randn_keyed_is_the_contract(_gpu):
    from hdmoe_hip import ops
    for S, i, n in ((SEED_A, 0, 1024), (SEED_A, 7, 1027), (SEED_B, 3, 5), ((1 << 64) - 1, 39, 4096)):
        assert torch.equal(ops.randn_keyed(torch.empty(n, device=DEV), S, i), contract_eps(n, S, i)), (S, i, n)
    assert not torch.equal(contract_eps(1024, SEED_A, 0), contract_eps(1024, SEED_A, 1))


# (n, misaligned): the 16-byte path; the scalar path by alignment with n % 4 != 0; the scalar path by n % 4 alone
SHAPES = [(4096, False), (4 * 257 + 3, True), (4 * 64 + 2, False)]


@gpu
@pytest.mark.parametrize("n,misaligned", SHAPES)
@pytest.mark.parametrize("in_place", [False, True])
def test_churn_kernel_matches_float64(_gpu, n, misaligned, in_place):
    from hdmoe_hip import ops
    N = 8
    t = schedule(N)
    td = t.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(21)
    s_min, s_max, s_noise, gcap = 0.05, 50.0, 1.007, min(3.0 / N, GAMMA_MAX)
    inside = [i for i in range(N) if s_min <= float(t[i]) <= s_max]
    outside = [i for i in range(N) if not s_min <= float(t[i]) <= s_max]
    assert 0 in outside and N - 1 in outside and len(inside) >= 3       # both ends of the window are exercised
    for S in (SEED_A, SEED_B):
        for i in range(N):
            x, out = _views(n, 2, misaligned, gen)
            x_in = x.clone()
            sig = torch.zeros((), device=DEV)
            that = torch.zeros(1, dtype=torch.float64, device=DEV)
            idx = torch.tensor([i], dtype=torch.int32, device=DEV)
            dst = x if in_place else out
            ops.heun_churn(dst, x, sig, that, td, idx, seed_word(S), gcap, s_min, s_max, s_noise)
            tc = float(t[i])
            gamma = gcap if i in inside else 0.0
            th = tc + gamma * tc
            tag = f"seed={S:#x} i={i} n={n} misaligned={misaligned} in_place={in_place}"
            assert float(that) == th, f"{tag}: t_hat {float(that)!r} != {th!r}"
            assert float(sig) == float(torch.tensor(th, dtype=torch.float64).float()), f"{tag}: sigma is not (float) t_hat"
            if i in outside:
                assert torch.equal(dst, x_in), f"{tag}: outside the window x_hat must be x bit-for-bit"
            else:
                eps = contract_eps(n, S, i).cpu().double()
                ref = x_in.cpu().double() + math.sqrt(th * th - tc * tc) * s_noise * eps
                close_scaled(dst, ref, 2e-6, msg=tag)
                assert not torch.equal(dst, x_in)
            if not in_place:
                assert torch.equal(x, x_in), f"{tag}: x changed"
            assert int(idx) == i


@gpu
def test_churn_kernel_invalid_arguments(_gpu):
    from hdmoe_hip import ops
    n = 64
    t = schedule(4).to(DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    x, out = torch.randn(n, device=DEV), torch.empty(n, device=DEV)
    sig, that, sd = torch.zeros((), device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV), seed_word(1)
    ok = (out, x, sig, that, t, idx, sd, 0.3, 0.0, float("inf"), 1.0, n)
    ops.call("hdmoe_heun_churn", *ok)
    bad = {f"null arg {k}": ok[:k] + (None,) + ok[k + 1:] for k in range(7)}
    bad.update({
        "gamma_cap < 0": ok[:7] + (-0.1,) + ok[8:], "gamma_cap nan": ok[:7] + (float("nan"),) + ok[8:],
        "gamma_cap inf": ok[:7] + (float("inf"),) + ok[8:], "s_min nan": ok[:8] + (float("nan"),) + ok[9:],
        "s_max nan": ok[:9] + (float("nan"),) + ok[10:], "s_noise < 0": ok[:10] + (-1.0, n), "s_noise inf": ok[:10] + (float("inf"), n),
        "n < 0": ok[:11] + (-4,),
    })
    for what, args in bad.items():
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.call("hdmoe_heun_churn", *args)
            pytest.fail(what)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("n,misaligned", SHAPES[:2])
@pytest.mark.parametrize("with_known", [False, True])
def test_heun_updates_from_t_hat(_gpu, n, misaligned, with_known):
    """t_hat == t[idx]: the _hat entry points equal hdmoe_heun_euler / hdmoe_heun_correct bit-for-bit.  t_hat > t[idx]: float64."""
    from hdmoe_hip import ops
    N = 6
    t = schedule(N)
    td = t.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(22)
    for i in (0, 2, N - 2):
        xh, den, xn, den2, x0, nz, mk, o1, o2 = _views(n, 9, misaligned, gen)
        mk.uniform_(0, 1, generator=gen)
        mk[: n // 3] = 1.0
        mk[n // 3: n // 2] = 0.0
        known = (x0, nz, mk) if with_known else None
        idx = torch.tensor([i], dtype=torch.int32, device=DEV)
        tc, tn = float(t[i]), float(t[i + 1])
        for gamma in (0.0, 0.3):
            th = tc + gamma * tc
            that = torch.tensor([th], dtype=torch.float64, device=DEV)
            tag = f"i={i} gamma={gamma} n={n} known={with_known}"
            X, D, Xn, D2 = (v.cpu().double() for v in (xh, den, xn, den2))
            h = tn - th

            def blend(r):
                if not with_known:
                    return r
                m64 = mk.cpu().double()
                return m64 * (x0.cpu().double() + tn * nz.cpu().double()) + (1 - m64) * r

            ops.heun_euler(o1, xh, den, td, idx, known, that)
            if gamma == 0.0:
                ops.heun_euler(o2, xh, den, td, idx, known)
                assert torch.equal(o1, o2), f"{tag}: euler from t_hat == t[idx] differs from hdmoe_heun_euler"
            close_scaled(o1, blend(X + h * (X - D) / th), 2e-6, msg=f"euler {tag}")
            ops.heun_correct(o1, xh, den, xn, den2, td, idx, known, that)
            if gamma == 0.0:
                ops.heun_correct(o2, xh, den, xn, den2, td, idx, known)
                assert torch.equal(o1, o2), f"{tag}: correct from t_hat == t[idx] differs from hdmoe_heun_correct"
            close_scaled(o1, blend(X + h * (0.5 * (X - D) / th + 0.5 * (Xn - D2) / tn)), 2e-6, msg=f"correct {tag}")
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("hdmoe_heun_euler_hat", o1, xh, den, td, idx, None, n, None, None, None)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("hdmoe_heun_correct_hat", o1, xh, den, xn, den2, td, idx, None, n, None, None, None)


def sde_update(t, i, i0, x, d, dp, eta, s_noise, eps):
    """DPM-Solver++(2M) SDE, midpoint form, in float64 (eps: the stage's draw, or None when nothing may be drawn)."""
    if t[i + 1] == 0:
        return d.clone()
    e = torch.exp(-eta * torch.log(t[i] / t[i + 1]))
    a = t[i + 1] / t[i] * e
    if i <= i0:
        x = a * x + (1 - a) * d
    else:
        r = torch.log(t[i - 1] / t[i]) / torch.log(t[i] / t[i + 1])
        x = a * x + (1 - a) * ((1 + 1 / (2 * r)) * d - (1 / (2 * r)) * dp)
    if eta > 0:
        x = x + t[i + 1] * torch.sqrt(1 - e * e) * s_noise * eps
    return x


BRANCHES = lambda N: ((0, 0), (2, 2), (1, 0), (4, 2), (N - 1, 0), (N - 1, N - 1))       # noqa: E731  (idx, i0): first, second, last


@gpu
@pytest.mark.parametrize("n,misaligned", SHAPES[:2])
@pytest.mark.parametrize("with_known", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
def test_sde_kernel(_gpu, n, misaligned, with_known, in_place):
    from hdmoe_hip import ops
    N = 6
    t = schedule(N)
    td = t.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(23)
    s_noise = 1.0 + 2.0 ** -7                                  # a float32 value: the launch scalar is a float
    for eta in (0.0, 0.5, 1.0):
        for i, i0 in BRANCHES(N):
            x, den, dp, x0, nz, mk, out, out2, dp2 = _views(n, 9, misaligned, gen)
            mk.uniform_(0, 1, generator=gen)
            mk[: n // 3] = 1.0
            mk[n // 3: n // 2] = 0.0
            known = (x0, nz, mk) if with_known else None
            if i <= i0 or i == N - 1:                       # den_prev is no input of the first-order and last stages
                dp.fill_(float("nan"))
            dp2.copy_(dp)
            x_in, den_in, dp_in = x.clone(), den.clone(), dp.clone()
            idx = torch.tensor([i], dtype=torch.int32, device=DEV)
            i0d = torch.tensor([i0], dtype=torch.int32, device=DEV)
            tag = f"eta={eta} i={i} i0={i0} n={n} known={with_known} in_place={in_place}"
            if eta == 0.0:
                ops.dpm2m_step(out2, x, den, dp2, td, idx, i0d, known)
            dst = x if in_place else out
            ops.dpm2m_sde_step(dst, x, den, dp, td, idx, i0d, eta, s_noise, seed_word(SEED_A), known)
            if eta == 0.0:
                assert torch.equal(dst, out2), f"{tag}: eta = 0 is not hdmoe_dpm2m_step bit-for-bit"
            eps = contract_eps(n, SEED_A, i).cpu().double()
            ref = sde_update(t, i, i0, x_in.cpu().double(), den_in.cpu().double(), dp_in.cpu().double(), eta, s_noise, eps)
            if with_known:
                m64 = mk.cpu().double()
                ref = m64 * (x0.cpu().double() + t[i + 1] * nz.cpu().double()) + (1 - m64) * ref
            close_scaled(dst, ref, 2e-6, msg=tag)
            assert torch.equal(dp, den_in), f"{tag}: den_prev is not den afterwards"
            assert torch.equal(den, den_in), f"{tag}: den changed"
            if i == N - 1:
                want = den_in.clone()
                if with_known:
                    keep = mk == 1
                    assert torch.equal(dst[keep], x0[keep]), f"{tag}: known region is not x0 at sigma = 0"
                    want[keep] = x0[keep]
                    free = mk == 0
                    assert torch.equal(dst[free], den_in[free]), tag
                else:
                    assert torch.equal(dst, want), f"{tag}: the last stage must return den"
            assert int(idx) == i and int(i0d) == i0


@gpu
def test_sde_kernel_invalid_arguments(_gpu):
    from hdmoe_hip import ops
    n = 64
    t = schedule(4).to(DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    i0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    x, den, dp, x0, nz, m = (torch.randn(n, device=DEV) for _ in range(6))
    big = torch.randn(2 * n, device=DEV)
    sd = seed_word(3)
    tail = (1.0, 1.0, sd)
    ok = (x, x, den, dp, t, idx, i0, n, None, None, None) + tail
    ops.call("hdmoe_dpm2m_sde_step", *ok)
    bad = {f"null arg {k}": ok[:k] + (None,) + ok[k + 1:] for k in range(7)}
    bad.update({
        "n < 0": ok[:7] + (-4, None, None, None) + tail,
        "partial known (x0 only)": ok[:8] + (x0, None, None) + tail,
        "partial known (no mask)": ok[:8] + (x0, nz, None) + tail,
        "den_prev is den": (x, x, den, den, t, idx, i0, n, None, None, None) + tail,
        "den_prev is x_out": (dp, x, den, dp, t, idx, i0, n, None, None, None) + tail,
        "den_prev is x": (x, dp, den, dp, t, idx, i0, n, None, None, None) + tail,
        "den_prev overlaps den": (x, x, big[:n], big[n // 2: n // 2 + n], t, idx, i0, n, None, None, None) + tail,
        "null seed": ok[:11] + (1.0, 1.0, None),
        "eta < 0": ok[:11] + (-0.5, 1.0, sd), "eta nan": ok[:11] + (float("nan"), 1.0, sd), "eta inf": ok[:11] + (float("inf"), 1.0, sd),
        "s_noise < 0": ok[:11] + (1.0, -1.0, sd), "s_noise nan": ok[:11] + (1.0, float("nan"), sd),
        "s_noise inf": ok[:11] + (1.0, float("inf"), sd),
    })
    for what, args in bad.items():
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.call("hdmoe_dpm2m_sde_step", *args)
            pytest.fail(what)
    torch.cuda.synchronize()


@gpu
def test_draw_statistics(_gpu):
    """n = 2^20 draws per stage, recovered from the churn kernel as (x_hat - x) / c: mean, variance, and correlation between consecutive
    stages and between two seeds, each within six standard errors (module docstring)."""
    from hdmoe_hip import ops
    n = 1 << 20
    N = 8
    t = schedule(N)
    td = t.to(DEV)
    gcap = GAMMA_MAX
    gen = torch.Generator(device=DEV).manual_seed(24)
    x = torch.randn(n, device=DEV, generator=gen)

    def recovered(S, i):
        out = torch.empty_like(x)
        sig, that = torch.zeros((), device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.heun_churn(out, x, sig, that, td, torch.tensor([i], dtype=torch.int32, device=DEV), seed_word(S), gcap, 0.0, float("inf"), 1.0)
        tc = float(t[i])
        th = tc + gcap * tc
        c = float(torch.tensor(math.sqrt(th * th - tc * tc), dtype=torch.float64).float())
        return ((out.double() - x.double()) / c).cpu()

    i = 3
    e_a0, e_a1, e_b0 = recovered(SEED_A, i), recovered(SEED_A, i + 1), recovered(SEED_B, i)
    ref = contract_eps(n, SEED_A, i).cpu().double()
    assert float((e_a0 - ref).abs().max()) <= 1e-5, "the recovered draw is not hdmoe_randn's"
    se = 1.0 / math.sqrt(n)
    for name, e in (("seed A stage i", e_a0), ("seed A stage i+1", e_a1), ("seed B stage i", e_b0), ("hdmoe_randn", ref)):
        mean, var = float(e.mean()), float(e.var(unbiased=False))
        print(f"{name}: mean {mean:+.3e} (bound {6 * se:.3e}), var - 1 {var - 1:+.3e} (bound {6 * math.sqrt(2.0 / n):.3e})")
        assert abs(mean) <= 6 * se, f"{name}: mean {mean:.3e}"
        assert abs(var - 1.0) <= 6 * math.sqrt(2.0 / n), f"{name}: var {var:.6f}"

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return float((a * b).mean() / (a.std(unbiased=False) * b.std(unbiased=False)))

    for name, c in (("stages i, i+1", corr(e_a0, e_a1)), ("two seeds", corr(e_a0, e_b0))):
        print(f"corr {name}: {c:+.3e} (bound {6 * se:.3e})")
        assert abs(c) <= 6 * se, f"corr {name}: {c:.3e}"


# ---- trajectories
def _den64(guide, s_model=0.9, s_gnet=0.5):
    return (lambda x: (s_gnet * x).lerp(s_model * x, guide)) if guide != 1.0 else (lambda x: s_model * x)


def restate(kind, noise, N, guide, strength, seed, x0=None, m=None, s_churn=0.0, s_min=0.0, s_max=float("inf"), s_noise=1.0, eta=1.0):
    """float64 CPU restatement of sample() for kind "churn" (Heun with churn) or "sde"; eps of stage i = contract_eps(.., seed, i)."""
    t = schedule(N)
    i0 = N - math.ceil(strength * N)
    n = noise.numel()
    noise = noise.cpu().double()
    x0 = None if x0 is None else x0.cpu().double()
    m = None if m is None else m.cpu().double()
    den = _den64(guide)
    eps = lambda i: contract_eps(n, seed, i).cpu().double().reshape(noise.shape)      # noqa: E731
    blend = lambda x, s: x if m is None else m * (x0 + s * noise) + (1 - m) * x       # noqa: E731
    x = t[i0] * noise if x0 is None else x0 + t[i0] * noise
    dp = None
    for i in range(i0, N):
        tn = t[i + 1]
        if kind == "sde":
            d = den(x)
            x = blend(sde_update(t, i, i0, x, d, dp, eta, s_noise, eps(i) if eta > 0 and tn > 0 else None), tn)
            dp = d
            continue
        tc = t[i]
        gamma = min(s_churn / N, GAMMA_MAX) if s_churn > 0 and s_min <= float(tc) <= s_max else 0.0
        th = tc + gamma * tc
        xh = x + torch.sqrt(th * th - tc * tc) * s_noise * eps(i) if gamma > 0 else x
        d = den(xh)
        h = tn - th
        xn = blend(xh + h * (xh - d) / th, tn)
        x = xn if i == N - 1 else blend(xh + h * (0.5 * (xh - d) / th + 0.5 * (xn - den(xn)) / tn), tn)
    return x


def _masks(B, H, W, gen):
    binary = (torch.rand(B, 1, H, W, generator=gen, device=DEV) > 0.5).float()
    soft = torch.rand(B, 1, H, W, generator=gen, device=DEV)
    soft[0, 0, :2] = 1.0
    soft[1, 0, -2:] = 0.0
    bcast = torch.zeros(1, 1, H, W, device=DEV)
    bcast[..., : W // 2] = 1.0
    return {"none": None, "binary": binary, "soft": soft, "broadcast": bcast}


def _known_exact(out, x0, mask, msg):
    keep = mask.expand_as(out) == 1
    assert bool(keep.any()) and bool((~keep).any())
    assert torch.equal(out[keep], x0[keep]), f"{msg}: known region is not init_latents bit-for-bit"


CHURN_KW = dict(S_churn=3.0, S_min=0.05, S_max=50.0, S_noise=1.007, churn_on_device=True)
CHURN_REF = dict(s_churn=3.0, s_min=0.05, s_max=50.0, s_noise=1.007)
SDE_NOISE = 1.0 + 2.0 ** -7


def _inputs(B, seed, hw=8):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    noise = torch.randn(B, 4, hw, hw, device=DEV, generator=gen)
    text = torch.randn(B, 5, 16, device=DEV, generator=gen)
    x0 = torch.randn(B, 4, hw, hw, device=DEV, generator=gen)
    return gen, noise, text, x0


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("guide", [1.0, 2.5])
@pytest.mark.parametrize("kind", ["churn", "sde", "sde_half"])
def test_trajectory_matches_restatement(_gpu, kind, use_graph, guide):
    N, B = 6, 3
    gen, noise, text, x0 = _inputs(B, 1)
    m, gnet = mocks()
    if kind == "churn":
        s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=guide, use_graph=use_graph, **CHURN_KW)
        ref_kw = dict(CHURN_REF)
    else:
        eta = 1.0 if kind == "sde" else 0.5
        s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=guide, use_graph=use_graph, solver=SDE, eta=eta, S_noise=SDE_NOISE)
        ref_kw = dict(eta=eta, s_noise=SDE_NOISE)
    for k, (mname, mask) in enumerate(_masks(B, 8, 8, gen).items()):
        for strength in (1.0, 0.6):
            for init in ((None, x0) if strength == 1.0 and mask is None else (x0,)):
                n_run = math.ceil(strength * N)
                seed = SEED_A if k % 2 == 0 else SEED_B + k
                m.calls = gnet.calls = 0
                out = s.sample(noise, text, -1.2, 1.6, init_latents=init, strength=strength, inpaint_mask=mask, seed=seed)
                ref = restate("churn" if kind == "churn" else "sde", noise, N, guide, strength, seed, init, mask, **ref_kw)
                tag = f"{kind} mask={mname} strength={strength} init={init is not None} guide={guide} graph={use_graph}"
                close_scaled(out, ref.float(), 1e-4, msg=tag)
                evals = 2 * n_run - 1 if kind == "churn" else n_run
                if not use_graph:                         # replays do not call the modules
                    assert m.calls == evals, tag
                    assert gnet.calls == (0 if guide == 1.0 else evals), tag
                assert s.fused_heun == (kind == "churn") and s.fused_dpm == (kind != "churn"), tag
                if mask is not None and mname != "soft":
                    _known_exact(out, x0, mask, tag)
    if use_graph:                                             # two graphs for the Heun stage (full, Euler-only), ONE for every DPM stage
        assert len(s._stage["g_heun" if kind == "churn" else "g_dpm"]) == (2 if kind == "churn" else 1)


def _sampler(kind, m, gnet, **kw):
    if kind == "churn":
        return EDM_Sampler(m, gnet, **{**CHURN_KW, **kw})
    return EDM_Sampler(m, gnet, solver=SDE, **kw)


@gpu
@pytest.mark.parametrize("kind", ["churn", "sde"])
def test_seeding_rules_on_one_captured_sampler(_gpu, kind):
    from hdmoe_hip import ops
    N, B = 5, 2
    gen, noise, text, x0 = _inputs(B, 2)
    mask = (torch.rand(B, 1, 8, 8, generator=gen, device=DEV) > 0.5).float()
    kw = dict(init_latents=x0, strength=0.8, inpaint_mask=mask)
    m, gnet = mocks()
    graphed = _sampler(kind, m, gnet, num_solve_steps=N, guidance=2.0, use_graph=True)
    eager = _sampler(kind, m, gnet, num_solve_steps=N, guidance=2.0)
    a1 = graphed.sample(noise, text, -1.2, 1.6, seed=SEED_A, **kw)
    b = graphed.sample(noise, text, -1.2, 1.6, seed=SEED_B, **kw)
    a2 = graphed.sample(noise, text, -1.2, 1.6, seed=SEED_A, **kw)
    assert torch.equal(a1, a2), "the same seed twice differs"
    assert float((a1 - b).abs().max()) > 1e-3, "two seeds give the same output"
    assert torch.equal(a1, eager.sample(noise, text, -1.2, 1.6, seed=SEED_A, **kw)), "graph replay differs from eager (same seed)"
    stage = graphed._stage
    # seed=None: the library's stream, once per call -- reproducible after manual_seed, fresh on every call of ONE capture
    ops.manual_seed(77)
    n1 = graphed.sample(noise, text, -1.2, 1.6, **kw)
    n2 = graphed.sample(noise, text, -1.2, 1.6, **kw)
    ops.manual_seed(77)
    n3 = graphed.sample(noise, text, -1.2, 1.6, **kw)
    ops.manual_seed(77)
    n4 = eager.sample(noise, text, -1.2, 1.6, **kw)
    assert float((n1 - n2).abs().max()) > 1e-3, "two seed=None calls on one captured sampler drew the same noise"
    assert torch.equal(n1, n3) and torch.equal(n1, n4), "seed=None after manual_seed does not reproduce"
    assert graphed._stage is stage, "a seed must not recapture"
    for out in (a1, b, n1, n2):
        _known_exact(out, x0, mask, kind)


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_device_churn_matches_host_loop(_gpu, use_graph):
    """Same seed: the fused churn stage and the host-driven loop (churn_on_device=False) draw the same eps."""
    N, B = 6, 2
    gen, noise, text, x0 = _inputs(B, 3)
    m, gnet = mocks()
    for mname, mask in _masks(B, 8, 8, gen).items():
        kw = dict(init_latents=x0, strength=0.6 if mask is not None else 1.0, inpaint_mask=mask, seed=SEED_B)
        dev_s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.5, use_graph=use_graph, **CHURN_KW)
        host_s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.5, use_graph=use_graph, **{**CHURN_KW, "churn_on_device": False})
        out = dev_s.sample(noise, text, -1.2, 1.6, **kw)
        host = host_s.sample(noise, text, -1.2, 1.6, **kw)
        assert dev_s.fused_heun and not host_s.fused_heun
        close_scaled(out, host, 1e-4, msg=f"device churn vs host loop mask={mname} graph={use_graph}")
        ref = restate("churn", noise, N, 2.5, kw["strength"], SEED_B, x0, mask, **CHURN_REF)
        close_scaled(host, ref.float(), 1e-4, msg=f"host loop vs restatement mask={mname} graph={use_graph}")
        assert torch.equal(host, host_s.sample(noise, text, -1.2, 1.6, **kw)), "the host loop with a seed is not reproducible"


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_eta_zero_is_dpmpp_2m(_gpu, use_graph):
    N, B = 6, 2
    gen, noise, text, x0 = _inputs(B, 4)
    mask = (torch.rand(B, 1, 8, 8, generator=gen, device=DEV) > 0.5).float()
    m, gnet = mocks()
    for kw in ({}, dict(init_latents=x0, strength=0.5, inpaint_mask=mask)):
        a = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.0, use_graph=use_graph, solver=SDE, eta=0.0).sample(
            noise, text, -1.2, 1.6, seed=5, **kw)
        b = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.0, use_graph=use_graph, solver="dpmpp_2m").sample(noise, text, -1.2, 1.6, **kw)
        assert torch.equal(a, b), "eta = 0 differs from solver='dpmpp_2m'"


@gpu
def test_churn_on_device_without_churn_changes_nothing(_gpu):
    N, B = 5, 2
    gen, noise, text, x0 = _inputs(B, 5)
    m, gnet = mocks()
    a = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.0, churn_on_device=True).sample(noise, text, -1.2, 1.6, seed=9)
    b = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.0).sample(noise, text, -1.2, 1.6)
    assert torch.equal(a, b)
    # S_churn > 0 without the flag stays on the host loop
    s = EDM_Sampler(m, gnet, num_solve_steps=N, S_churn=3.0)
    s.sample(noise, text, -1.2, 1.6)
    assert not s.fused_heun and not s.fused_dpm


@gpu
def test_changed_parameters_recapture(_gpu):
    """S_churn / S_noise / eta are baked into a capture as launch scalars: changing one on a captured sampler must recapture."""
    N, B = 5, 2
    gen, noise, text, x0 = _inputs(B, 6)
    m, gnet = mocks()
    g = EDM_Sampler(m, gnet, num_solve_steps=N, use_graph=True, **CHURN_KW)
    first = g.sample(noise, text, -1.2, 1.6, seed=SEED_A)
    for attr, key, val in (("s_churn", "S_churn", 1.5), ("s_noise", "S_noise", 1.1), ("s_max", "S_max", 5.0)):
        setattr(g, attr, val)
        kw = {**CHURN_KW, **{a.replace("s_", "S_"): getattr(g, a) for a in ("s_churn", "s_noise", "s_max")}}
        fresh = EDM_Sampler(m, gnet, num_solve_steps=N, **kw).sample(noise, text, -1.2, 1.6, seed=SEED_A)
        out = g.sample(noise, text, -1.2, 1.6, seed=SEED_A)
        assert torch.equal(out, fresh), f"{key} changed on a captured sampler: stale capture"
        assert float((out - first).abs().max()) > 1e-4, f"{key} has no effect"
        first = out
    g = EDM_Sampler(m, gnet, num_solve_steps=N, use_graph=True, solver=SDE)
    first = g.sample(noise, text, -1.2, 1.6, seed=SEED_A)
    for attr, val in (("eta", 0.5), ("s_noise", 1.25)):
        setattr(g, attr, val)
        fresh = EDM_Sampler(m, gnet, num_solve_steps=N, solver=SDE, eta=g.eta, S_noise=g.s_noise).sample(noise, text, -1.2, 1.6, seed=SEED_A)
        out = g.sample(noise, text, -1.2, 1.6, seed=SEED_A)
        assert torch.equal(out, fresh), f"{attr} changed on a captured sampler: stale capture"
        assert float((out - first).abs().max()) > 1e-4, f"{attr} has no effect"
        first = out


@gpu
@pytest.mark.parametrize("kind", ["churn", "sde"])
def test_bf16_latents_take_the_host_loop(_gpu, kind):
    N, B = 5, 2
    gen, noise, text, x0 = _inputs(B, 7)
    mask = (torch.rand(B, 1, 8, 8, generator=gen, device=DEV) > 0.5).float()
    m, gnet = mocks()
    s = _sampler(kind, m, gnet, num_solve_steps=N, guidance=2.0, dtype=torch.bfloat16)
    for seed in (None, SEED_A):
        for strength in (1.0, 0.4):
            m.calls = 0
            out = s.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=strength, inpaint_mask=mask, seed=seed)
            n_run = math.ceil(strength * N)
            assert not s.fused_heun and not s.fused_dpm and out.dtype == torch.bfloat16
            assert torch.isfinite(out).all()
            assert m.calls == (2 * n_run - 1 if kind == "churn" else n_run)
            _known_exact(out, x0.to(torch.bfloat16), mask, f"bf16 {kind} seed={seed} strength={strength}")
    a = s.sample(noise, text, -1.2, 1.6, seed=SEED_A)
    assert torch.equal(a, s.sample(noise, text, -1.2, 1.6, seed=SEED_A))
    assert float((a.float() - s.sample(noise, text, -1.2, 1.6, seed=SEED_B).float()).abs().max()) > 1e-2


@gpu
def test_sde_host_loop_matches_restatement(_gpu):
    """The extended _dpm_host_loop (bf16 latents) follows the SDE rule within bf16 rounding (the 4e-2 of the dpmpp_2m host-loop test)."""
    N, B = 6, 2
    gen, noise, text, x0 = _inputs(B, 8)
    m, gnet = mocks()
    s = EDM_Sampler(m, gnet, num_solve_steps=N, guidance=2.5, dtype=torch.bfloat16, solver=SDE, eta=0.5)
    out = s.sample(noise, text, -1.2, 1.6, init_latents=x0, strength=0.5, seed=SEED_B)
    ref = restate("sde", noise.bfloat16(), N, 2.5, 0.5, SEED_B, x0.bfloat16(), None, eta=0.5)
    close_scaled(out, ref.float(), 4e-2, msg="bf16 sde host loop")


# ---- real model (config-2 golden weights)
@pytest.fixture(scope="module")
def real_model(_gpu):
    from models import model_config2
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    model = model_config2.preconditioned_HDMOEM(**g["cfg"])
    model.load_state_dict(g["state"])
    model = model.to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(0)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    EDM_Sampler(model, model, num_solve_steps=2).sample(noise, g["text"][:2].to(DEV), -1.2, 1.6)    # registers the weight bank
    return model, g


@gpu
@pytest.mark.parametrize("kind", ["churn", "sde"])
def test_real_model_eager_vs_graph_bit_identical(real_model, kind):
    """Inpainting + strength 0.5 + guidance 2.0 with an unconditional embedding and router masks: eager and replay are one function, and
    the noise of a replay is the noise of the eager run with the same seed."""
    model, g = real_model
    gen = torch.Generator(device=DEV).manual_seed(4)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    x0 = torch.randn(2, 4, 16, 16, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    unc = torch.zeros_like(text)
    mask = torch.zeros(2, 1, 16, 16, device=DEV)
    mask[0, :, :, :8] = 1.0
    mask[1, :, 4:12, 4:12] = 1.0
    um = torch.tensor([1.0, 0.0, 1.0, 1.0], device=DEV)
    kw = dict(init_latents=x0, strength=0.5, inpaint_mask=mask, Unet_router_mask=um)
    mk = lambda **o: _sampler(kind, model, model, num_solve_steps=6, guidance=2.0, **o)        # noqa: E731
    eager_s, graph_s = mk(), mk(use_graph=True)
    eager = eager_s.sample(noise, text, -1.2, 1.6, unc, seed=SEED_A, **kw)
    graphed = graph_s.sample(noise, text, -1.2, 1.6, unc, seed=SEED_A, **kw)
    assert (eager_s.fused_heun and graph_s.fused_heun) if kind == "churn" else (eager_s.fused_dpm and graph_s.fused_dpm)
    assert torch.isfinite(eager).all()
    assert torch.equal(graphed, eager), f"graph replay differs from eager: max {float((graphed - eager).abs().max()):.3e}"
    _known_exact(eager, x0, mask, "eager")
    other = graph_s.sample(noise, text, -1.2, 1.6, unc, seed=SEED_B, **kw)
    assert float((other - eager).abs().max()) > 1e-4                  # the seed is in effect on the replay
    _known_exact(other, x0, mask, "second seed")
    assert torch.equal(graph_s.sample(noise, text, -1.2, 1.6, unc, seed=SEED_A, **kw), eager)
    det = EDM_Sampler(model, model, num_solve_steps=6, guidance=2.0, solver="heun" if kind == "churn" else "dpmpp_2m").sample(
        noise, text, -1.2, 1.6, unc, **kw)
    assert float((det - eager).abs().max()) > 1e-4                    # the noise is in effect
