"""Composed guidance over several prompts, weights and regions: sample() / denoise() keywords compose_text, compose_weights, compose_masks,
model.forward_composed, ops.guide_compose / ops.nhwc_to_nchw_compose and the two entry points behind them (hdmoe_guide_compose,
hdmoe_nhwc_to_nchw_compose).

The oracle is compose64 below, a float64 restatement (per sample n, element (c, p)):
    c_k = a[n, k] m[n, k, p]  (no masks: a[n, k]);   c_0 = 1 - sum_k c_k;   D_c = c_0 D_u + sum_k c_k D_k
followed by combine64 of tests/test_sampler_guide_combine.py on (D_c, D_u).

Tolerances.
  composition alone (w = 1, eta = 1, r = inf, beta = 0, phi = 0: out = D_c).  The kernel makes, per element, in fp32: one rounding per c_k
      (with masks), K roundings in the chain of c_0, K + 1 products and K sums.  With u = 2^-24 the unit roundoff, S = 1 + sum_k |c_k| (it
      bounds |c_0| and every partial difference of its chain) and mag = |c_0| |D_u| + sum_k |c_k| |D_k| (it bounds every partial sum):
        error of c_0           <= K u S + u sum_k |c_k| <= (K + 1) u S               -> (K + 1) u S |D_u| in D_c
        roundings of the c_k   <= u sum_k |c_k| |D_k| <= u mag
        K + 1 products         <= u mag
        K sums                 <= K u mag
      to first order (K + 1) u S |D_u| + (K + 2) u mag; the bound used is that with EPS32 = 2 u in place of u, the factor 2 for the
      higher-order terms.  The egress form adds, for each operand it forms, the existing egress allowance e = 4 EPS32 (|sx x| + |sf F|)
      weighted as the operand enters D_c: |c_0| e_u + sum_k |c_k| e_k.  bf16 outputs: one more rounding, 2^-8 of the magnitude.
  combine on top, two-pass fp32: bit-identical to ops.guide_combine(ref = D_u, d = the D_c read back at w = 1) -- no tolerance.
  combine on top, egress: against combine64 of (the D_c read back at w = 1, D_u in float64 from the values the kernel reads), the
      guide-combine test's bound 8 EPS32 |f| (|a| |D_c| + |b| (|D_c| + |D_u| + |beta| |M_prev|)); D_c has the kernel's own bits, D_u is
      formed in registers within e_u, which enters M and so the output as |f b| e_u, and the scalars to second order: (1 + |f b|) e_u more.
      The written momentum: 3 EPS32 (|D_c| + |D_u| + |beta| |M_prev|) + e_u.
  degenerate case (K = 1, a = 1, no masks): bit-identical to the existing entry points.
  real model, one evaluation: (|g| A + |1 - g|) x 1e-3 (the fp32 single-evaluation bound of tests/test_hip_parity.py) in close_scaled form,
      A = max_p (|c_0| + sum_k |c_k|): the composed output is sum of c's times single evaluations, each within 1e-3 of its oracle value.
  real model, trajectory: 4 x TWO_PASS_ERR_N5 of tests/test_sampler_guidance_interval.py (inputs with A = 1, g = 2.0).
  mock trajectories against their float64 restatement: 1e-4 (the existing sampler tests' bound); replay against eager: torch.equal."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_sampler_guidance_interval as gi  # noqa: E402  (close_scaled, schedule, restate64, TWO_PASS_ERR_N5, the real-model loader)
import test_sampler_guide_combine as gc  # noqa: E402  (combine64, the mock with the combine's shared pass)
from EDM_sampler import EDM_Sampler  # noqa: E402
from hdmoe_hip import ops  # noqa: E402

DEV = "cuda"
gpu = pytest.mark.gpu
EPS32 = 2.0 ** -23
TP, SOFT = gi.TP, gi.SOFT
INF = float("inf")
IDENT = (1.0, 1.0, INF, 0.0, 0.0)                         # w, eta, r, beta, phi: out = D_c
combine64 = gc.combine64


def coef64(a, m, B, K):
    """c_1 .. c_K as (B, K, 1, *spatial) float64 (spatial = () without masks) from the float32 values the kernel reads, and c_0."""
    a = torch.as_tensor(a, dtype=torch.float32).reshape(B, K).double()
    if m is None:
        c = a.view(B, K, 1, 1, 1)
    else:
        c = a.view(B, K, 1, 1, 1) * m.float().double().reshape(B, K, 1, *m.shape[2:])
    return c, 1.0 - c.sum(1)


def compose64(ds, du, a, m, w=1.0, eta=1.0, r=INF, beta=0.0, phi=0.0, mprev=None):
    """float64 restatement: D_c of the K outputs ds (each (B, C, H, W)) and du, then combine64 on (D_c, du).
    Returns out, M, (a, b, f), D_c and the per-element bound of the composition (module docstring) without the egress allowance."""
    B, K = du.shape[0], len(ds)
    du, ds = du.double(), [d.double() for d in ds]
    c, c0 = coef64(a, m, B, K)
    dc = c0 * du
    mag = c0.abs() * du.abs()
    for k in range(K):
        dc = dc + c[:, k] * ds[k]
        mag = mag + c[:, k].abs() * ds[k].abs()
    S = 1.0 + c.abs().sum(1)
    bound = EPS32 * ((K + 1) * S * du.abs() + (K + 2) * mag)
    out, M, abf = combine64(dc, du, w, eta, r, beta, phi, mprev)
    return out, M, abf, dc, bound


def amplification(a, m, B, K):
    """A = max_p (|c_0| + sum_k |c_k|)."""
    c, c0 = coef64(a, m, B, K)
    return float((c0.abs() + c.abs().sum(1)).max())


class _ComposeMock(gc._CombineMock):
    """The closed-form mock D(x; text) = scale slope(text) x + 0.3 mean(text) with the composed shared pass: ops.guide_compose (checked
    against float64 below) on its K + 1 closed-form outputs, plus the marker bias."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.composed = []

    def forward_composed(self, x, sigma, text_embs, uncond_text_emb, weights, masks, guidance, Unet_router_mask, Vit_router_mask, zeta,
                         transition_point, softness, guide_combine=None):
        assert sigma.ndim == 0 and Unet_router_mask.shape == (x.shape[0], self.num_experts) and zeta == 0
        self.composed.append((text_embs.shape[0], masks is not None, guidance if not isinstance(guidance, torch.Tensor) else None))
        eta, r, beta, phi, state = (1.0, INF, 0.0, 0.0, None) if guide_combine is None else guide_combine
        out = ops.guide_compose(self._d(x, uncond_text_emb), [self._d(x, t) for t in text_embs], weights, masks, guidance, eta=eta,
                                norm_threshold=r, momentum=beta, rescale=phi, state=state)
        return {"denoised": out + self.guided_bias}


class _RaisingMock(_ComposeMock):
    """Any model call is a failure of "before any device work"."""

    def forward(self, *a, **k):
        raise RuntimeError("the model was called")

    forward_guided = forward_composed = forward


# ----------------------------------------------------------------------------------------------- 1. argument checks (CPU)
def _bad_compose():
    B, K, H, W = 3, 2, 8, 8
    text = torch.randn(B, 5, 16)
    more = torch.randn(K - 1, B, 5, 16)
    okw, okm = torch.tensor([0.6, 0.4]), torch.rand(K, H, W)
    return text, [
        ("compose_text", dict(compose_text=torch.randn(B, 5, 16))),                              # not stacked
        ("compose_text", dict(compose_text=torch.randn(1, B, 5, 8))),                            # another embedding width
        ("compose_text", dict(compose_text=[more])),
        ("compose_text", dict(compose_text=torch.randn(8, B, 5, 16))),                           # K = 9
        ("compose_text", dict(compose_weights=okw)),                                             # weights without compose_text
        ("compose_text", dict(compose_masks=okm)),                                               # masks without compose_text
        ("compose_weights", dict(compose_text=more, compose_weights=torch.ones(B, 3))),
        ("compose_weights", dict(compose_text=more, compose_weights=torch.ones(K, B))),
        ("compose_weights", dict(compose_text=more, compose_weights=[0.6, 0.4])),
        ("compose_weights", dict(compose_text=more, compose_weights=torch.tensor([0.6, float("nan")]))),
        ("compose_weights", dict(compose_text=more, compose_weights=torch.tensor([[0.6, INF]] * B))),
        ("compose_masks", dict(compose_text=more, compose_masks=torch.rand(K, H, W) + 0.5)),     # above 1
        ("compose_masks", dict(compose_text=more, compose_masks=-torch.rand(B, K, H, W))),       # below 0
        ("compose_masks", dict(compose_text=more, compose_masks=torch.full((K, H, W), float("nan")))),
        ("compose_masks", dict(compose_text=more, compose_masks=torch.rand(K, H, 2 * W))),       # not the latents' H, W
        ("compose_masks", dict(compose_text=more, compose_masks=torch.rand(B, 3, H, W))),
        ("compose_masks", dict(compose_text=more, compose_masks=torch.rand(H, W))),
        ("compose_masks", dict(compose_text=more, compose_masks=torch.ones(K, H, W, dtype=torch.int32))),
    ]


@pytest.mark.parametrize("shared", [False, True])
def test_arguments_are_checked_before_any_device_work(shared):
    """Each failure is a ValueError naming the keyword, from sample() and from denoise(), in front of a model that raises when called."""
    m = _RaisingMock(0.9)
    s = EDM_Sampler(m, m, num_solve_steps=5, guidance=2.0, shared_guidance=shared)
    text, cases = _bad_compose()
    x, unc, sig = torch.randn(3, 4, 8, 8), torch.randn(3, 5, 16), torch.tensor(1.0)
    for name, kw in cases:
        with pytest.raises(ValueError, match=name):
            s.sample(x, text, TP, SOFT, unc, **kw)
        with pytest.raises(ValueError, match=name):
            s.denoise(x, sig, text, TP, SOFT, unc, **kw)
    more = torch.randn(1, 3, 5, 16)
    for bad_unc in (None, torch.randn(3, 5, 8)):
        with pytest.raises(ValueError, match="uncond_text_emb"):
            s.sample(x, text, TP, SOFT, bad_unc, compose_text=more)
        with pytest.raises(ValueError, match="uncond_text_emb"):
            s.denoise(x, sig, text, TP, SOFT, bad_unc, compose_text=more)
    # the rule for K = 1: legal when asked for with an explicit empty compose_text; good arguments get as far as the model
    empty = text.new_empty((0,) + tuple(text.shape))
    for kw in (dict(compose_text=empty, compose_weights=torch.tensor([0.5])), dict(compose_text=empty, compose_masks=torch.rand(1, 8, 8)),
               dict(compose_text=empty), dict(compose_text=more, compose_weights=torch.tensor([0.6, -0.4]), compose_masks=torch.rand(3, 2, 8, 8))):
        with pytest.raises(RuntimeError, match="the model was called"):
            s.denoise(x, sig, text, TP, SOFT, unc, **kw)


def test_shared_composition_needs_forward_composed():
    m = gi._MockDenoiser(0.9)                              # has forward_guided, no forward_composed
    s = EDM_Sampler(m, m, num_solve_steps=5, guidance=2.0, shared_guidance=True)
    with pytest.raises(ValueError, match="forward_composed"):
        s.denoise(torch.randn(3, 4, 8, 8), torch.tensor(1.0), torch.randn(3, 5, 16), TP, SOFT, torch.randn(3, 5, 16),
                  compose_text=torch.randn(1, 3, 5, 16))


def test_entry_points_refuse_bad_arguments():
    """The HDMOE_EINVAL cases of both entry points through the C ABI.  Nothing is launched (and no pointer but the host array d_ptrs is
    read), so placeholder device addresses do."""
    from hdmoe_hip import _lib
    lib = _lib.lib()
    P = lambda v=4096: ctypes.c_void_p(v)                  # noqa: E731
    NULL = None

    def ptrs(n, hole=None):
        arr = (ctypes.c_void_p * max(n, 1))()
        for i in range(n):
            arr[i] = None if i == hole else 4096
        return ctypes.cast(arr, ctypes.c_void_p), arr

    def two_pass(K=2, a=P(), m=NULL, HW=16, d=None, r=INF, beta=0.0, mom=NULL, rows=2, per=64, g=2.0, out=P(), ref=P()):
        dp, keep = d if d is not None else ptrs(min(max(K, 0), 8))
        return lib.hdmoe_guide_compose(out, ref, dp, K, a, m, HW, g, NULL, 1.0, r, beta, 0.0, mom, rows, per, 0, NULL)

    def egress(K=2, a=P(), m=NULL, HW=16, C=4, N=2, r=INF, beta=0.0, mom=NULL, g=2.0, sx=P()):
        return lib.hdmoe_nhwc_to_nchw_compose(P(), P(), P(), P(), sx, K, a, m, g, NULL, 1.0, r, beta, 0.0, mom, N, C, HW, 0, NULL)

    EINVAL = -1
    for fn in (two_pass, egress):
        assert fn(K=0) == EINVAL and fn(K=-1) == EINVAL and fn(K=ops.COMPOSE_MAX + 1) == EINVAL
        assert fn(a=NULL) == EINVAL
        assert fn(r=0.0) == EINVAL and fn(g=float("nan")) == EINVAL and fn(beta=0.5) == EINVAL           # what gc_args_ok refuses
    assert two_pass(d=ptrs(2, hole=1)) == EINVAL and two_pass(d=ptrs(2, hole=0)) == EINVAL and two_pass(K=8, d=ptrs(8, hole=7)) == EINVAL
    assert two_pass(d=(NULL, None)) == EINVAL and two_pass(out=NULL) == EINVAL and two_pass(ref=NULL) == EINVAL
    assert two_pass(m=P(), HW=0) == EINVAL and two_pass(m=P(), HW=-4) == EINVAL and two_pass(m=P(), HW=48) == EINVAL     # 64 % 48 != 0
    assert two_pass(rows=0) == EINVAL and two_pass(per=0) == EINVAL
    assert egress(m=P(), HW=0) == EINVAL and egress(HW=0) == EINVAL and egress(C=0) == EINVAL and egress(N=0) == EINVAL
    assert egress(sx=NULL) == EINVAL
    hdr = open(os.path.join(ROOT, "include", "hdmoe.h")).read()
    assert f"#define HDMOE_COMPOSE_MAX {ops.COMPOSE_MAX}\n" in hdr and ops.COMPOSE_MAX == 8


# ----------------------------------------------------------------------------------------------- 2. the restatement (CPU)
def test_restatement_reduces_to_combine64():
    """K = 1, a = 1, no masks: compose64 is combine64 exactly (c_0 = 0, D_c = D_1); with sum_k c_k = 1 the result does not depend on D_u
    at w = 1 to float64 rounding (c_0 = 0 up to the rounding of the sum)."""
    gen = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)        # noqa: E731
    d1, du, mp = 0.5 * rn(3, 4, 8, 8) + 0.05, 0.5 * rn(3, 4, 8, 8), 0.1 * rn(3, 4, 8, 8)
    for par in ((7.5, 0.0, 2.5, -0.5, 0.7), (2.0, 1.0, INF, 0.0, 0.0), ((0.0, 1.0, 7.5), 0.25, 15.0, -0.75, 1.0)):
        out, M, abf, dc, _ = compose64([d1], du, torch.ones(3, 1), None, *par, mprev=mp)
        ref, Mr, abfr = combine64(d1, du, *par, mp)
        assert torch.equal(dc, d1) and torch.equal(out, ref) and torch.equal(M, Mr) and all(torch.equal(p, q) for p, q in zip(abf, abfr))
    # sum_k c_k = 1: weights (0.5, 0.25, 0.25) without masks (exact in float32, as the kernel reads them), and a partition of the
    # positions by masks with unit weights
    ds = [0.5 * rn(3, 4, 8, 8) for _ in range(3)]
    part = torch.zeros(3, 3, 8, 8)
    part[:, 0, :, :3], part[:, 1, :, 3:5], part[:, 2, :, 5:] = 1.0, 1.0, 1.0
    for a, m in ((torch.tensor([[0.5, 0.25, 0.25]] * 3), None), (torch.ones(3, 3), part)):
        o1, _, _, dc1, _ = compose64(ds, du, a, m)
        o2, _, _, dc2, _ = compose64(ds, 100.0 * rn(3, 4, 8, 8), a, m)
        assert torch.equal(o1, dc1)                                             # w = 1 with the identity scalars: out = D_c
        assert float((dc1 - dc2).abs().max()) <= 400.0 * 2.0 ** -50, float((dc1 - dc2).abs().max())
    assert amplification(torch.tensor([[0.6, 0.4]]), torch.stack([torch.ones(1, 4, 4), torch.zeros(1, 4, 4)], 1), 1, 2) == pytest.approx(1.0)


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


# ---- 3. the kernels against float64
# N, C, H, W, K, masks: the smallest shapes that reach each arm (the issue's table)
KERNEL_CASES = {
    "1x3x1x5_element": (1, 3, 1, 5, 1, False),
    "3x4x4x4_vector_resident": (3, 4, 4, 4, 3, True),
    "2x4x72x72_reread": (2, 4, 72, 72, 2, True),
    "2x4x3x6_mask_forced_element": (2, 4, 3, 6, 2, True),
}
assert 4 * 72 * 72 > ops.GUIDE_COMBINE_RESIDENT and (3 * 6) % 4 != 0
COMBINE_PARAMS = [((2.5, -0.5, 7.5), 0.25, 2.5, -0.5, 0.7), (4.0, 0.5, 15.0, 0.0, 1.0)]


def _case(name, seed=5):
    """Operands of one kernel case, all float32 on the GPU: du, ds, the weights (a negative one, a zero, a row summing to 1), the masks
    (fractional, with an all-zero and an all-one plane), the previous momentum."""
    N, C, H, W, K, masked = KERNEL_CASES[name]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=gen)           # noqa: E731
    du = 0.5 * rn(N, C, H, W) + 0.05
    ds = [du + 0.2 * rn(N, C, H, W) for _ in range(K)]
    rows = {1: [[0.7]], 2: [[1.25, -0.25], [0.0, 0.8]], 3: [[0.5, 0.3, 0.2], [1.2, -0.5, 0.0], [0.7, 0.0, -0.3]]}[K]
    a = torch.tensor(rows[:N], device=DEV)
    m = None
    if masked:
        m = torch.rand(N, K, H, W, device=DEV, generator=gen)
        m[0, 0] = 0.0
        m[-1, -1] = 1.0
    mp = 0.1 * rn(N, C, H, W)
    return N, C, H, W, K, du, ds, a, m, mp


def _egress_from(du, ds, seed):
    """F (variant-stacked NHWC float32), sf, x, sx whose formed operands follow ds / du, those operands in float64 from the values the
    kernel reads, and the egress allowance e = 4 EPS32 (|sx x| + |sf F|) of each."""
    N = du.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(du.shape, device=DEV, generator=gen)
    sf = torch.rand(N, device=DEV, generator=gen) + 0.5
    sx = 0.5 * (torch.rand(N, device=DEV, generator=gen) - 0.5)
    col = lambda v: v.view(-1, 1, 1, 1)                                # noqa: E731
    F = torch.cat([(d - col(sx) * x) / col(sf) for d in ds + [du]]).permute(0, 2, 3, 1).contiguous()
    sxx = (col(sx).double() * x.double()).cpu()
    ops64, allow = [], []
    for v in range(len(ds) + 1):
        sff = col(sf).double().cpu() * F[v * N:(v + 1) * N].double().permute(0, 3, 1, 2).cpu()
        ops64.append(sxx + sff)
        allow.append(4 * EPS32 * (sxx.abs() + sff.abs()))
    return F, sf, x, sx, ops64[:-1], ops64[-1], allow[:-1], allow[-1]


GUARD = -777.0


def _guarded(rows, per):
    big = torch.full((rows + 2, per), GUARD, device=DEV)
    return big, big[1:-1]


def _launch(form, case, par, dtype=torch.float32, eg=None, with_mom=True):
    """One launch of the entry point itself with guard rows around out, the momentum and the masks; returns out (N, C, H, W) and the
    written momentum (None when beta == 0)."""
    N, C, H, W, K, du, ds, a, m, mp = case
    w, eta, r, beta, phi = par
    per = C * H * W
    g_rows = torch.tensor(w, device=DEV) if isinstance(w, tuple) else None
    gbig, out = _guarded(N, per)
    mbig, mom = _guarded(N, per)
    mom.copy_(mp.reshape(N, per))
    kbig = mk = None
    if m is not None:
        kbig = torch.full((N + 2, K * H * W), GUARD, device=DEV)
        mk = kbig[1:-1]
        mk.copy_(m.reshape(N, -1))
    use_mom = mom if (beta != 0.0 and with_mom) else None
    if form == "two_pass":
        obig = torch.full((N + 2, per), GUARD, device=DEV, dtype=dtype)
        out = obig[1:-1]
        ops.call("hdmoe_guide_compose", out, du.to(dtype), [d.to(dtype) for d in ds], K, a, mk, H * W, 0.0 if g_rows is not None else w,
                 g_rows, eta, r, beta, phi, use_mom, N, per, 0 if dtype == torch.float32 else 1)
        gbig = obig
    else:
        F, sf, x, sx = eg[:4]
        ops.call("hdmoe_nhwc_to_nchw_compose", out, F, sf, x, sx, K, a, mk, 0.0 if g_rows is not None else w, g_rows, eta, r, beta, phi,
                 use_mom, N, C, H * W, 0)
    torch.cuda.synchronize()
    assert bool((gbig[0] == GUARD).all()) and bool((gbig[-1] == GUARD).all()), f"{form}: wrote outside out"
    assert bool((mbig[0] == GUARD).all()) and bool((mbig[-1] == GUARD).all()), f"{form}: wrote outside the momentum"
    if use_mom is None:
        assert torch.equal(mom, mp.reshape(N, per)), f"{form}: beta = 0 touched the momentum buffer"
    if kbig is not None:
        assert bool((kbig[0] == GUARD).all()) and bool((kbig[-1] == GUARD).all()) and torch.equal(mk, m.reshape(N, -1)), f"{form}: masks changed"
    return out.reshape(N, C, H, W).clone(), (mom.reshape(N, C, H, W).clone() if use_mom is not None else None)


def _within(tag, got, ref, bound):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite output"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{tag}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), f"{tag}: max err / bound = {ratio:.3f}"


@gpu
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_two_pass_compose_matches_float64(_gpu, name):
    """hdmoe_guide_compose, fp32 and bf16: the composition alone against compose64; the combine on top (fp32) bit-identical to
    ops.guide_combine on (D_u, the D_c read back), output and momentum; the guards intact."""
    case = _case(name)
    N, C, H, W, K, du, ds, a, m, mp = case
    cpu = lambda t: None if t is None else t.double().cpu()                # noqa: E731
    # The bit-identity needs both kernels on the same arm (another arm sums in another order).  The masks force 2x4x3x6 onto the element
    # arm although per % 4 == 0: there guide_combine gets D_u at an address that is no multiple of 16 bytes, its own way onto that arm.
    du_same_arm = du
    if (H * W) % 4 != 0 and (C * H * W) % 4 == 0:
        du_same_arm = torch.empty(du.numel() + 1, device=DEV)[1:].view_as(du).copy_(du)
        assert du_same_arm.data_ptr() % 16 != 0 and du_same_arm.is_contiguous()
    for dtype in (torch.float32, torch.bfloat16):
        du_t, ds_t = du.to(dtype), [d.to(dtype) for d in ds]
        dc_rb, none = _launch("two_pass", case, IDENT, dtype)
        assert none is None and dc_rb.dtype == dtype
        _, _, _, dc64, bound = compose64([cpu(d) for d in ds_t], cpu(du_t), a.cpu(), cpu(m))
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * (dc64.abs() + bound)
        _within(f"two-pass {name} {dtype}: composition alone", dc_rb, dc64, bound)
        via_ops = ops.guide_compose(du_t, ds_t, a, m, 1.0)
        assert torch.equal(via_ops, dc_rb), "ops.guide_compose differs from the entry point"
        if dtype != torch.float32:
            continue
        for par in COMBINE_PARAMS:
            w, eta, r, beta, phi = par
            if isinstance(w, tuple):
                w = w[:N]
            out, mom = _launch("two_pass", case, (w, eta, r, beta, phi))
            state = mp.clone()
            ref = ops.guide_combine(du_same_arm, dc_rb, torch.tensor(w, device=DEV) if isinstance(w, tuple) else w, eta=eta, norm_threshold=r,
                                    momentum=beta, rescale=phi, state=state if beta else None)
            assert torch.equal(out, ref), f"{name} {par}: not the bits of guide_combine(D_u, D_c), max diff {float((out - ref).abs().max()):.3e}"
            assert (mom is None) == (beta == 0.0) and (mom is None or torch.equal(mom, state))
            assert float((out - dc_rb).abs().max()) > 1e-3


@gpu
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_egress_compose_matches_float64(_gpu, name):
    """hdmoe_nhwc_to_nchw_compose on a float32 F: the composition alone against compose64 of the operands it forms; the combine on top
    against combine64 within the guide-combine bound plus the egress allowance; the guards intact."""
    case = _case(name, seed=9)
    N, C, H, W, K, du, ds, a, m, mp = case
    eg = _egress_from(du, ds, 17)
    F, sf, x, sx, ds64, du64, e_k, e_u = eg
    cpu = lambda t: None if t is None else t.double().cpu()                # noqa: E731
    dc_rb, _ = _launch("egress", case, IDENT, eg=eg)
    _, _, _, dc64, bound = compose64(ds64, du64, a.cpu(), cpu(m))
    c, c0 = coef64(a.cpu(), cpu(m), N, K)
    bound = bound + c0.abs() * e_u + sum(c[:, k].abs() * e_k[k] for k in range(K))
    _within(f"egress {name}: composition alone", dc_rb, dc64, bound)
    assert torch.equal(ops.nhwc_to_nchw_compose(F, sf, x, sx, K, a, m, 1.0), dc_rb), "ops.nhwc_to_nchw_compose differs from the entry point"
    for par in COMBINE_PARAMS:
        w, eta, r, beta, phi = par
        if isinstance(w, tuple):
            w = w[:N]
        out, mom = _launch("egress", case, (w, eta, r, beta, phi), eg=eg)
        ref, M64, (a_, b_, f_) = combine64(cpu(dc_rb), du64, w, eta, r, beta, phi, cpu(mp))
        mag = cpu(dc_rb).abs() + du64.abs() + abs(gc.f32(beta)) * cpu(mp).abs()
        bnd = 8 * EPS32 * f_.abs() * (a_.abs() * cpu(dc_rb).abs() + b_.abs() * mag) + (1.0 + (f_ * b_).abs()) * e_u
        _within(f"egress {name} {par}: combine on top", out, ref, bnd)
        if mom is not None:
            _within(f"egress {name} {par}: momentum", mom, M64, 3 * EPS32 * mag + e_u)


@gpu
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_degenerate_case_is_bit_identical(_gpu, name):
    """K = 1, a = 1, no masks: the bits of hdmoe_guide_combine / hdmoe_nhwc_to_nchw_guide_combine with the same launch scalars, output and
    momentum, fp32 and (two-pass) bf16."""
    N, C, H, W, _, du, ds, _, _, mp = _case(name, seed=13)
    d1 = ds[0]
    ones = torch.ones(N, 1, device=DEV)
    for w, eta, r, beta, phi in COMBINE_PARAMS + [IDENT]:
        g = torch.tensor(w[:N], device=DEV) if isinstance(w, tuple) else w
        kw = dict(eta=eta, norm_threshold=r, momentum=beta, rescale=phi)
        for dtype in (torch.float32, torch.bfloat16):
            s1, s2 = mp.clone(), mp.clone()
            got = ops.guide_compose(du.to(dtype), [d1.to(dtype)], ones, None, g, state=s1 if beta else None, **kw)
            ref = ops.guide_combine(du.to(dtype), d1.to(dtype), g, state=s2 if beta else None, **kw)
            assert torch.equal(got, ref) and torch.equal(s1, s2), f"two-pass {name} {dtype} {(w, eta, r, beta, phi)}"
        F, sf, x, sx = _egress_from(du, [d1], 19)[:4]
        s1, s2 = mp.clone(), mp.clone()
        got = ops.nhwc_to_nchw_compose(F, sf, x, sx, 1, ones, None, g, state=s1 if beta else None, **kw)
        ref = ops.nhwc_to_nchw_guide_combine(F, sf, x, sx, g, state=s2 if beta else None, **kw)
        assert torch.equal(got, ref) and torch.equal(s1, s2), f"egress {name} {(w, eta, r, beta, phi)}"


@gpu
def test_bindings_validate_on_the_host(_gpu):
    N, C, H, W, K, du, ds, a, m, mp = _case("3x4x4x4_vector_resident")
    with pytest.raises(ValueError, match="guide_compose"):
        ops.guide_compose(du, [ds[0][:, :-1]] + ds[1:], a, m, 2.0)
    with pytest.raises(ValueError, match="weights"):
        ops.guide_compose(du, ds, a[:, :2], m, 2.0)
    with pytest.raises(ValueError, match="weights"):
        ops.guide_compose(du, ds, a.double(), m, 2.0)
    with pytest.raises(ValueError, match="masks"):
        ops.guide_compose(du, ds, a, m[:, :, :2], 2.0)
    with pytest.raises(ValueError, match="conditions"):
        ops.guide_compose(du, ds * 3, a.repeat(1, 3), None, 2.0)
    with pytest.raises(ValueError, match="state"):
        ops.guide_compose(du, ds, a, m, 2.0, eta=0.5, momentum=-0.5)
    F, sf, x, sx = _egress_from(du, ds, 21)[:4]
    with pytest.raises(ValueError, match="stacked"):
        ops.nhwc_to_nchw_compose(F, sf, x, sx, K - 1, a[:, :K - 1], None, 2.0)
    with pytest.raises(ValueError, match="masks"):
        ops.nhwc_to_nchw_compose(F, sf, x, sx, K, a, m.reshape(N, K, H * W), 2.0)


# ---- 4. the sampler on the closed-form mock
def composed64(texts, unc, a, m, g, interval, kw, scale=0.9, bias=0.0, log=None):
    """The mock's composed denoiser in float64: D_c of the K closed-form outputs; a guided evaluation (sigma in the interval) applies the
    combine with the scale and carries the momentum, the others return D_c (scale 1, identity scalars) and leave it alone."""
    t64, u64 = [t.cpu().double() for t in texts], unc.cpu().double()
    d64 = lambda x, tx: (scale * gc._slope(tx)) * x + 0.3 * tx.mean(dim=(1, 2)).view(-1, 1, 1, 1)          # noqa: E731
    eta = 1.0 if kw.get("apg_eta") is None else kw["apg_eta"]
    r, beta, phi = kw.get("apg_norm_threshold", INF), kw.get("apg_momentum", 0.0), kw.get("guidance_rescale", 0.0)
    a, m = a.cpu(), None if m is None else m.cpu()
    state = {}

    def den(x, t):
        ds, du = [d64(x, tx) for tx in t64], d64(x, u64)
        B = x.shape[0]
        aa = a.expand(B, len(ds))
        mm = None if m is None else m.expand(B, len(ds), *m.shape[-2:])
        if interval is None or interval[0] <= float(t) <= interval[1]:
            out, M, _, _, _ = compose64(ds, du, aa, mm, g, eta, r, beta, phi, state.get("M", torch.zeros_like(x)))
            state["M"] = M
            if log is not None:
                log.append(float(t))
            return out + bias
        return compose64(ds, du, aa, mm)[3] + bias
    return den


def _mock_compose_inputs(seed, K, masks=True):
    noise, text, unc = gi.mock_inputs(seed)
    gen = torch.Generator(device=DEV).manual_seed(seed + 1000)
    more = torch.randn(K - 1, *text.shape, device=DEV, generator=gen)
    a = (torch.rand(3, K, device=DEV, generator=gen) * 1.5 - 0.25)
    m = torch.rand(3, K, 8, 8, device=DEV, generator=gen) if masks else None
    return noise, text, unc, more, a, m


MOCK_CASES = {
    "interval": (dict(guidance_interval=(1.0, 20.0)), {}),
    "apg_momentum": (dict(guidance_rescale=0.7, apg_eta=0.25, apg_norm_threshold=0.5, apg_momentum=-0.5), {}),
    "per_sample_vector": (dict(guidance_rescale=0.5), dict(guidance=[4.0, 0.0, 2.5])),
    "dpmpp_2m": (dict(solver="dpmpp_2m", apg_eta=0.5, apg_momentum=0.25, guidance_interval=(0.1, 30.0)), {}),
}


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", list(MOCK_CASES))
def test_mock_trajectory_matches_restatement(_gpu, case, use_graph, shared):
    """K = 3 with masks and a negative weight, N = 5, guidance 3: the guidance interval, APG with momentum, a per-sample guidance vector
    and DPM-Solver++(2M), each against the float64 restatement, eagerly and replayed, in both modes."""
    N, guide, K = 5, 3.0, 3
    skw, ckw = MOCK_CASES[case]
    noise, text, unc, more, a, m = _mock_compose_inputs(31, K)
    a[:, 1] = -a[:, 1].abs()
    bias = 0.25 if shared else 0.0
    mock = _ComposeMock(0.9, guided_bias=bias).to(DEV)
    s = EDM_Sampler(mock, mock, num_solve_steps=N, guidance=guide, use_graph=use_graph, shared_guidance=shared, **skw)
    gvec = ckw.get("guidance")
    out = s.sample(noise, text, TP, SOFT, unc, compose_text=more, compose_weights=a, compose_masks=m,
                   **({} if gvec is None else dict(guidance=torch.tensor(gvec))))
    seen = []
    den = composed64([text, *more], unc, a, m, guide if gvec is None else gvec, skw.get("guidance_interval"), skw, bias=bias, log=seen)
    kind = "dpm" if skw.get("solver") else "heun"
    ref = gi.restate64(kind, den, noise, N)
    gi.close_scaled(out, ref.float(), 1e-4, msg=f"{case} graph={use_graph} shared={shared}: vs the float64 restatement")
    assert s.fused_heun or s.fused_dpm
    assert s.last_evaluations["guided"] == len(seen) and s.last_evaluations["plain"] == (N if kind == "dpm" else 2 * N - 1) - len(seen)
    if shared:
        assert mock.calls == 0 and all(k == K and has for k, has, _ in mock.composed) and not mock.guided
    else:
        assert not mock.composed
    single = EDM_Sampler(mock, mock, num_solve_steps=N, guidance=guide, shared_guidance=shared, **skw).sample(
        noise, text, TP, SOFT, unc, **({} if gvec is None else dict(guidance=torch.tensor(gvec))))
    assert float((single - out).abs().max()) > 1e-2, "the composition changes nothing on this case"


def _dpm_restate64(den, noise, N, t, x_start=None, known=None, sde=None):
    """DPM-Solver++(2M) (SDE: eta, S_noise = 1 and the stage draws eps[i]) in float64 with the inpainting blend after each update."""
    x = t[0] * noise.cpu().double() if x_start is None else x_start
    dp = None
    for i in range(N):
        d = den(x, t[i])
        tc, tn = float(t[i]), float(t[i + 1])
        e = math.exp(-sde[0] * math.log(tc / tn)) if sde is not None and tn > 0 else 1.0
        al = tn / tc * e
        if tn == 0:
            x = d.clone()
        elif i == 0:
            x = al * x + (1 - al) * d
        else:
            hr = 0.5 * math.log(tc / tn) / math.log(float(t[i - 1]) / tc)
            x = al * x + (1 - al) * ((1 + hr) * d - hr * dp)
        if sde is not None and sde[0] > 0 and tn > 0:
            x = x + tn * math.sqrt(1.0 - e * e) * sde[1][i]
        if known is not None:
            x0, nz, mk = known
            x = mk * (x0 + tn * nz) + (1 - mk) * x
        dp = d
    return x


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("case", ["dpmpp_2m_sde", "inpainting"])
def test_mock_sde_and_inpainting(_gpu, case, shared):
    """The 2M SDE under a seed and inpainting (DPM-Solver++(2M), strength 1) with composition, against the float64 restatement that draws
    the same eps / applies the same blend; the replay is the eager run."""
    N, guide, K = 5, 3.0, 2
    noise, text, unc, more, a, m = _mock_compose_inputs(41, K)
    bias = 0.25 if shared else 0.0
    mock = _ComposeMock(0.9, guided_bias=bias).to(DEV)
    den = composed64([text, *more], unc, a, m, guide, None, {}, bias=bias)
    t = gi.schedule(N)
    comp = dict(compose_text=more, compose_weights=a, compose_masks=m)
    if case == "dpmpp_2m_sde":
        skw, kw = dict(solver="dpmpp_2m_sde", eta=0.5), dict(seed=12345)
        eps = [ops.randn_keyed(noise, 12345, i).double().cpu() for i in range(N)]
        ref = _dpm_restate64(den, noise, N, t, sde=(0.5, eps))
    else:
        x0 = gi.mock_inputs(42)[0]
        mask = torch.zeros(3, 1, 8, 8, device=DEV)
        mask[..., :4] = 1.0
        skw, kw = dict(solver="dpmpp_2m"), dict(init_latents=x0, inpaint_mask=mask)
        ref = _dpm_restate64(den, noise, N, t, x_start=x0.cpu().double() + t[0] * noise.cpu().double(),
                             known=(x0.cpu().double(), noise.cpu().double(), mask.cpu().double()))
    mk = lambda **o: EDM_Sampler(mock, mock, num_solve_steps=N, guidance=guide, shared_guidance=shared, **skw, **o)    # noqa: E731
    eager = mk().sample(noise, text, TP, SOFT, unc, **comp, **kw)
    gi.close_scaled(eager, ref.float(), 1e-4, msg=f"{case} shared={shared}: vs the float64 restatement")
    assert torch.equal(mk(use_graph=True).sample(noise, text, TP, SOFT, unc, **comp, **kw), eager)
    if case == "inpainting":
        assert torch.equal(eager[..., :4], kw["init_latents"][..., :4])


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_replay_equals_eager_and_reuses_the_capture(_gpu, solver, shared):
    """Eager equals graph replay (torch.equal).  Other weights, masks and extra text of the same K replay the same capture, the result is
    a fresh sampler's; another K, or dropping the masks, recaptures."""
    N, K = 6, 3
    noise, text, unc, more, a, m = _mock_compose_inputs(51, K)
    _, text2, unc2, more2, a2, m2 = _mock_compose_inputs(52, K)
    mock = _ComposeMock(0.9, guided_bias=0.25).to(DEV)
    kw = dict(num_solve_steps=N, guidance=2.5, solver=solver, shared_guidance=shared, guidance_interval=(0.5, 10.0), apg_eta=0.25,
              apg_momentum=-0.5, guidance_rescale=0.7)
    graphed = EDM_Sampler(mock, mock, use_graph=True, **kw)
    fresh = lambda tx, uc, **c: EDM_Sampler(mock, mock, **kw).sample(noise, tx, TP, SOFT, uc, **c)     # noqa: E731
    c1 = dict(compose_text=more, compose_weights=a, compose_masks=m)
    c2 = dict(compose_text=more2, compose_weights=a2[0].cpu(), compose_masks=m2[0])                # (K,) and (K, H, W) forms, other devices
    first = graphed.sample(noise, text, TP, SOFT, unc, **c1)
    assert torch.equal(first, fresh(text, unc, **c1))
    stage = graphed._stage
    name = "g_heun" if solver == "heun" else "g_dpm"
    graphs = list(stage[name])
    assert stage["key"][1] == (K, True) and stage["texts"].shape[0] == K
    second = graphed.sample(noise, text2, TP, SOFT, unc2, **c2)
    assert graphed._stage is stage and all(p is q for p, q in zip(stage[name], graphs)) and len(stage[name]) == len(graphs)
    assert torch.equal(second, fresh(text2, unc2, **c2)) and float((second - first).abs().max()) > 1e-3
    assert torch.equal(graphed.sample(noise, text, TP, SOFT, unc, **c1), first)
    graphed.sample(noise, text, TP, SOFT, unc, compose_text=more, compose_weights=a)               # no masks: another capture
    assert graphed._stage is not stage and graphed._stage["key"][1] == (K, False)
    stage = graphed._stage
    graphed.sample(noise, text, TP, SOFT, unc, compose_text=more[:1], compose_weights=a[:, :2])    # K = 2
    assert graphed._stage is not stage and graphed._stage["key"][1] == (2, False)


@gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_host_loop_with_bf16_latents(_gpu, use_graph):
    """bf16 latents take the host loops: the two-pass composition is the bf16 arm of hdmoe_guide_compose; the captured evaluation replays
    the eager run."""
    noise, text, unc, more, a, m = _mock_compose_inputs(61, 2)
    mock = _ComposeMock(0.9).to(DEV)
    kw = dict(num_solve_steps=5, guidance=3.0, dtype=torch.bfloat16, solver="dpmpp_2m", guidance_interval=(1.0, 20.0), guidance_rescale=0.5)
    comp = dict(compose_text=more, compose_weights=a, compose_masks=m)
    s = EDM_Sampler(mock, mock, use_graph=use_graph, **kw)
    out = s.sample(noise, text, TP, SOFT, unc, **comp)
    assert out.dtype == torch.bfloat16 and not (s.fused_heun or s.fused_dpm) and torch.isfinite(out.float()).all()
    if use_graph:
        assert torch.equal(out, EDM_Sampler(mock, mock, **kw).sample(noise, text, TP, SOFT, unc, **comp))
    single = EDM_Sampler(mock, mock, **kw).sample(noise, text, TP, SOFT, unc)
    assert float((out.float() - single.float()).abs().max()) > 1e-2


# ---- 5. the real model (config-2 golden weights): B = 2, 4x16x16, fp32 compute mode
real_model = gi.real_model


def _real_compose_inputs(g, K, seed):
    """x, the K conditions, the unconditional embedding (all on the GPU), weights and masks on the host."""
    x, text, unc = gi._real_inputs(g, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    texts = [text, g["text"][2:4].to(DEV)] + [torch.randn(text.shape, generator=gen).to(DEV) for _ in range(K - 2)]
    left = torch.zeros(16, 16)
    left[:, :8] = 1.0
    if K == 2:                                             # left / right halves, weights (0.6, 0.4): A = 1
        a, m = torch.tensor([0.6, 0.4]), torch.stack([left, 1.0 - left])
    else:                                                  # K = 3, one negative weight
        a, m = torch.tensor([0.8, 0.5, -0.4]), torch.stack([left, 1.0 - left, torch.rand(16, 16, generator=gen)])
    return x, texts, unc, a, m


@gpu
@pytest.mark.parametrize("K", [2, 3])
def test_one_composed_evaluation_matches_oracle(real_model, K):
    """forward_composed (through denoise) against the CPU oracle's K + 1 single evaluations composed in float64, within
    (|g| A + |1 - g|) x 1e-3; the two-pass path within the same bound of the oracle and of the shared pass."""
    from oracle import hdmoe_oracle as O
    model, g = real_model
    guide = 2.0
    x, texts, unc, a, m = _real_compose_inputs(g, K, 71)
    sig = torch.tensor(1.3, device=DEV)
    ones = torch.ones(2, g["cfg"]["num_experts"])
    with torch.no_grad():
        outs = [O.preconditioned_hdmoem(g["state"], g["cfg"], 2, x.cpu(), sig.cpu(), tx.cpu(), ones, ones, transition_point=TP,
                                        softness=SOFT)["denoised"] for tx in texts + [unc]]
    B = x.shape[0]
    ref = compose64(outs[:-1], outs[-1], a.expand(B, K), m.expand(B, K, 16, 16), guide)[0]
    A = amplification(a.expand(B, K), m.expand(B, K, 16, 16), B, K)
    assert (K != 2) or A == pytest.approx(1.0, abs=1e-6)
    rel = (abs(guide) * A + abs(1.0 - guide)) * 1e-3
    comp = dict(compose_text=torch.stack(texts[1:]), compose_weights=a, compose_masks=m)
    res = {}
    with torch.no_grad():
        for shared in (True, False):
            res[shared] = EDM_Sampler(model, model, num_solve_steps=4, guidance=guide, shared_guidance=shared).denoise(
                x, sig, texts[0], TP, SOFT, unc, **comp)
            gi.close_scaled(res[shared], ref.float(), rel, msg=f"K={K} A={A:.2f} shared={shared}: composed evaluation vs the oracle")
        single = EDM_Sampler(model, model, num_solve_steps=4, guidance=guide).denoise(x, sig, texts[0], TP, SOFT, unc)
    gi.close_scaled(res[True], res[False], rel, msg=f"K={K}: shared vs two-pass")
    assert float((res[True] - single).abs().max()) > 1e-3 * float(single.abs().max()), "the composition changes nothing on this input"


@gpu
def test_launch_counts_of_one_composed_evaluation(real_model):
    """The shared pass of K = 3: the ingress (stem input), each router head and each dispatch plan once, the composed egress once and
    last, the paired gathers of one shared pass; the two-pass form makes K + 1 of each and one hdmoe_guide_compose."""
    from hdmoe_hip import _lib
    model, g = real_model
    K = 3
    x, texts, unc, a, m = _real_compose_inputs(g, K, 73)
    sig = torch.tensor(1.3, device=DEV)
    comp = dict(compose_text=torch.stack(texts[1:]), compose_weights=a, compose_masks=m)
    names = ("hdmoe_nchw_to_nhwc", "hdmoe_router_head_fwd", "hdmoe_dispatch_plan", "hdmoe_nhwc_to_nchw_compose", "hdmoe_guide_compose",
             "hdmoe_nhwc_to_nchw", "hdmoe_gather_rows_paired")
    counts = {}
    for mode in ("shared", "two_pass", "plain"):
        s = EDM_Sampler(model, model, num_solve_steps=4, guidance=1.0 if mode == "plain" else 2.0, shared_guidance=mode == "shared")
        kw = {} if mode == "plain" else comp
        with torch.no_grad():
            s.denoise(x, sig, texts[0], TP, SOFT, unc, **kw)               # warm: nothing one-off in the log
            _lib.CALL_LOG = []
            try:
                s.denoise(x, sig, texts[0], TP, SOFT, unc, **kw)
                log = [n for n, _ in _lib.CALL_LOG]
            finally:
                _lib.CALL_LOG = None
        counts[mode] = dict({n: log.count(n) for n in names}, total=len(log), last=log[-1])
    print(counts)
    sh, tp, one = counts["shared"], counts["two_pass"], counts["plain"]
    for n in ("hdmoe_nchw_to_nhwc", "hdmoe_router_head_fwd", "hdmoe_dispatch_plan"):
        assert sh[n] == one[n] and tp[n] == (K + 1) * one[n], n
    assert one["hdmoe_router_head_fwd"] == 2 and one["hdmoe_dispatch_plan"] == 2
    assert sh["hdmoe_nhwc_to_nchw_compose"] == 1 and sh["last"] == "hdmoe_nhwc_to_nchw_compose" and sh["hdmoe_nhwc_to_nchw"] == 0
    assert sh["hdmoe_guide_compose"] == 0 and sh["hdmoe_gather_rows_paired"] == 4
    assert tp["hdmoe_guide_compose"] == 1 and tp["last"] == "hdmoe_guide_compose" and tp["hdmoe_nhwc_to_nchw"] == K + 1
    assert tp["hdmoe_nhwc_to_nchw_compose"] == 0 and sh["total"] < tp["total"]


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_real_model_trajectory(real_model, solver, shared):
    """N = 5, g = 2.0, K = 2 with the half masks (A = 1): against the same run with the composition and the blend applied in float64 to
    the two-pass outputs of each evaluation, within 4 x TWO_PASS_ERR_N5."""
    model, g = real_model
    N, B, guide, K = 5, 2, 2.0, 2
    _, texts, unc, a, m = _real_compose_inputs(g, K, 75)
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(gi.TRAJ_SEED))
    ones = torch.ones(B, g["cfg"]["num_experts"], device=DEV)

    def den(x, t):
        kw = dict(x=x.float().to(DEV), sigma=t.float().to(DEV), Unet_router_mask=ones, Vit_router_mask=ones, zeta=0, transition_point=TP,
                  softness=SOFT)
        with torch.no_grad():
            outs = [model(text_emb=tx, **kw)["denoised"].double().cpu() for tx in texts + [unc]]
        return compose64(outs[:-1], outs[-1], a.expand(B, K), m.expand(B, K, 16, 16), guide)[0]

    ref = gi.restate64("heun" if solver == "heun" else "dpm", den, noise, N)
    run = lambda **c: EDM_Sampler(model, model, num_solve_steps=N, guidance=guide, solver=solver, shared_guidance=shared).sample(  # noqa: E731
        noise.to(DEV), texts[0], TP, SOFT, unc, **c).cpu()
    out = run(compose_text=torch.stack(texts[1:]), compose_weights=a, compose_masks=m)
    err = float((out.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"{solver} shared={shared}: composed trajectory err {err:.3e} (relative to max|reference trajectory|), bound 4 x "
          f"{gi.TWO_PASS_ERR_N5[solver]}")
    assert torch.isfinite(out).all()
    assert err <= 4 * gi.TWO_PASS_ERR_N5[solver], f"{solver}: composed err {err:.3e} > 4 x {gi.TWO_PASS_ERR_N5[solver]:.3e}"
    assert float((out - run()).abs().max()) > 1e-4, "the composed run is the single-prompt run"


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_k1_default_weights_is_the_single_prompt_run(real_model, use_graph, shared):
    """K = 1 (an explicit empty compose_text), default weights, guidance_rescale = 0.5: sample() has the bits of the same call without the
    compose keywords -- the degenerate case of the kernels through the whole sampler, eager and replayed."""
    model, g = real_model
    noise, text, unc = gi._real_inputs(g, 77)
    mk = lambda: EDM_Sampler(model, model, num_solve_steps=3, guidance=2.0, guidance_rescale=0.5, shared_guidance=shared,  # noqa: E731
                             use_graph=use_graph)
    plain = mk().sample(noise, text, TP, SOFT, unc)
    s = mk()
    empty = text.new_empty((0,) + tuple(text.shape))
    out = s.sample(noise, text, TP, SOFT, unc, compose_text=empty)
    assert torch.isfinite(out).all() and torch.equal(out, plain), f"max diff {float((out - plain).abs().max()):.3e}"
    if use_graph:
        assert torch.equal(s.sample(noise, text, TP, SOFT, unc, compose_text=empty), plain) and s._stage["key"][1] == (1, False)
