"""The router trunks' GroupNorm(1, C) + ReLU backward on the bf16 streaming path (ops._TrunkFn.backward): hdmoe_gn1t_stats +
hdmoe_gn1t_apply, with the pooled last layer's sums taken from hdmoe_gn1_finalize_relu_mean_pq, against the layer-at-a-time kernels
hdmoe_gn1t_bwd + hdmoe_gn1t_act on the same inputs, at the benchmark's size (N = 256, 32 x 32, trunk widths 32 -> 64 -> 128 -> 128).

  a (the next conv's input) bit-identical; dx within one bf16 ulp; s1 / s2 / dgamma / dbeta within 1e-5 of their scale; pcnt / qsum
  against fp64 on the CPU; two runs bit-identical; one sample's results independent of the other samples of its batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, S = 256, 1024
LAYERS = [(2, 128, 128), (1, 128, 64), (0, 64, 32)]       # (l, C = conv output width, CI = conv input width)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    return call


def _inputs(l, C, CI, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                # noqa: E731
    t = dict(y=(r(N, S, C) * 1.7 + 0.4).cuda(), gamma=(1 + 0.3 * r(C)).cuda(), beta=(0.2 * r(C)).cuda(),
             xin=(r(N, S, CI) * 1.3 - 0.1).cuda(), g=r(N, C).cuda(), dz=r(N, S, C).to(torch.bfloat16).cuda())
    if l > 0:
        t["isc"], t["ish"] = (1 + 0.2 * r(N, CI)).cuda(), (0.3 * r(N, CI)).cuda()
    else:
        t["isc"] = t["ish"] = None
    return t


def _stats(call, t, C):
    """The pooled forward with a single statistics slot per sample: mean / rstd (and pcnt / qsum) exactly as the trunk forward makes them."""
    y = t["y"]
    slot = torch.stack([y.double().sum((1, 2)), y.double().square().sum((1, 2))], -1).float().reshape(N, 1, 2).contiguous()
    out, sc, sh = (torch.empty(N, C, device="cuda") for _ in range(3))
    mean, rstd = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    P, Q = torch.empty(N, C, device="cuda"), torch.empty(N, C, device="cuda")
    call("hdmoe_gn1_finalize_relu_mean_pq", out, sc, sh, mean, rstd, P, Q, y, slot, t["gamma"], t["beta"], N, 1, S, C, 1e-5)
    return mean, rstd, P, Q


def _old(call, t, l, C, CI, mean, rstd):
    dx = torch.empty(N, S, C, dtype=torch.bfloat16, device="cuda")
    dg, db, ws = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.empty(2 * N, device="cuda")
    pooled = l == 2
    call("hdmoe_gn1t_bwd", dx, dg, db, ws, None if pooled else t["dz"], t["g"] if pooled else None, 1.0 / S if pooled else 1.0,
         t["y"], t["gamma"], t["beta"], mean, rstd, N, S, C)
    a = torch.empty(N, S, CI, dtype=torch.bfloat16, device="cuda")
    call("hdmoe_gn1t_act", a, t["xin"], t["isc"], t["ish"], N, S, CI)
    return dict(dx=dx, a=a, dg=dg, db=db, s1=ws[:N], s2=ws[N:])


def _new(call, t, l, C, CI, mean, rstd, P, Q):
    import hdmoe_hip
    dx = torch.empty(N, S, C, dtype=torch.bfloat16, device="cuda")
    a = torch.empty(N, S, CI, dtype=torch.bfloat16, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    pooled = l == 2
    ws = None
    if not pooled:
        ws = torch.full((hdmoe_hip.lib().hdmoe_gn1t_stats_floats(N, S, C),), float("nan"), device="cuda")
        call("hdmoe_gn1t_stats", ws, t["dz"], t["y"], t["gamma"], t["beta"], mean, rstd, N, S, C)
    call("hdmoe_gn1t_apply", dx, a, dg, db, ws, None if pooled else t["dz"], t["g"] if pooled else None, 1.0 / S if pooled else 1.0,
         P if pooled else None, Q if pooled else None, t["y"], t["gamma"], t["beta"], mean, rstd, t["xin"], t["isc"], t["ish"], N, S, C, CI)
    r = dict(dx=dx, a=a, dg=dg, db=db)
    if pooled:
        k = (t["g"].double() / S * t["gamma"].double())
        r["s1"], r["s2"] = (k * P.double()).sum(1), (k * Q.double()).sum(1)
    else:
        parts = ws.numel() // (2 * N * (1 + C))
        slots = ws[:2 * N * parts].view(N, parts, 2).double().sum(1)
        r["s1"], r["s2"], r["slots"] = slots[:, 0], slots[:, 1], ws[:2 * N * parts].view(N, parts, 2)
    return r


def _ulp_close(a, b, rel_atol=1e-6):
    a, b = a.float(), b.float()
    m = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(m > 0, torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-30))) - 7), torch.zeros_like(m))
    return bool(((a - b).abs() <= ulp + rel_atol * float(b.abs().max())).all())


@pytest.mark.parametrize("l,C,CI", LAYERS)
def test_matches_the_layer_at_a_time_kernels(lib, l, C, CI):
    call = lib
    t = _inputs(l, C, CI, 11 + l)
    mean, rstd, P, Q = _stats(call, t, C)
    old = _old(call, t, l, C, CI, mean, rstd)
    new = _new(call, t, l, C, CI, mean, rstd, P, Q)
    torch.cuda.synchronize()
    assert torch.equal(new["a"], old["a"])
    assert _ulp_close(new["dx"], old["dx"])
    for k in ("s1", "s2", "dg", "db"):
        ref = old[k].double()
        assert float((new[k].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), k


def test_pooled_statistics_against_fp64(lib):
    call = lib
    C = 128
    t = _inputs(2, C, 128, 5)
    mean, rstd, P, Q = _stats(call, t, C)
    y = t["y"].cpu().double()
    xh = (y - mean.cpu().double()[:, None, None]) * rstd.cpu().double()[:, None, None]
    mask = xh * t["gamma"].cpu().double() + t["beta"].cpu().double() > 0
    Pref, Qref = mask.double().sum(1), (xh * mask).sum(1)
    P, Q = P.cpu().double(), Q.cpu().double()
    # a pre-activation within fp32 rounding of zero may open in one and not the other: a handful of the 33.5 M at most
    same = P == Pref
    assert int((~same).sum()) <= 8 and float((P - Pref).abs().max()) <= 1
    assert float((Q - Qref)[same].abs().max()) <= 1e-5 * float(Qref.abs().max())


@pytest.mark.parametrize("l,C,CI", LAYERS)
def test_deterministic_and_batch_independent(lib, l, C, CI):
    call = lib
    t = _inputs(l, C, CI, 23 + l)
    mean, rstd, P, Q = _stats(call, t, C)
    r1 = _new(call, t, l, C, CI, mean, rstd, P, Q)
    r2 = _new(call, t, l, C, CI, mean, rstd, P, Q)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    # every sample but the first replaced: the first sample's outputs and sums keep every bit
    u = _inputs(l, C, CI, 99 + l)
    u["gamma"], u["beta"] = t["gamma"], t["beta"]
    for k, v in u.items():
        if v is not None and v.dim() > 1 and k in t:
            v[0] = t[k][0]
    m2, rs2, P2, Q2 = _stats(call, u, C)
    assert torch.equal(m2[0], mean[0]) and torch.equal(rs2[0], rstd[0]) and torch.equal(P2[0], P[0]) and torch.equal(Q2[0], Q[0])
    r3 = _new(call, u, l, C, CI, m2, rs2, P2, Q2)
    torch.cuda.synchronize()
    assert torch.equal(r3["dx"][0], r1["dx"][0]) and torch.equal(r3["a"][0], r1["a"][0])
    assert torch.equal(r3["s1"][0], r1["s1"][0]) and torch.equal(r3["s2"][0], r1["s2"][0])
    if "slots" in r1:
        assert torch.equal(r3["slots"][0], r1["slots"][0])


def test_forward_mask_agrees_bit_for_bit_with_the_backward_masks(lib):
    """pcnt of the pooled forward counts exactly the positions whose ReLU the backward kernels see open.  With dz = 1 the statistics
    kernels' dbeta partials are those counts (integers: exact in fp32 in any order); with dz = 1 and zero sums the apply kernel's dx is
    nonzero exactly where its mask is open."""
    import hdmoe_hip
    call = lib
    C = 128
    t = _inputs(2, C, 128, 7)
    mean, rstd, P, Q = _stats(call, t, C)
    ones = torch.ones(N, S, C, dtype=torch.bfloat16, device="cuda")
    ws = torch.full((hdmoe_hip.lib().hdmoe_gn1t_stats_floats(N, S, C),), float("nan"), device="cuda")
    call("hdmoe_gn1t_stats", ws, ones, t["y"], t["gamma"], t["beta"], mean, rstd, N, S, C)
    parts = ws.numel() // (2 * N * (1 + C))
    cnt_stats = ws[2 * N * parts:].view(2, C, N, parts)[1].sum(-1).t()
    zero = torch.zeros_like(ws)
    dx = torch.empty(N, S, C, dtype=torch.bfloat16, device="cuda")
    a = torch.empty(N, S, 128, dtype=torch.bfloat16, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    call("hdmoe_gn1t_apply", dx, a, dg, db, zero, ones, None, 1.0, None, None, t["y"], t["gamma"], t["beta"], mean, rstd, t["xin"],
         t["isc"], t["ish"], N, S, C, 128)
    cnt_apply = (dx != 0).sum(1).float()
    odx, odg, odb, ows = torch.empty_like(dx), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.empty(2 * N, device="cuda")
    call("hdmoe_gn1t_bwd", odx, odg, odb, ows, ones, None, 1.0, t["y"], t["gamma"], t["beta"], mean, rstd, N, S, C)
    torch.cuda.synchronize()
    assert bool((t["gamma"] != 0).all())
    assert torch.equal(cnt_stats, P)
    assert torch.equal(cnt_apply, P)
    assert torch.equal(odb, P.sum(0))
