"""EDM loss, router head and dispatch kernels against fp64 restatements of the reference, at their clamps, masks and launch edges.

* ops.edm_loss          (csrc/loss.hip)   vs oracle.edm_loss in float64 (reference Utils/utils.py:127-172), stats + six gradients
* ops.router_head       (csrc/router.hip) vs masked_fill -> softmax -> top-k -> softmax -> scatter (models/model_components.py:155-168)
* ops.DispatchPlan, gather_rows, combine_rows, seg / route counters  vs  x[mask] per expert, output[mask] += y * w
  (models/model_config1.py:11-39)

Every comparison checks the NaN pattern and the exact-zero pattern first, then a stated bound on the rest.
u = 2**-24 is the fp32 unit roundoff.
"""
import math

import pytest
import torch

from oracle import hdmoe_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
STATS = ("loss", "denoising", "balance", "z_loss", "pure_loss")


def _ops():
    from hdmoe_hip import ops
    return ops


def _match(k, r, bound, msg):
    """k (device, any float) vs r (fp64 CPU): same NaN and +-inf positions, zero exactly where r is zero (and only there),
    |k - r| <= bound elsewhere (bound: tensor broadcastable to r, or a float)."""
    k = k.detach().cpu().double()
    assert k.shape == r.shape, (msg, k.shape, r.shape)
    assert torch.equal(k.isnan(), r.isnan()), f"{msg}: NaN pattern {int(k.isnan().sum())} vs {int(r.isnan().sum())}"
    assert torch.equal(k.isinf(), r.isinf()) and torch.equal(k[k.isinf()], r[r.isinf()]), f"{msg}: inf pattern"
    assert torch.equal(k == 0, r == 0), f"{msg}: zero pattern ({int((k == 0).sum())} vs {int((r == 0).sum())} zeros)"
    fin = torch.isfinite(r)
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(r)
    err = (k - r).abs()
    bad = fin & (err > b)
    assert not bad.any(), f"{msg}: {int(bad.sum())} entries over the bound, worst |err| {float(err[bad].max()):.3e} " \
                          f"at bound {float(b[bad][err[bad].argmax()]):.3e}"


# =====================================================================================================
# 1. EDM loss
# =====================================================================================================
G_LOSS = 0.625          # cotangent of the loss (exact in fp32): checks that the backward scales by the incoming gradient


def _loss_ref(D, T, lv, pU, pV, rU, rV, lam):
    """oracle.edm_loss evaluated in float64 on the same fp32 inputs: (stats (5,), [dD, dlv, dpU, dpV, drU, drV])."""
    leaves = [None if t is None else t.double().requires_grad_(True) for t in (D, lv, pU, pV, rU, rV)]
    d, l, pu, pv, ru, rv = leaves
    out = O.edm_loss({"denoised": d, "log_var": l, "Unet_router_loss": pu, "vit_router_loss": pv, "Unet_raw": ru, "vit_raw": rv},
                     T.double(), pU.shape[1], *lam)
    out["loss"].backward(torch.tensor(G_LOSS, dtype=torch.float64))
    return torch.stack([out[s].detach() for s in STATS]), [None if t is None else t.grad for t in leaves]


def _loss_hip(D, T, lv, pU, pV, rU, rV, lam):
    leaves = [None if t is None else t.to(DEV).requires_grad_(True) for t in (D, lv, pU, pV, rU, rV)]
    d, l, pu, pv, ru, rv = leaves
    loss, st = _ops().edm_loss(d, T.to(DEV), l, pu, pv, ru, rv, *lam)
    lf = float(loss.detach())
    assert float(st[0]) == lf or (math.isnan(float(st[0])) and math.isnan(lf))
    loss.backward(torch.tensor(G_LOSS, device=DEV))
    return st, [None if t is None else t.grad for t in leaves]


def _check_loss(D, T, lv, pU, pV, rU, rV, lam, tag):
    """Stats: fp32 sums of <= 16 serial terms per thread, a 256-wide tree, <= 4 chunk atomics and one B-wide tree, plus
    __expf / __logf (relative error ~ |arg| u): 1e-5 relative, with 1e-6 absolute for terms that cancel (lv < 0) or vanish.
    Gradients: each entry is a product of a few fp32 factors (one __expf): 1e-5 relative, plus 1e-6 of the tensor's largest
    magnitude for the entries that cancel (dlog_var = gp (1 - ms e^-lv) / B; dlogits carry lse = m + log s).  Zero and NaN
    patterns are exact, so a gradient that a flag wrongly kills or passes fails whatever its size."""
    st_r, g_r = _loss_ref(D, T, lv, pU, pV, rU, rV, lam)
    st_k, g_k = _loss_hip(D, T, lv, pU, pV, rU, rV, lam)
    _match(st_k, st_r, 1e-5 * st_r.abs().nan_to_num(0.0) + 1e-6, f"{tag}: stats {STATS}")
    for name, k, r in zip(("d_denoised", "d_log_var", "d_pU", "d_pV", "d_rU", "d_rV"), g_k, g_r):
        if r is None:
            assert k is None, (tag, name)
            continue
        fin = r[torch.isfinite(r)]
        amax = float(fin.abs().max()) if fin.numel() else 0.0
        _match(k, r, 1e-5 * r.abs().nan_to_num(0.0) + 1e-6 * amax, f"{tag}: {name}")
    return st_r, g_r


def _loss_inputs(B, L, E, with_lv, seed, shape=None):
    g = torch.Generator().manual_seed(seed)
    shape = shape or (B, L, 1, 1)
    T = torch.randn(shape, generator=g)
    D = T + 0.5 * torch.randn(shape, generator=g)
    lv = (torch.rand(B, 1, 1, 1, generator=g) * 3 - 1.5) if with_lv else None
    pU = torch.softmax(torch.randn(B, E, generator=g), -1)
    pV = torch.softmax(2 * torch.randn(B, E, generator=g), -1)
    rU = 3 * torch.randn(B, E, generator=g)
    rV = 2 * torch.randn(B, E, generator=g) + 1
    return D, T, lv, pU, pV, rU, rV


# (B, L, E): every B in {1, 3, 256, 257, 1000}, every L in {1, 4095, 4096, 4097, 3*4096+5} (chunk tails of sse_rows_kernel),
# every E in {1, 4, 8, 64}
LOSS_SHAPES = [(1, 1, 1), (3, 4095, 4), (256, 4096, 8), (257, 4097, 64), (1000, 3 * 4096 + 5, 4), (3, 1, 64), (1, 3 * 4096 + 5, 8),
               (257, 4095, 1), (1000, 4097, 8), (256, 1, 4)]


@pytest.mark.parametrize("with_lv", [False, True])
@pytest.mark.parametrize("B,L,E", LOSS_SHAPES)
def test_edm_loss_shapes(B, L, E, with_lv):
    st, _ = _check_loss(*_loss_inputs(B, L, E, with_lv, seed=B * 7 + L + E), (0.5, 0.7, 0.05), f"B={B} L={L} E={E} lv={with_lv}")
    assert bool(torch.isfinite(st).all()) and float(st[0]) < 50.0       # the unclamped regime: every gradient flows


@pytest.mark.parametrize("with_lv", [False, True])
def test_edm_loss_bench_latent(with_lv):
    """BASELINE config 2 (the bench workload): B = 256 latents of img_channels x img_resolution^2, 4 experts."""
    from Utils import configs
    bc = configs.BASELINE_CONFIGS[2]
    kw = configs.model_kwargs(**bc["over"])
    B, C, R, E = bc["batch"], kw["IN_in_channels"], kw["IN_img_resolution"], kw["num_experts"]
    lc = configs.loss_configs
    _check_loss(*_loss_inputs(B, C * R * R, E, with_lv, seed=2, shape=(B, C, R, R)), (lc["unet_bal"], lc["vit_bal"], lc["z_bal"]),
                f"bench latent lv={with_lv}")


def _regime(name):
    """Inputs + lambdas that put exactly one clamp of the loss in the regime `name` (the others stay well inside)."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    B, L, E = 4, 5, 4
    T = torch.randn(B, L, 1, 1, generator=g)
    D = T + 0.3 * torch.randn(B, L, 1, 1, generator=g)
    lv = None
    pU = torch.softmax(torch.randn(B, E, generator=g), -1)
    pV = torch.softmax(torch.randn(B, E, generator=g), -1)
    rU, rV = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    lam = (0.5, 0.5, 0.01)
    if name == "pure_gt50":            # pure clamps; balance = z = 0 so the total sits exactly at 50 and passes its own clamp
        D = T + 12.0 * torch.randn(B, L, 1, 1, generator=g)
        lam = (0.0, 0.0, 0.0)
    elif name == "pure_eq50":          # B = 2, L = 1, errors 8 and 6: pure = (64 + 36) / 2 = 50 exactly -> gradient passes
        B, L = 2, 1
        T = torch.tensor([1.0, -2.0]).view(2, 1, 1, 1)
        D = T + torch.tensor([8.0, 6.0]).view(2, 1, 1, 1)
        pU, pV, rU, rV = pU[:2], pV[:2], rU[:2], rV[:2]
        lam = (0.0, 0.0, 0.0)
    elif name == "bal_gt50":           # large lambda; pure = z = 0
        D = T.clone()
        lam = (400.0, 300.0, 0.0)
    elif name == "bal_eq50":           # E = 1, p = 1: balance = lu * 1 * 1 = 50 exactly
        D, E = T.clone(), 1
        pU, pV, rU, rV = torch.ones(B, 1), torch.ones(B, 1), torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)
        lam = (50.0, 0.0, 0.0)
    elif name == "z_gt50":
        D = T.clone()
        rU, rV = 30 * torch.randn(B, E, generator=g), 30 * torch.randn(B, E, generator=g)
        lam = (0.0, 0.0, 2.0)
    elif name == "z_eq50_lse_eq10":    # E = 1, logit 10: lse = 10 exactly, lse^2 = 100 exactly (passes), z = 0.25 * (100 + 100) = 50
        D, E = T.clone(), 1
        pU, pV = torch.ones(B, 1), torch.ones(B, 1)
        rU, rV = torch.full((B, 1), 10.0), torch.full((B, 1), 10.0)
        lam = (0.0, 0.0, 0.25)
    elif name == "total_gt50":         # pure ~ 30, balance ~ 16, z ~ 7: each below 50, the sum above
        D = T + 5.5 * torch.randn(B, L, 1, 1, generator=g)
        lam = (8.0, 8.0, 0.5)
        rU, rV = 4 + torch.randn(B, E, generator=g), 4 + torch.randn(B, E, generator=g)
    elif name == "log_var_edges":      # outside +-10 (no gradient), exactly +-10 (torch passes the gradient), inside
        B = 6
        T = torch.randn(B, L, 1, 1, generator=g)
        D = T + 1e-3 * torch.randn(B, L, 1, 1, generator=g)
        lv = torch.tensor([-12.0, -10.0, 10.0, 12.0, 0.5, -3.0]).view(B, 1, 1, 1)
        pU, pV = torch.softmax(torch.randn(B, E, generator=g), -1), torch.softmax(torch.randn(B, E, generator=g), -1)
        rU, rV = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    elif name == "logit_edges":        # raw logits outside +-50, exactly +-50, -inf (masked); row 0's lse^2 clamps at 100
        E = 8
        rU = torch.tensor([[60.0, 50.0, -50.0, -60.0, -math.inf, 1.0, 2.0, 3.0],
                           [-50.0, -60.0, -math.inf, 2.0, 1.0, 0.5, -49.5, -50.5],
                           [-math.inf, -50.0, -50.0, 0.0, 1.5, -2.0, 3.0, -70.0],
                           [2.0, 1.0, 0.0, -1.0, -2.0, -3.0, -50.0, 55.0]])
        rV = torch.tensor([[-55.0, -50.0, 0.25, 1.0, 2.0, -math.inf, -math.inf, 3.0]] * 4)
        pU = torch.softmax(torch.randn(B, E, generator=g), -1)
        pV = torch.softmax(torch.randn(B, E, generator=g), -1)
        lam = (0.5, 0.5, 0.02)
    else:
        raise KeyError(name)
    return (D, T, lv, pU, pV, rU, rV), lam


# which gradients must vanish identically in each regime (besides exact agreement of the zero pattern, which _match checks)
REGIMES = {"pure_gt50": ("d_denoised",), "pure_eq50": (), "bal_gt50": ("d_pU", "d_pV"), "bal_eq50": (), "z_gt50": ("d_rU", "d_rV"),
           "z_eq50_lse_eq10": (), "total_gt50": ("d_denoised", "d_pU", "d_pV", "d_rU", "d_rV"), "log_var_edges": (), "logit_edges": ()}
NONZERO = {"pure_eq50": ("d_denoised",), "bal_eq50": ("d_pU",), "z_eq50_lse_eq10": ("d_rU", "d_rV")}


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_edm_loss_clamp_regimes(name):
    inputs, lam = _regime(name)
    st, g = _check_loss(*inputs, lam, name)
    names = ("d_denoised", "d_log_var", "d_pU", "d_pV", "d_rU", "d_rV")
    grads = dict(zip(names, g))
    for n in REGIMES[name]:                                    # the regime is what the inputs claim it is
        assert float(grads[n].abs().max()) == 0.0, (name, n)
    for n in NONZERO.get(name, ()):                            # exactly at a bound: torch's clamp passes the gradient
        assert bool((grads[n] != 0).any()), (name, n)
    if name.endswith("eq50") or name == "z_eq50_lse_eq10":
        assert float(st[0]) == 50.0
    if name == "total_gt50":                                   # each term below its own bound, the total above
        assert float(st[0]) == 50.0 and max(float(st[2]), float(st[3]), float(st[4])) < 50.0 and float(st[2] + st[3] + st[4]) > 50.0
    if name == "log_var_edges":                                # no gradient beyond +-10, a gradient at +-10 and inside
        assert grads["d_log_var"].flatten().ne(0).tolist() == [False, True, True, False, True, True]
    if name == "logit_edges":                                  # row 0 lse^2 > 100: no z gradient; row 1: -50 passes, -50.5 / -inf do not
        assert grads["d_rU"][0].abs().max() == 0 and grads["d_rU"][1].ne(0).tolist() == [True, False, False, True, True, True, True, False]


NONFINITE = ["nan_denoised", "nan_denoised_lv", "nan_log_var", "nan_gate_row", "nan_raw_logit"]


@pytest.mark.parametrize("name", NONFINITE)
def test_edm_loss_nonfinite(name):
    """A NaN anywhere makes the reference's loss NaN (torch.clamp propagates NaN); the kernel must report the same stats and the same
    NaN / exact-zero gradient pattern, not a finite loss read off a clamp bound."""
    D, T, lv, pU, pV, rU, rV = _loss_inputs(5, 33, 8, name in ("nan_denoised_lv", "nan_log_var"), seed=11)
    if name.startswith("nan_denoised"):
        D[2, 7] = float("nan")
    elif name == "nan_log_var":
        lv[3] = float("nan")
    elif name == "nan_gate_row":                   # an all-masked sample: the router's gate probabilities are NaN on that row
        mask = torch.ones(5, 8)
        mask[1] = 0
        pU = O.router_head(rU, mask, 2)[1]
        rU = rU.masked_fill(mask == 0, float("-inf"))
        assert pU[1].isnan().all()
    elif name == "nan_raw_logit":
        rV[4, 3] = float("nan")
    st, g = _check_loss(D, T, lv, pU, pV, rU, rV, (0.5, 0.7, 0.05), name)
    assert math.isnan(float(st[0]))
    if name == "nan_log_var":                      # the reference's pattern (checked above against the kernel): dlv = 0, dD NaN on row 3 only
        assert float(g[1].abs().max()) == 0.0 and g[0][3].isnan().all() and float(g[0][[0, 1, 2, 4]].abs().max()) == 0.0


# =====================================================================================================
# 2. Router head
# =====================================================================================================
def _head_ref(logits, noise, mask, k):
    """The reference head with the noise added in fp32 (as the model does) and the rest in fp64 autograd.  Top-k order: a stable
    descending sort, i.e. ties -> lowest index (torch.topk leaves the tie order open; the kernel documents lowest index first)."""
    x = logits if noise is None else logits + noise
    if mask is not None:
        x = x.masked_fill(mask == 0, float("-inf"))
    xd = x.double().requires_grad_(True)
    probs = torch.softmax(xd, -1)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
    w = torch.softmax(xd.gather(-1, order), -1)
    sparse = torch.zeros_like(xd).scatter(-1, order, w)
    return x, xd, sparse, probs, order


def _head_check(logits, noise, mask, k, seed, tag):
    B, E = logits.shape
    ops = _ops()
    x, xd, sp_r, pr_r, idx_r = _head_ref(logits, noise, mask, k)
    lg = logits.to(DEV).requires_grad_(True)
    sp, pr, xo, idx = ops.router_head(lg, None if noise is None else noise.to(DEV), None if mask is None else mask.to(DEV), k)
    assert torch.equal(xo.detach().cpu(), x), f"{tag}: masked logits (bit-exact fp32)"
    assert torch.equal(idx.cpu().long(), idx_r), f"{tag}: top-k indices (lowest index on ties)"
    # fp32: one expf (~1 ulp) of an argument rounded to |x - max| u, a sum of <= E positive terms ((E - 1) u), one division
    gap_p = (x.double() - x.double().amax(-1, keepdim=True)).abs().nan_to_num(0.0, posinf=0.0)
    top = x.double().gather(-1, idx_r[:, :1])
    gap_s = (x.double() - top).abs().nan_to_num(0.0, posinf=0.0)
    pr_r32 = pr_r.detach().float().double()       # fp32 rounding of the reference: exp(-120) underflows to 0 there as in the kernel
    _match(pr, pr_r32, (E + 4 + gap_p) * U * pr_r32.abs().nan_to_num(0.0) + 1e-44, f"{tag}: probs")
    sp_r32 = sp_r.detach().float().double()
    _match(sp, sp_r32, (k + 4 + gap_s) * U * sp_r32.abs().nan_to_num(0.0) + 1e-44, f"{tag}: sparse")
    # backward: random cotangents on all three outputs
    g = torch.Generator().manual_seed(seed)
    cs, cp, cx = (torch.randn(B, E, generator=g) for _ in range(3))
    (dl_r,) = torch.autograd.grad((sp_r, pr_r, xd), (xd,), (cs.double(), cp.double(), cx.double()))
    if mask is not None:
        dl_r = dl_r.masked_fill(mask == 0, 0.0)           # masked_fill's backward
    (dl,) = torch.autograd.grad((sp, pr, xo), (lg,), (cs.to(DEV), cp.to(DEV), cx.to(DEV)))
    p, s = pr_r.detach().nan_to_num(0.0), sp_r.detach().nan_to_num(0.0)
    scale = cx.double().abs() + p * (cp.double().abs() + (p * cp.double().abs()).sum(-1, keepdim=True)) \
        + s * (cs.double().abs() + (s * cs.double().abs()).sum(-1, keepdim=True))
    # dl = dx + p (dp - <p, dp>) + s (ds - <s, ds>): p and s carry the forward's relative error ((E + 4 + gap) u <= ~1e-5 here),
    # the dot products a few u more: 2e-5 of the magnitude sum.  Masked entries and all-masked rows: exactly 0.
    _match(dl, dl_r, 2e-5 * scale, f"{tag}: dlogits")
    if mask is not None:
        assert not bool(dl.cpu()[mask == 0].ne(0).any()), f"{tag}: dlogits on masked entries"
    return sp, idx


def _tied_logits(B, E, g):
    """Logits and noise on a 1/4 grid: their fp32 sum is exact and ties are common, at the k-th place included."""
    return torch.round(4 * torch.randn(B, E, generator=g)) / 4, torch.round(2 * torch.randn(B, E, generator=g)) / 4


def _masks(B, E, k, g):
    """none | random | rows with fewer than k unmasked experts | all-masked rows (mixed with ordinary rows)."""
    rnd = (torch.rand(B, E, generator=g) > 0.3).float()
    rnd[:, 0] = torch.where(rnd.sum(1) == 0, 1.0, rnd[:, 0])     # random: every row keeps one expert
    few = torch.ones(B, E)
    if E > 1:
        for b in range(B):
            keep = torch.randperm(E, generator=g)[: max(1, min(k - 1, E - 1)) if b % 2 == 0 else 1]
            few[b] = 0
            few[b, keep] = 1
    allm = rnd.clone()
    allm[:: 3] = 0
    return {"none": None, "random": rnd, "few": few, "all_masked": allm}


HEAD_EK = [(1, 1), (2, 1), (2, 2), (8, 1), (8, 2), (8, 8), (64, 1), (64, 2), (64, 64)]


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("E,k", HEAD_EK)
def test_router_head(E, k, B, noisy):
    g = torch.Generator().manual_seed(E * 1000 + k * 10 + B + noisy)
    lg, nz = _tied_logits(B, E, g)
    for mname, mask in _masks(B, E, k, g).items():
        tag = f"E={E} k={k} B={B} noise={noisy} mask={mname}"
        sp, idx = _head_check(lg, nz if noisy else None, mask, k, seed=B + E, tag=tag)
        spc = sp.detach().cpu()
        if mask is not None:                                   # masked experts are never routed: weight exactly 0
            assert not bool(spc.nan_to_num(0.0)[mask == 0].ne(0).any()), tag
        if mname == "few" and E > 1:                           # -inf picks: in idx, weight 0, not routed (sparse > 0 is False)
            n_open = mask.sum(1).long()
            short = n_open < k
            assert bool(short.any()) or k == 1
            assert torch.equal((spc > 0).sum(1)[short], n_open[short]), tag


def test_router_head_ties_exact():
    """Exact ties at the k-th place: lowest index wins, and the tied picks get bit-equal weights."""
    ops = _ops()
    lg = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, 0.0, 2.0, 2.0],
                       [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0],
                       [0.0, 1.0, 2.0, 2.0, -1.0, 2.0, 1.0, 2.0]])
    sp, _, _, idx = ops.router_head(lg.to(DEV), None, None, 2)
    assert idx.cpu().tolist() == [[1, 2], [0, 1], [2, 3]]
    spc = sp.cpu()
    assert spc[0, 1] == spc[0, 2] == 0.5 and spc[1, 0] == spc[1, 1] == 0.5 and spc[2, 2] == spc[2, 3] == 0.5
    assert int((spc > 0).sum()) == 6


def test_router_head_underflow():
    """Gaps beyond 104 underflow exp() in fp32 (the reference's fp32 weight is exactly 0, so the pair is not routed);
    a gap of 60 stays a normal number and is routed."""
    lg = torch.tensor([[0.0, -120.0, -130.0, -200.0], [10.0, -50.0, -111.0, -115.0], [-5.0, -125.0, 100.0, 99.0]])
    sp, _ = _head_check(lg, None, None, 2, seed=5, tag="underflow")
    spc = sp.detach().cpu()
    assert spc[0, 1] == 0 and spc[0, 0] == 1 and spc[1, 1] > 0 and spc[2, 3] > 0
    assert (spc > 0).sum(1).tolist() == [1, 2, 2]
    plan = _ops().DispatchPlan(sp.detach(), 2)
    assert plan.seg.cpu().tolist() == [0, 2, 3, 4, 5]


def test_router_head_grid_stride():
    """B > 2048 blocks x 256 threads: the row loop wraps (thread t also owns row t + 524288)."""
    B, E, k = 2048 * 256 + 1000, 4, 2
    g = torch.Generator().manual_seed(77)
    lg, nz = _tied_logits(B, E, g)
    mask = (torch.rand(B, E, generator=g) > 0.25).float()
    mask[::97] = 0
    _head_check(lg, nz, mask, k, seed=78, tag="grid-stride")


# =====================================================================================================
# 3. Dispatch plan, gather, combine, counters
# =====================================================================================================
def _plan_ref(sparse, kcap):
    """x[mask] per expert, concatenated (expert-major, sample-stable), at capacity R = B * kcap: routed <=> weight > 0 (NaN: no).
    inv[b * kcap + j] = position of sample b's j-th routed expert (ascending expert order), -1 when absent."""
    B, E = sparse.shape
    R = B * kcap
    routed = sparse > 0
    e_i, b_i = routed.t().nonzero(as_tuple=True)
    n = min(int(e_i.numel()), R)
    perm = torch.full((R,), -1, dtype=torch.long)
    row_expert = torch.full((R,), -1, dtype=torch.long)
    row_w = torch.zeros(R)
    inv = torch.full((R,), -1, dtype=torch.long)
    perm[:n], row_expert[:n], row_w[:n] = b_i[:n], e_i[:n], sparse[b_i[:n], e_i[:n]]
    slot = (routed.long().cumsum(1) - 1)[b_i[:n], e_i[:n]]
    keep = slot < kcap
    inv[b_i[:n][keep] * kcap + slot[keep]] = torch.arange(n)[keep]
    seg = torch.cat([torch.zeros(1, dtype=torch.long), routed.sum(0).cumsum(0)]).clamp(max=R)
    return dict(perm=perm, row_expert=row_expert, row_w=row_w, inv=inv, seg=seg)


def _sparse_pattern(B, E, k, pattern, g):
    """(B, E) gate weights.  mixed: k random experts per row from a subset that leaves experts empty, some top-k weights exactly 0,
    rows routed nowhere (all zero) and all-masked rows (NaN at the picks); one_expert: every row to one expert;
    overflow: rows with more routed experts than kcap = k (positions past R are dropped, seg clamps at R)."""
    sp = torch.zeros(B, E)
    if pattern == "one_expert":
        sp[:, E // 2] = torch.rand(B, generator=g) + 0.1
        return sp
    if pattern == "overflow":
        m = torch.rand(B, E, generator=g) < 0.7
        return torch.where(m, torch.rand(B, E, generator=g) + 0.01, torch.zeros(B, E))
    pool = torch.arange(E)[torch.arange(E) % 3 != 1] if E >= 3 else torch.arange(E)
    for b in range(B):
        pick = pool[torch.randperm(len(pool), generator=g)[: min(k, len(pool))]]
        sp[b, pick] = torch.rand(len(pick), generator=g) + 0.05
        r = b % 11
        if r == 3:
            sp[b, pick[0]] = 0.0                   # zero-weight top-k entry
        elif r == 5:
            sp[b] = 0.0                            # routed nowhere
        elif r == 7:
            sp[b, pick] = float("nan")             # all-masked sample
    return sp


def _check_plan(sparse, kcap, tag):
    ops = _ops()
    plan = ops.DispatchPlan(sparse.to(DEV), kcap)
    ref = _plan_ref(sparse, kcap)
    for f in ("perm", "row_expert", "inv", "seg"):
        got = getattr(plan, f).cpu().long()
        assert torch.equal(got, ref[f]), f"{tag}: {f} differs at {int((got != ref[f]).sum())} positions"
    assert torch.equal(plan.row_w.cpu(), ref["row_w"]), f"{tag}: row_w (bit-exact copy of the weight, 0 padding)"
    return plan, ref


@pytest.mark.parametrize("kcap_mode", ["k", "E"])
@pytest.mark.parametrize("E", [1, 8, 64])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 4096])
def test_dispatch_plan(B, E, kcap_mode):
    """64-lane ballot and 1024-thread workgroup edges of the single-workgroup scan; exact perm / row_expert / row_w / inv / seg."""
    k = min(2, E)
    kcap = k if kcap_mode == "k" else E
    g = torch.Generator().manual_seed(B * 100 + E + kcap)
    for pattern in ("mixed", "one_expert") + (("overflow",) if kcap == k else ()):
        sparse = _sparse_pattern(B, E, k, pattern, g)
        plan, ref = _check_plan(sparse, kcap, f"B={B} E={E} kcap={kcap} {pattern}")
        if pattern == "mixed" and E >= 3:
            seg = ref["seg"]
            assert int((seg[1:] == seg[:-1]).sum()) > 0            # the case really has experts without rows
        # counters accumulate across calls: two calls == twice the restated per-expert row counts
        ops = _ops()
        cs = torch.zeros(E, device=DEV)
        cr = torch.zeros(E, device=DEV)
        for _ in range(2):
            ops.call("hdmoe_seg_counts", cs, plan.seg, E)
            ops.call("hdmoe_route_counts", cr, sparse.to(DEV).contiguous(), B, E)
        assert torch.equal(cs.cpu(), 2 * (ref["seg"][1:] - ref["seg"][:-1]).float())
        assert torch.equal(cr.cpu(), 2 * (sparse > 0).sum(0).float())


def _plan_for(B, E, k, kcap, seed):
    g = torch.Generator().manual_seed(seed)
    sparse = _sparse_pattern(B, E, k, "mixed", g)
    plan, ref = _check_plan(sparse, kcap, f"plan B={B} E={E} kcap={kcap}")
    return sparse, plan, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L,offset", [(8, 0), (64, 0), (7, 0), (8, 1), (1, 0)])
@pytest.mark.parametrize("B", [65, 1025])
def test_gather_rows(B, L, offset, dtype):
    """16-byte path (L * size % 16 == 0, aligned) and the scalar path (odd L, or a view one element off): bit-exact,
    zeros in unused rows; the backward (combine without weights) sums the routed rows in slot order -- exact in fp32 and,
    rounded once, in bf16."""
    ops = _ops()
    E, k, kcap = 8, 2, 2
    sparse, plan, ref = _plan_for(B, E, k, kcap, seed=B + L + offset)
    g = torch.Generator().manual_seed(L)
    buf = torch.randn(B * L + offset, generator=g).to(dtype)
    if offset:                                     # a contiguous view one element past an aligned base: scalar path
        x = buf.to(DEV)[offset:].view(B, L)
        assert x.data_ptr() % 16 != 0
    else:
        x = buf.to(DEV).view(B, L).clone().requires_grad_(True)
    out = ops.gather_rows(x, plan)
    perm = ref["perm"]
    want = torch.where((perm >= 0).view(-1, 1), buf[offset:].view(B, L)[perm.clamp(min=0)], torch.zeros((), dtype=dtype))
    assert torch.equal(out.detach().cpu(), want), f"gather B={B} L={L} offset={offset} {dtype}"
    if offset == 0:
        go = torch.randn(plan.R, L, generator=g).to(dtype)
        (dx,) = torch.autograd.grad(out, x, go.to(DEV))
        inv = ref["inv"].view(B, kcap)
        acc = torch.zeros(B, L)
        for j in range(kcap):
            r = inv[:, j]
            acc = acc + torch.where((r >= 0).view(-1, 1), go.float()[r.clamp(min=0)], torch.zeros(()))
        assert torch.equal(dx.cpu(), acc.to(dtype)), f"gather backward B={B} L={L} {dtype}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kcap", [2, 8])
@pytest.mark.parametrize("L", [1, 8192, 8193, 3 * 8192 + 5])
def test_combine_rows(L, kcap, dtype):
    """out[b] = sum of w * ys over b's routed rows; dys = w * dout[perm] (one fp32 product: exact); dsparse = <dout[b], ys[r]>
    summed per 8192-element chunk and added atomically (chunk boundaries at L = 8192, 8193, 3*8192+5)."""
    ops = _ops()
    B, E, k = 65, 8, 2
    sparse, plan, ref = _plan_for(B, E, k, kcap, seed=L + kcap)
    R = plan.R
    g = torch.Generator().manual_seed(L * 3 + kcap)
    ys = torch.randn(R, L, generator=g).to(dtype)
    dout = torch.randn(B, L, generator=g).to(dtype)
    ys_d = ys.to(DEV).requires_grad_(True)
    sp_d = sparse.to(DEV).requires_grad_(True)
    out = ops.combine_rows(ys_d, sp_d, plan)
    dys, dsp = torch.autograd.grad(out, (ys_d, sp_d), dout.to(DEV))
    # fp64 restatement: output[mask] += y * w over the routed pairs that the plan holds (slot < kcap)
    perm, rexp, inv = ref["perm"], ref["row_expert"], ref["inv"]
    pos = inv[inv >= 0]
    b_i, e_i = perm[pos], rexp[pos]
    ysd = ys.double().requires_grad_(True)
    spd = sparse.double().requires_grad_(True)
    out_r = torch.zeros(B, L, dtype=torch.float64).index_add(0, b_i, spd[b_i, e_i].unsqueeze(1) * ysd[pos])
    dys_r, dsp_r = torch.autograd.grad(out_r, (ysd, spd), dout.double())
    # forward: <= kcap fp32 products and adds (kcap u of sum |w y|), then the output rounding (2^-24 fp32, 2^-8 bf16)
    mag = torch.zeros(B, L, dtype=torch.float64).index_add(0, b_i, (spd[b_i, e_i].unsqueeze(1) * ysd[pos]).abs()).detach()
    rnd = U if dtype == torch.float32 else 2.0 ** -8
    _match(out, out_r.detach(), (kcap + 1) * U * mag + rnd * out_r.detach().abs(), f"combine fwd L={L} kcap={kcap} {dtype}")
    # dys: w * dout[perm[r]] computed once in fp32 and rounded to the storage type -- bit-exact; rows without a sample: 0
    gsel = torch.where((perm >= 0).view(-1, 1), dout.float()[perm.clamp(min=0)], torch.zeros(()))
    assert torch.equal(dys.cpu(), (ref["row_w"].view(-1, 1) * gsel).to(dtype)), f"dys L={L} kcap={kcap} {dtype}"
    # dsparse: per thread <= 32 serial fp32 products (8192 / 256), an 8-level block tree, ceil(L / 8192) atomics:
    # (32 + 8 + nck + 2) u of sum |dout ys| (bf16 products are exact in fp32).  Pairs not routed: exactly 0 (NaN rows too).
    nck = -(-L // 8192)
    dmag = torch.zeros(B, E, dtype=torch.float64)
    dmag[b_i, e_i] = (dout.double()[b_i] * ys.double()[pos]).abs().sum(1)
    _match(dsp, dsp_r.nan_to_num(0.0), (42 + nck) * U * dmag, f"dsparse L={L} kcap={kcap} {dtype}")
