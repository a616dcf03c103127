"""Pointwise layers, input gradient + weight gradient in one launch (csrc/pbwd.hip, hdmoe_pw_bwd) -- GPU.

hdmoe_pw_bwd is called directly and compared with fp64 on the CPU, computed from the same bf16-rounded operands:

* dx, per element: half a bf16 ulp of the exact value (the store's rounding) + |alpha| * O * 2^-24 * sum_o |dy||wd| (the fp32
  accumulation over O products and the multiplication by alpha, one fp32 rounding each at most).  Derived, not tuned.
* dW: today's hdmoe_conv_wgrad (lwg_bf16_kernel) runs on the same inputs in the same test; both kernels' maximum error against fp64,
  scaled per element by sum_p |dy||x|, is measured and printed, and the fused kernel must stay within TWICE the old kernel's value:
  both sum in fp32 in a free order (MFMA chains per wave, float atomics between workgroups), a factor of two is the spread one expects
  between two such orders.  Every measured value is printed (run with -s), once more as one JSON line at the end.
* memory the launch must not touch (guard regions around dx and every G slab, the slabs of groups without rows) is compared bit for bit.
* dispatch: a bench-width model in bf16 mode with the weight bank active takes the fused launch (STATS["pbwd"], kernel_selections()
  ["pw_bwd"]) and its parameter gradients agree with the step in which the fused call is made to decline (the two old launches).
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
MARK_DX, MARK_G = 768.0, -12345.5                          # (both exact in their dtypes)
_measured = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)
    if _measured:
        print("\npointwise_bwd measured: " + json.dumps(_measured, sort_keys=True))


def _half_ulp_bf16(v64):
    """Half a bf16 ulp (8 significand bits) of |v|, 0 at v == 0 (fp64 tensor)."""
    _, e = torch.frexp(v64.abs())                              # |v| = m * 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    return torch.where(v64 == 0, torch.zeros_like(v64), torch.ldexp(torch.ones_like(v64), e - 9))


def _run_case(tag, I, O, N, HW, seg_rows, alpha=1.0, prefill=False, seed=0):
    """seg_rows: list of G + 1 row offsets, or None (seg == NULL, one group).  Returns the measured figures."""
    from hdmoe_hip._lib import call, BF16
    from hdmoe_hip import ops
    gen = torch.Generator().manual_seed(seed)
    G = 1 if seg_rows is None else len(seg_rows) - 1
    P = N * HW
    x = torch.randn(P, I, generator=gen).to(torch.bfloat16)
    dy = (0.5 * torch.randn(P, O, generator=gen)).to(torch.bfloat16)
    w = (torch.randn(G, O, I, generator=gen) / I ** 0.5).to(torch.bfloat16)
    wd = w.transpose(1, 2).contiguous()                        # the flipped image of a 1 x 1 layer: [g][I][Opad = O]
    bounds = [0, N] if seg_rows is None else list(seg_rows)
    seg = None if seg_rows is None else torch.tensor(seg_rows, dtype=torch.int32, device=DEV)

    # fp64 reference
    x64, dy64, w64 = x.double(), dy.double(), w.double()
    dx_ref = torch.zeros(P, I, dtype=torch.float64)
    dx_mag = torch.zeros(P, I, dtype=torch.float64)
    dw_ref = torch.zeros(G, O, I, dtype=torch.float64)
    dw_mag = torch.zeros(G, O, I, dtype=torch.float64)
    for g in range(G):
        a, b = bounds[g] * HW, bounds[g + 1] * HW
        dx_ref[a:b] = alpha * (dy64[a:b] @ w64[g])
        dx_mag[a:b] = abs(alpha) * (dy64[a:b].abs() @ w64[g].abs())
        dw_ref[g] = dy64[a:b].T @ x64[a:b]
        dw_mag[g] = dy64[a:b].abs().T @ x64[a:b].abs()

    # device buffers with guard regions
    xd, dyd, wdd = x.to(DEV), dy.to(DEV), wd.to(DEV)
    dxbuf = torch.full((GUARD + P * I + GUARD,), MARK_DX, dtype=torch.bfloat16, device=DEV)
    dxv = dxbuf[GUARD:GUARD + P * I]
    slab = O * I
    init = (torch.randn(G, O, I, generator=gen) * 3.0) if prefill else torch.zeros(G, O, I)

    def make_g():
        buf = torch.full((GUARD + G * (slab + GUARD),), MARK_G, dtype=torch.float32, device=DEV)
        views = [buf[GUARD + g * (slab + GUARD):GUARD + g * (slab + GUARD) + slab] for g in range(G)]
        for g in range(G):
            views[g].copy_(init[g].reshape(-1))
        return buf, views

    gbuf, gs = make_g()
    gbuf_old, gs_old = make_g()
    before = ops.kernel_selections()
    rc = call("hdmoe_pw_bwd", xd, dyd, wdd, dxv, gs, seg, G, I * O, N, HW, I, O, alpha, BF16)
    assert rc == 0, f"{tag}: hdmoe_pw_bwd declined a shape of its domain"
    assert ops.kernel_selections()["pw_bwd"] == before["pw_bwd"] + 1
    rc = call("hdmoe_conv_wgrad", xd, dyd, gs_old, seg, G, N, HW, 1, HW, 1, I, I, O, 1, 0, [1] * G, [1] * G, [0] * G, [0] * G, BF16)
    assert rc == 0
    torch.cuda.synchronize()

    # untouched memory: the guards, dx of rows outside every group, slabs of groups without rows
    assert bool((dxbuf[:GUARD] == MARK_DX).all()) and bool((dxbuf[GUARD + P * I:] == MARK_DX).all()), f"{tag}: dx guard overwritten"
    gh = gbuf.cpu()
    mask = torch.ones_like(gh, dtype=torch.bool)
    for g in range(G):
        o = GUARD + g * (slab + GUARD)
        mask[o:o + slab] = False
    assert bool((gh[mask] == MARK_G).all()), f"{tag}: G guard overwritten"
    dx_got = dxv.cpu().reshape(P, I)
    a, b = bounds[0] * HW, bounds[-1] * HW
    assert bool((dx_got[:a] == MARK_DX).all()) and bool((dx_got[b:] == MARK_DX).all()), f"{tag}: dx written outside the groups' rows"
    for g in range(G):
        if bounds[g + 1] == bounds[g]:
            assert torch.equal(gs[g].cpu(), init[g].reshape(-1)), f"{tag}: slab of the empty group {g} changed"

    # dx
    got = dx_got[a:b].double()
    ref, mag = dx_ref[a:b], dx_mag[a:b]
    bound = _half_ulp_bf16(ref) + O * 2.0 ** -24 * mag
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{tag}: dx max err / bound = {worst:.4f}  (max abs err {float(err.max()) if err.numel() else 0.0:.3e})")
    # dW against fp64, scaled by sum_p |dy||x| (prefilled slabs: the initial value is part of the exact result)
    exact = dw_ref + init.double()
    scale = (dw_mag + init.double().abs()).clamp_min(1e-300)
    new = torch.stack([t.cpu() for t in gs]).reshape(G, O, I).double()
    old = torch.stack([t.cpu() for t in gs_old]).reshape(G, O, I).double()
    e_new, e_old = float(((new - exact).abs() / scale).max()), float(((old - exact).abs() / scale).max())
    print(f"{tag}: dW scaled max err  fused {e_new:.3e}   hdmoe_conv_wgrad {e_old:.3e}   ratio {e_new / max(e_old, 1e-300):.3f}")
    _measured[tag] = dict(I=I, O=O, N=N, HW=HW, groups=G, alpha=alpha, dx_err_over_bound=worst, dw_err_fused=e_new, dw_err_conv_wgrad=e_old)
    assert bool((err <= bound).all()), f"{tag}: dx outside its bound ({worst:.3f} x)"
    assert e_new <= 2.0 * e_old, f"{tag}: dW error {e_new:.3e} > 2 x {e_old:.3e}"
    return _measured[tag]


# the bench's own shapes (profiles/r04_conv_events.json), I -> O
FLAT = [(32, 32), (64, 32)]
GROUPED = [(64, 32, 32), (64, 32, 128), (64, 128, 32), (256, 128, 64), (256, 96, 64), (1024, 64, 32), (1024, 96, 32), (1024, 32, 64)]


@pytest.mark.parametrize("I,O", FLAT, ids=[f"{i}to{o}" for i, o in FLAT])
def test_bench_shapes_flat(I, O):
    _run_case(f"flat_HW262144_{I}to{O}", I, O, 1, 262144, None)


@pytest.mark.parametrize("HW,I,O", GROUPED, ids=[f"HW{s}_{i}to{o}" for s, i, o in GROUPED])
def test_bench_shapes_grouped(HW, I, O):
    _run_case(f"grouped_N512_HW{HW}_{I}to{O}", I, O, 512, HW, [0, 131, 256, 300, 512])


@pytest.mark.parametrize("I,O", [(32, 32), (96, 64), (64, 128)], ids=["32to32", "96to64", "64to128"])
def test_edges_ragged_groups_alpha_prefill(I, O):
    """A group without rows, a group of one row, 49 positions per row (no multiple of 64 anywhere), alpha != 1, G pre-filled (+=), and
    rows in front of / behind the groups that belong to nobody."""
    _run_case(f"edges_HW49_{I}to{O}", I, O, 40, 49, [1, 6, 6, 7, 38], alpha=0.7, prefill=True, seed=3)


def test_edges_seg_null():
    _run_case("edges_segnull_HW49_32to64", 32, 64, 3, 49, None, alpha=-1.25, prefill=True, seed=4)
    _run_case("edges_segnull_HW1_64to64", 64, 64, 5, 1, None, alpha=1.0, prefill=False, seed=5)


def test_outside_the_domain_declines_without_launching():
    from hdmoe_hip._lib import call, BF16, F32
    from hdmoe_hip import ops
    P = 128
    before = ops.kernel_selections()
    for I, O, dt, tdt in [(128, 128, BF16, torch.bfloat16), (96, 96, BF16, torch.bfloat16), (48, 32, BF16, torch.bfloat16), (32, 160, BF16, torch.bfloat16),
                          (32, 32, F32, torch.float32)]:
        x = torch.ones(P, I, dtype=tdt, device=DEV)
        dy = torch.ones(P, O, dtype=tdt, device=DEV)
        wd = torch.ones(I, O, dtype=tdt, device=DEV)
        dx = torch.full((P, I), MARK_DX, dtype=tdt, device=DEV)
        G = torch.full((O, I), MARK_G, dtype=torch.float32, device=DEV)
        assert call("hdmoe_pw_bwd", x, dy, wd, dx, [G], None, 1, I * O, 1, P, I, O, 1.0, dt) == 1
        torch.cuda.synchronize()
        assert bool((dx == MARK_DX).all()) and bool((G == MARK_G).all())
    assert ops.kernel_selections()["pw_bwd"] == before["pw_bwd"]


def _grad_step(model, g, inp, kw, steps=3):
    from Utils.utils import EDM_LOSS
    lc = g["loss_cfg"]
    crit = EDM_LOSS(num_experts=kw["num_experts"], sigma_data=0.5, Unet_bal=lc["unet_bal"], vit_bal=lc["vit_bal"], z_bal=lc["z_bal"], prior_bal=0.0)
    for _ in range(steps):
        model.zero_grad(set_to_none=False)
        x = inp["x"].clone().requires_grad_(True)
        out = model(x=x, sigma=inp["sigma"], text_emb=inp["text"], Unet_router_mask=inp["unet_mask"], Vit_router_mask=inp["vit_mask"],
                    zeta=0.0, return_log_var=True, **g["extra"])
        crit(sigma_vec=inp["sigma"], x=inp["x0"], sigma=inp["sigma"], out_model=out)["loss"].backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_model_dispatch_takes_the_fused_launch(monkeypatch):
    """The bench-width model (fixture of BASELINE config 2, B = 2 ... 8), bf16 mode, third step (weight bank active): the pointwise
    layers take hdmoe_pw_bwd, and every parameter gradient agrees with the step whose fused pointwise calls are made to decline.
    Agreement: the two paths round dx to bf16 from sums taken in different orders (single-ulp flips, 2^-8 relative, in a few
    elements) and add the weight gradient's partial sums in a different order; the bound is the one this project holds its bf16
    gradients to against the reference (6e-2 of the tensor's maximum), and the median over the parameters must
    stay under two bf16 ulps (2^-7)."""
    import hdmoe_hip
    from hdmoe_hip import ops
    from conftest import wide_setup
    g = torch.load(os.path.join(ROOT, "tests", "golden", "wide_config2.pt"), weights_only=False)

    def build():
        hdmoe_hip.set_compute_dtype(torch.bfloat16)
        variant, model, kw, state, inp = wide_setup(g)
        model.load_state_dict(state)
        model = model.to(DEV).eval()
        return model, kw, {k_: v.to(DEV) for k_, v in inp.items()}

    try:
        model, kw, inp = build()
        ops.STATS.clear()
        sel0 = ops.kernel_selections()
        fused = _grad_step(model, g, inp, kw)
        assert model._hdmoe_bank is not None and len(model._hdmoe_bank.entries) > 100
        assert ops.STATS["pbwd"] > 0, dict(ops.STATS)
        assert ops.kernel_selections()["pw_bwd"] > sel0["pw_bwd"]
        n_fused = ops.STATS["pbwd"]

        real = ops._fused_bwd
        declined = []

        def decline_pointwise(bank, ent, label, name, *rest):
            if name == "hdmoe_pw_bwd":
                declined.append(label)
                return False
            return real(bank, ent, label, name, *rest)

        monkeypatch.setattr(ops, "_fused_bwd", decline_pointwise)
        model, kw, inp = build()
        ops.STATS.clear()
        sel1 = ops.kernel_selections()
        plain = _grad_step(model, g, inp, kw)
        assert ops.STATS["pbwd"] == 0 and len(declined) > 0
        assert ops.kernel_selections()["pw_bwd"] == sel1["pw_bwd"]
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)
    assert set(fused) == set(plain)
    rels = {}
    for n in fused:
        a, b = fused[n], plain[n]
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)), n
        rels[n] = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    worst = max(rels, key=rels.get)
    med = sorted(rels.values())[len(rels) // 2]
    print(f"dispatch: {n_fused} fused pointwise launches in 3 steps; parameter gradients fused vs declined: max rel {rels[worst]:.3e} ({worst}), median {med:.3e}")
    _measured["dispatch_cfg2"] = dict(pbwd_launches=n_fused, grad_max_rel=rels[worst], grad_max_rel_param=worst, grad_median_rel=med)
    assert rels[worst] <= 6e-2, (worst, rels[worst])
    assert med <= 2.0 ** -7, med
