"""ViT expert bank: patch embed / unpatch over each expert's own row window (ops.vit_bank_embed / ops.vit_bank_unpatch) -- GPU.

1. Window contract of every row-windowed entry point (hdmoe_patch_relayout_rows, hdmoe_patch_relayout_tiled_rows, hdmoe_bias_add_rows,
   hdmoe_pw_fwd_rows, the hdmoe_rag_*_own family, hdmoe_rag_zero_unowned): N = 5 rows, 16 x 16 images, windows [1, 3), [0, 5) and the empty
   [2, 2) read from a device tensor; input rows outside the window hold NaN, the output is prefilled with a finite sentinel between guard
   regions.  Rows inside the window are torch.equal to what the all-rows entry point writes for them from clean input, rows outside still
   hold the sentinel, the guards are intact, and [0, N) equals the all-rows result everywhere.
2. Windowed weight and bias gradients (hdmoe_conv_wgrad with seg = the window and one group, hdmoe_colsum_rows): operands NaN outside the
   window, result finite, compared with an fp64 sum over the window's rows; the yardstick is today's all-rows kernel on inputs zeroed
   outside the window against the same fp64 reference (both printed): the windowed kernel may have at most twice that error (another
   summation order of the same fp32 sums).  An empty window gives exactly zero.
3. The bank end to end against the ops.VIT_BANK_ROWS = False path on the same weights: output and dx equal with ==, the router-weight
   gradient and every parameter gradient within the tolerance test_vit_bank_matches_the_per_expert_path uses, a never-routed expert has a
   zero or None gradient, the row_window selection counter moved -- and stays at zero for a declined shape (res 10, p = 4 / 5).
4. A torch.cuda.graph of forward + backward captured under routing A and replayed under routing B (other counts, one expert loses all its
   rows) against an eager run under B; once without and once with the weight bank (unpatch_proj's gradient through the bank's slabs).
5. The sampler's bank (8 experts, patches [4, 4, 8, 8, 8, 16, 16, 16]) forward in eval mode against the attribute-off path.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
MARK = 768.0                                                    # exact in bf16 and fp32
N, HH, WW = 5, 16, 16
WINDOWS = [(1, 3), (0, 5), (2, 2)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)
    hdmoe_hip.ops.VIT_BANK_ROWS = True


def _guarded(n, dtype, mark=MARK):
    buf = torch.full((GUARD + n + GUARD,), mark, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n, mark=MARK):
    return bool((buf[:GUARD] == mark).all()) and bool((buf[GUARD + n:] == mark).all())


def _rows(b, e):
    return torch.tensor([b, e], dtype=torch.int32, device=DEV)


def _window_contract(tag, src, out_per_row, out_dtype, run_rows, run_all):
    """src (N, ...) clean input; run_rows(out, inp, rows) / run_all(out, inp) launch on out (N * out_per_row elements, flat)."""
    n_out = N * out_per_row
    rbuf, ref = _guarded(n_out, out_dtype)
    run_all(ref, src)
    torch.cuda.synchronize()
    assert _guards_ok(rbuf, n_out), f"{tag}: the all-rows call wrote outside its output"
    ref = ref.view(N, out_per_row)
    assert bool(torch.isfinite(ref.float()).all())
    for b, e in WINDOWS:
        inp = src.clone()
        inp[:b] = float("nan")
        inp[e:] = float("nan")
        buf, out = _guarded(n_out, out_dtype)
        run_rows(out, inp, _rows(b, e))
        torch.cuda.synchronize()
        assert _guards_ok(buf, n_out), f"{tag} [{b},{e}): wrote outside its output"
        out = out.view(N, out_per_row)
        assert torch.equal(out[b:e], ref[b:e]), f"{tag} [{b},{e}): rows inside the window differ from the all-rows result"
        assert bool((out[:b] == MARK).all()) and bool((out[e:] == MARK).all()), f"{tag} [{b},{e}): rows outside the window were written"


def _randn(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("p", [4, 8, 16])
@pytest.mark.parametrize("to_img", [0, 1])
def test_relayout_rows_window_contract(p, to_img, dtype):
    """Both relayout entry points, both directions, PixelShuffle order (and order 0 on the plain entry point)."""
    from hdmoe_hip._lib import call, dtype_code
    from hdmoe_hip import ops
    C, hp, wp = 8, HH // p, WW // p
    dt = dtype_code(dtype)
    n_img, n_tok = HH * WW * C, hp * wp * C * p * p
    src = _randn((N, n_tok if to_img else n_img), dtype, 11 * p + to_img)
    per = n_img if to_img else n_tok
    before = ops.kernel_selections()["row_window"]
    for order in (1, 0):
        geo = (N, HH, WW, C, p, hp, wp, order, to_img, dt)
        _window_contract(f"relayout_rows p={p} order={order}", src, per, dtype,
                         lambda o, i, r: call("hdmoe_patch_relayout_rows", o, i, r, *geo),
                         lambda o, i: call("hdmoe_patch_relayout", o, i, *geo))
    assert ops.kernel_selections()["row_window"] - before == 2 * len(WINDOWS)
    geo = (N, HH, WW, C, p, hp, wp, 1, to_img, dt)
    probe = torch.empty(N * per, dtype=dtype, device=DEV)
    if call("hdmoe_patch_relayout_tiled", probe, src, *geo) == 0:            # p is a multiple of the vector width: the tiled kernel's domain
        def tiled_rows(o, i, r):
            assert call("hdmoe_patch_relayout_tiled_rows", o, i, r, *geo) == 0
        _window_contract(f"relayout_tiled_rows p={p}", src, per, dtype, tiled_rows,
                         lambda o, i: call("hdmoe_patch_relayout_tiled", o, i, *geo))
    else:
        assert call("hdmoe_patch_relayout_tiled_rows", probe, src, _rows(0, N), *geo) == 1   # declines what the all-rows form declines
        assert p == 4 and dtype == torch.bfloat16


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_bias_add_rows_window_contract(dtype):
    from hdmoe_hip._lib import call, dtype_code
    S, L = 16, 8
    src = _randn((N, S * L), dtype, 5)
    bias = _randn((L,), torch.float32, 6)
    dt = dtype_code(dtype)
    _window_contract("bias_add_rows", src, S * L, dtype,
                     lambda o, i, r: call("hdmoe_bias_add_rows", o, i, bias, r, N, S, L, dt),
                     lambda o, i: call("hdmoe_bias_add", o, i, bias, N * S, L, dt))


# (Cin, Cout, positions per row, flat): the patch GEMM and its input gradient at C = 8, E = 8 (generic kernels, per-row tiles), the same at
# C = 32, E = 32 (kgemm forward: Cin >= 512), unpatch_proj forward and its input gradient as one long row of positions (conv_fwd5 / kgemm)
PW_CASES = [(128, 8, 16, 0), (512, 8, 4, 0), (2048, 8, 1, 0), (8, 128, 16, 0), (8, 2048, 1, 0),
            (512, 32, 16, 0), (2048, 32, 4, 0), (8192, 32, 1, 0), (32, 512, 16, 0),
            (8, 128, 16, 1), (8, 512, 4, 1), (8, 2048, 1, 1), (32, 512, 16, 1), (32, 8192, 1, 1), (512, 32, 16, 1), (8192, 32, 1, 1), (128, 8, 16, 1)]


@pytest.mark.parametrize("Cin,Cout,L,flat", PW_CASES)
def test_pw_fwd_rows_window_contract(Cin, Cout, L, flat):
    from hdmoe_hip._lib import call, BF16
    Ipad = (Cin + 15) // 16 * 16
    src = _randn((N, L * Cin), torch.bfloat16, Cin + Cout + L)
    w = torch.zeros(Cout, Ipad, dtype=torch.bfloat16, device=DEV)
    w[:, :Cin] = _randn((Cout, Cin), torch.bfloat16, Cin * 3 + Cout) / Cin ** 0.5
    geo = (1, 1, N * L) if flat else (N, 1, L)

    def run_rows(o, i, r):
        assert call("hdmoe_pw_fwd_rows", i, w, o, 1.0, r, N, 1, L, Cin, Ipad, Cout, flat, BF16) == 0

    def run_all(o, i):
        call("hdmoe_conv_fwd", i, w, o, None, 1.0, 0.0, None, 1, w.numel(), *geo, geo[1], geo[2], Cin, Cin, Ipad, Cout, Cout, 1, 0, [1], [1], [0], [0], BF16)
    _window_contract(f"pw_fwd_rows {Cin}->{Cout} L={L} flat={flat}", src, L * Cout, torch.bfloat16, run_rows, run_all)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rag_own_rows_window_contract(dtype):
    """The own-row modes against the all-rows kernels: expert g's compact tensor is touched in [seg[g], seg[g+1]) only.  Three experts
    over 5 rows (+ one row of no expert): windows [0, 2), [2, 2) (empty) and [2, 4)."""
    from hdmoe_hip._lib import call, dtype_code
    dt = dtype_code(dtype)
    R, C, lens, Sp = N, 8, [16, 4, 1], 16
    segl = [0, 2, 2, 4]
    seg = torch.tensor(segl, dtype=torch.int32, device=DEV)
    tok = _randn((R, Sp, C), dtype, 3)
    # unpack
    refs = [torch.empty((R, L, C), dtype=dtype, device=DEV) for L in lens]
    call("hdmoe_rag_unpack", refs, tok, seg, lens, 3, R, Sp, C, dt)
    bufs = [_guarded(R * L * C, dtype) for L in lens]
    call("hdmoe_rag_unpack_own", [o for _, o in bufs], tok, seg, lens, 3, R, Sp, C, dt)
    torch.cuda.synchronize()
    for g, ((buf, out), L) in enumerate(zip(bufs, lens)):
        assert _guards_ok(buf, R * L * C)
        out, b, e = out.view(R, L, C), segl[g], segl[g + 1]
        assert torch.equal(out[b:e], refs[g][b:e]) and bool((out[:b] == MARK).all()) and bool((out[e:] == MARK).all()), g
    # pack backward
    pos_a = [torch.zeros((1, L, C), dtype=torch.float32, device=DEV) for L in lens]
    pos_b = [torch.zeros((1, L, C), dtype=torch.float32, device=DEV) for L in lens]
    call("hdmoe_rag_pack_bwd", refs, pos_a, tok, seg, lens, 3, R, Sp, C, dt)
    bufs = [_guarded(R * L * C, dtype) for L in lens]
    call("hdmoe_rag_pack_bwd_own", [o for _, o in bufs], pos_b, tok, seg, lens, 3, R, Sp, C, dt)
    torch.cuda.synchronize()
    for g, ((buf, out), L) in enumerate(zip(bufs, lens)):
        assert _guards_ok(buf, R * L * C)
        out, b, e = out.view(R, L, C), segl[g], segl[g + 1]
        assert torch.equal(out[b:e], refs[g][b:e]) and bool((out[:b] == MARK).all()) and bool((out[e:] == MARK).all()), g
        torch.testing.assert_close(pos_b[g], pos_a[g], rtol=1e-6, atol=1e-6)
    assert float(pos_b[1].abs().max()) == 0.0                                  # the expert without rows: exact zero
    # unpack backward: NaN outside the own rows must not be read; the all-rows kernel gets zeros there
    parts = [_randn((R, L, C), dtype, 20 + g) for g, L in enumerate(lens)]
    clean, dirty = [], []
    for g, pt in enumerate(parts):
        b, e = segl[g], segl[g + 1]
        z, d = torch.zeros_like(pt), torch.full_like(pt, float("nan"))
        z[b:e] = pt[b:e]
        d[b:e] = pt[b:e]
        clean.append(z); dirty.append(d)
    ref = torch.empty((R, Sp, C), dtype=dtype, device=DEV)
    call("hdmoe_rag_unpack_bwd", ref, clean, seg, lens, 3, R, Sp, C, dt)
    buf, out = _guarded(R * Sp * C, dtype)
    call("hdmoe_rag_unpack_bwd_own", out, dirty, seg, lens, 3, R, Sp, C, dt)
    torch.cuda.synchronize()
    assert _guards_ok(buf, R * Sp * C) and bool((out.view(R, Sp, C) == ref).all())
    # rows of no expert := 0, owned rows untouched
    buf, out = _guarded(R * 64, dtype)
    call("hdmoe_rag_zero_unowned", out, seg, 3, R, 64 * out.element_size())
    torch.cuda.synchronize()
    out = out.view(R, 64)
    assert _guards_ok(buf, R * 64) and bool((out[:4] == MARK).all()) and bool((out[4:] == 0).all())


# (Cin of x, Cout of dy, positions per row, dtype): patch-embed weight gradient at E = 8 (tiled general kernel) and E = 32 (streamed
# pointwise kernel), unpatch_proj's at E = 32, the streamed kernel in fp32
WG_CASES = [(128, 8, 16, torch.bfloat16), (512, 32, 16, torch.bfloat16), (2048, 32, 4, torch.bfloat16), (32, 512, 16, torch.bfloat16),
            (32, 8192, 1, torch.bfloat16), (128, 32, 16, torch.float32)]


@pytest.mark.parametrize("I,O,L,dtype", WG_CASES)
def test_windowed_weight_and_bias_gradients(I, O, L, dtype):
    from hdmoe_hip._lib import call, dtype_code
    dt = dtype_code(dtype)
    x = _randn((N, L, I), dtype, I + L)
    dy = _randn((N, L, O), dtype, O + L + 1) * 0.5
    geo = (N, 1, L, 1, L, I, I, O, 1, 0, [1], [1], [0], [0], dt)
    for b, e in WINDOWS:
        xn, dyn = torch.full_like(x, float("nan")), torch.full_like(dy, float("nan"))
        xz, dyz = torch.zeros_like(x), torch.zeros_like(dy)
        for clean, src in ((xn, x), (xz, x), (dyn, dy), (dyz, dy)):
            clean[b:e] = src[b:e]
        ref = torch.einsum("po,pi->oi", dy[b:e].reshape(-1, O).double().cpu(), x[b:e].reshape(-1, I).double().cpu())
        refb = dy[b:e].reshape(-1, O).double().cpu().sum(0)
        Gw = torch.zeros((1, O, I), dtype=torch.float32, device=DEV)
        Ga = torch.zeros((1, O, I), dtype=torch.float32, device=DEV)
        call("hdmoe_conv_wgrad", xn, dyn, [Gw], _rows(b, e), 1, *geo)
        call("hdmoe_conv_wgrad", xz, dyz, [Ga], None, 1, *geo)
        bw = torch.zeros(O, dtype=torch.float32, device=DEV)
        ba = torch.zeros(O, dtype=torch.float32, device=DEV)
        call("hdmoe_colsum_rows", bw, dyn, _rows(b, e), N, L, O, dt)
        call("hdmoe_colsum", ba, dyz, N * L, O, dt)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(Gw).all()) and bool(torch.isfinite(bw).all()), f"[{b},{e}): a row outside the window was read"
        ew, ea = float((Gw[0].double().cpu() - ref).abs().max()), float((Ga[0].double().cpu() - ref).abs().max())
        ebw, eba = float((bw.double().cpu() - refb).abs().max()), float((ba.double().cpu() - refb).abs().max())
        print(f"wgrad {I}->{O} L={L} {dtype} [{b},{e}): windowed err {ew:.3e}, all-rows err {ea:.3e} (max |G| {float(ref.abs().max()):.3e}); "
              f"colsum windowed {ebw:.3e}, all-rows {eba:.3e}")
        if b == e:
            assert float(Gw.abs().max()) == 0.0 and float(bw.abs().max()) == 0.0
        assert ew <= 2 * ea and ebw <= 2 * eba


# ------------------------------------------------------------------------------------------------------------ the bank
def _close_scaled(a, b, rel, msg="", atol=1e-6):
    """max|a-b| <= rel * max|b| + atol (tests/test_hip_parity.py close_scaled)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), msg
    d, bound = float((a - b).abs().max()), rel * float(b.abs().max()) + atol
    assert d <= bound, f"{msg}: max|a-b| = {d:.3e} > {bound:.3e}"


def _make_bank(res, patches, C=8):
    import models.model_components as mc
    torch.manual_seed(7)
    bank = torch.nn.ModuleList([mc.Vit_expert(num_heads=2, num_groups=2, in_channels=C, seq_ln=(-(-res // p)) ** 2, emb_dim=8, num_blocks=2,
                                              patch_size=p, time_dim=6, text_dim=5) for p in patches]).to(DEV)
    with torch.no_grad():
        for n, prm in bank.named_parameters():
            if "rel_pos_bias" in n or "pos_emb" in n:
                prm.normal_(0, 0.5)
            elif n.endswith(".bias") or ("norm" in n or "GN" in n) and n.endswith(".weight"):
                prm.add_(0.3 * torch.randn_like(prm))
    return bank


def _routing(B, E, k, seed, dead):
    """(B, E) routing weights, at most k experts per sample; the experts in ``dead`` get no sample; sample 1 goes to one expert only."""
    g = torch.Generator().manual_seed(seed)
    live = [e for e in range(E) if e not in dead]
    w = torch.zeros(B, E)
    for b in range(B):
        idx = torch.tensor(live)[torch.randperm(len(live), generator=g)[:k]]
        w[b, idx] = torch.rand(len(idx), generator=g) + 0.2
    w[1] = 0.0
    w[1, live[0]] = 1.0
    return w.to(DEV)


def _inputs(B, res, C=8):
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return mk(B, C, res, res), mk(B, 6), mk(B, 5), mk(B, C, res, res)


def _run_bank(mods, x, te, text, w, gout, k, rows_on, backward=True):
    import hdmoe_hip
    from hdmoe_hip import ops
    from models import _assembly as A
    ops.VIT_BANK_ROWS = rows_on
    try:
        before = ops.kernel_selections()["row_window"]
        xx = x.clone().requires_grad_(backward)
        ww = w.clone().requires_grad_(backward)
        xs = ops.cast(ops.to_nhwc(xx), torch.bfloat16)
        out = ops.from_nhwc(A._dispatch_nhwc(xs, mods, ww, te, text, kcap=k))
        if backward:
            out.float().backward(gout)
        torch.cuda.synchronize()
        return dict(out=out.detach().float(), dx=xx.grad, dw=ww.grad, pg={n: p.grad for n, p in mods.named_parameters()},
                    windowed=ops.kernel_selections()["row_window"] - before)
    finally:
        ops.VIT_BANK_ROWS = True


def _compare(new, old, dead, E, rel=3e-2):
    assert bool((new["out"] == old["out"]).all()), "out"
    assert bool((new["dx"] == old["dx"]).all()), "dx"
    _close_scaled(new["dw"], old["dw"], rel, msg="d(router weights)")
    gmax = max(float(v.abs().max()) for v in old["pg"].values() if v is not None)
    for n, gref in old["pg"].items():
        gnew = new["pg"][n]
        if any(n.startswith(f"{d}.") for d in dead):
            assert gnew is None or float(gnew.abs().max()) == 0.0, n       # never-routed expert: no gradient
        elif gref is None:
            assert gnew is None or float(gnew.abs().max()) == 0.0, n
        else:
            _close_scaled(gnew, gref, rel * 2, msg=n, atol=rel * 0.1 * gmax)


@pytest.mark.parametrize("res,patches,k", [(16, [4, 8, 8, 16], 2), (8, [2, 4, 8], 1)])
def test_bank_rows_matches_all_rows_path(res, patches, k):
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    E, B = len(patches), 6
    bank = _make_bank(res, patches)
    ref_bank = copy.deepcopy(bank)
    x, te, text, gout = _inputs(B, res)
    w = _routing(B, E, k, 3, dead=[E - 1])
    new = _run_bank(bank, x, te, text, w, gout, k, True)
    old = _run_bank(ref_bank, x, te, text, w, gout, k, False)
    assert new["windowed"] > 0 and old["windowed"] == 0
    _compare(new, old, [E - 1], E)


def test_bank_rows_declined_shape_takes_the_all_rows_path():
    """res 10 does not divide into patches of 4: no windowed launch, and the result is the attribute-off path's."""
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    patches, k, B = [2, 4, 5, 4], 2, 6
    bank = _make_bank(10, patches)
    ref_bank = copy.deepcopy(bank)
    x, te, text, gout = _inputs(B, 10)
    w = _routing(B, 4, k, 3, dead=[3])
    new = _run_bank(bank, x, te, text, w, gout, k, True)
    old = _run_bank(ref_bank, x, te, text, w, gout, k, False)
    assert new["windowed"] == 0 and old["windowed"] == 0
    _compare(new, old, [3], 4)


def test_graph_replay_follows_the_new_routing():
    """Forward + backward captured under routing A, replayed under routing B (other counts; expert 1 goes from some rows to none)."""
    import hdmoe_hip
    from hdmoe_hip import ops, bank as wbank
    from models import _assembly as A
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    res, patches, k, B = 16, [4, 8, 8, 16], 2, 6
    E = len(patches)
    wbank.deactivate()
    mods = _make_bank(res, patches).eval()                     # (eval: the forward does not re-normalise the stored weights in place)
    ref_mods = copy.deepcopy(mods)
    x, te, text, gout = _inputs(B, res)
    wA, wB = _routing(B, E, k, 3, dead=[E - 1]), _routing(B, E, k, 4, dead=[1])
    assert not torch.equal((wA > 0).sum(0), (wB > 0).sum(0)) and int((wA[:, 1] > 0).sum()) > 0
    eager = _run_bank(ref_mods, x, te, text, wB, gout, k, True)

    sx, sw = x.clone().requires_grad_(True), wA.clone().requires_grad_(True)

    def step():
        ops.zero_pool_reset(sx.device)                         # the accumulate-into scratch of the backward kernels starts from zero
        xs = ops.cast(ops.to_nhwc(sx), torch.bfloat16)
        out = ops.from_nhwc(A._dispatch_nhwc(xs, mods, sw, te, text, kcap=k))
        out.float().backward(gout)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                 # warm-up under routing A (lazy attribute calls, the zero pool's size)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in [sx, sw] + list(mods.parameters()):
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sout = step()
    with torch.no_grad():
        sw.copy_(wB)
    graph.replay()
    torch.cuda.synchronize()
    new = dict(out=sout.detach().float(), dx=sx.grad, dw=sw.grad, pg={n: p.grad for n, p in mods.named_parameters()})
    _compare(new, eager, [1], E)


def test_graph_replay_with_the_weight_bank_follows_the_new_routing():
    """The same with the weight bank active, as in the benchmarked step: unpatch_proj's images come from the bank, its windowed weight
    gradient accumulates into the bank's slab and the bank's finish launch (queued by note_backward) makes the gradient.  The reference is
    the same procedure run eagerly under routing B on a copy of the experts with a bank of its own."""
    import hdmoe_hip
    from hdmoe_hip import ops, bank as wbank
    from models import _assembly as A
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    res, patches, k, B = 16, [4, 8, 8, 16], 2, 6
    E = len(patches)
    x, te, text, gout = _inputs(B, res)
    wA, wB = _routing(B, E, k, 3, dead=[E - 1]), _routing(B, E, k, 4, dead=[1])
    base = _make_bank(res, patches).eval()                     # (eval: the bank's prepare launch does not re-normalise the stored weights)

    def make():
        mods = copy.deepcopy(base)
        sx, sw = x.clone().requires_grad_(True), wA.clone().requires_grad_(True)
        bank = wbank.bank_for(mods)

        def step():
            for t in [sx, sw] + list(mods.parameters()):       # the kernels and the bank's finish launch accumulate into .grad
                if t.grad is not None:
                    t.grad.zero_()
            bank.begin_step(False)
            xs = ops.cast(ops.to_nhwc(sx), torch.bfloat16)
            out = ops.from_nhwc(A._dispatch_nhwc(xs, mods, sw, te, text, kcap=k))
            out.float().backward(gout)
            return out
        return mods, sx, sw, bank, step

    def result(mods, sx, sw, out):
        return dict(out=out.detach().float(), dx=sx.grad, dw=sw.grad, pg={n: p.grad for n, p in mods.named_parameters()})

    try:
        mods, sx, sw, bank, step = make()
        step()                                                 # registers the call sites with the bank
        step()                                                 # first step on the bank's images and slabs
        with torch.no_grad():
            sw.copy_(wB)
        eager = result(mods, sx, sw, step())
        torch.cuda.synchronize()
        eager = {k_: (v.clone() if torch.is_tensor(v) else {n: (None if g is None else g.clone()) for n, g in v.items()}) for k_, v in eager.items()}
        ent = bank.lookup([mods[0].unpatch_proj.weights], torch.bfloat16, 1.0, 1.0, True)
        assert ent is not None and ent.used_bwd, "unpatch_proj did not run on the weight bank"

        mods, sx, sw, bank, step = make()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        before = ops.kernel_selections()["row_window"]
        with torch.cuda.graph(graph):
            sout = step()
        assert ops.kernel_selections()["row_window"] > before
        with torch.no_grad():
            sw.copy_(wB)
        graph.replay()
        torch.cuda.synchronize()
        _compare(result(mods, sx, sw, sout), eager, [1], E)
    finally:
        wbank.deactivate()


def test_sampler_bank_forward_matches_all_rows_path():
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    patches, k, B = [4, 4, 8, 8, 8, 16, 16, 16], 2, 6
    bank = _make_bank(16, patches).eval()
    x, te, text, gout = _inputs(B, 16)
    w = _routing(B, 8, k, 9, dead=[2])
    with torch.no_grad():
        new = _run_bank(bank, x, te, text, w, gout, k, True, backward=False)
        old = _run_bank(bank, x, te, text, w, gout, k, False, backward=False)
    assert new["windowed"] > 0 and old["windowed"] == 0
    assert bool((new["out"] == old["out"]).all())
