"""FiLM backward in the dgrad epilogue of the streaming backward launch (hdmoe_conv_bwd6_film: conv7_body<.., EPI = 1> in csrc/conv7_body.h)
and the keep-mask variants of the FiLM kernels (hdmoe_film_silu_drop_fwd_mask / hdmoe_film_silu_mask_bwd in csrc/elementwise.hip).

The two-launch form is the reference for everything that must not move: dx of hdmoe_conv_bwd6 followed by hdmoe_film_silu_drop_bwd gives du,
and the fused launch must reproduce it BIT FOR BIT (same rounding of g to bf16, same multiplications in the same order, keep bits taken from
the Philox words the forward drew).  The weight gradients of the same launch are compared against a second two-launch run (their own
run-to-run difference).  de is a sum over the image in another order: it is compared against an fp64 evaluation of the same formula from the
same bf16 tensors, normalised per entry by sum |g'| |u| (g' = g * keep / (1 - p) * mp_silu'(u e)), and may be at most twice as far from it
as the standalone kernel is (or as that kernel's run-to-run spread, it sums with float atomics); two fused runs must agree exactly.

Shapes: the smallest that reach each path (C7_MIN_IMAGES = 192 images).  u holds exact zeros (kept, with a non-zero gradient: the mask cannot be
recovered from h == 0) and negative values; one expert has no rows.

Case b (64 channels on 32 x 32 maps) keeps its partial sums of de in the weight-ring buffer the last stage has consumed (they do not fit
behind the two image tiles)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {   # N, map, C (conv_res2: C -> C), kernel sizes, segment ends, fused?
    "a": (192, 32, 32, (3, 5, 3), (90, 90, 192), True),
    "b": (192, 32, 64, (3, 5, 3), (90, 90, 192), True),
    "c": (193, 16, 64, (3, 5, 3, 5), (51, 51, 100, 193), True),          # groups of 51 and 93 rows: pairs with an absent second image
    "d": (191, 32, 32, (3, 5, 3), (90, 90, 191), False),                 # below conv7's domain
}
P_DROP = (0.2, 0.0)
SEED = 0x1234567


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _silu_grad64(x):
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s)) / 0.596


_cache = {}


def _setup(case, p):
    """Operands, the forward with and without the mask, and the two-launch backward (twice) -- computed once per (case, p)."""
    if (case, p) in _cache:
        return _cache[(case, p)]
    from hdmoe_hip import ops
    from hdmoe_hip._lib import _int_array, call, lib
    from hdmoe_hip.bank import w6_record
    N, R, C, ks, split, _ = CASES[case]
    g = torch.Generator().manual_seed(1000 * N + R + C)
    u = torch.randn(N, R, R, C, generator=g)
    u[torch.rand(N, R, R, C, generator=g) < 0.05] = 0.0                # exact zeros; negatives come with randn
    u = u.bfloat16().cuda()
    e = (1.0 + 0.3 * torch.randn(N, C, generator=g)).cuda()
    dy = torch.randn(N, R, R, C, generator=g).bfloat16().cuda()
    ws = [(torch.randn(C, C, k, k, generator=g) / (k * C ** 0.5)).cuda() for k in ks]
    E, taps = len(ks), max(k * k for k in ks)
    wstride = taps * C * C
    wf = torch.empty(E * wstride, dtype=torch.bfloat16, device="cuda")
    wd = torch.empty(E * wstride, dtype=torch.bfloat16, device="cuda")
    call("hdmoe_wprep_fwd", ws, None, 1.0, list(ks), list(ks), E, C, C, C, C, wf, wstride, wd, wstride, 0, 0, 1, 1)
    seg = torch.tensor([0] + list(split), dtype=torch.int32, device="cuda")
    HW = R * R
    # ---- forward: h with and without the mask output
    h0 = torch.empty_like(u)
    mask = None
    if p > 0:
        call("hdmoe_film_silu_drop_fwd", h0, u, e, N, HW, C, SEED, None, p, 1)
        h = torch.empty_like(u)
        mask = torch.full((u.numel() // 8,), 0xAA, dtype=torch.uint8, device="cuda")
        call("hdmoe_film_silu_drop_fwd_mask", h, mask, u, e, N, HW, C, SEED, None, p, 1)
    else:
        call("hdmoe_film_silu_fwd", h0, u, e, N, HW, C, 1)
        h = h0
    kib = lib().hdmoe_conv_wgrad6_ws_kib(E, N, R, R, C, C, ctypes.cast(_int_array(ks), ctypes.c_void_p), ctypes.cast(_int_array(ks), ctypes.c_void_p), 1)
    assert kib > 0
    pts = [(k - 1) // 2 for k in ks]
    alpha = 0.7

    def wgrads(launch):
        wsb = torch.full((2 * kib * 256,), float("nan"), dtype=torch.float32, device="cuda")
        Gs = [torch.zeros(k * k, C, C, device="cuda") for k in ks]
        before = ops.kernel_selections()
        rc = launch(Gs, wsb)
        sel = _delta(before, ops.kernel_selections())
        if rc == 0:
            call("hdmoe_conv_wgrad6_reduce_batch", Gs + [None] * (8 - E), [seg], [wsb], w6_record(E, N, R, R, C, C, 1, ks), 1)
        return rc, Gs, sel

    def unfused():
        dx = torch.full_like(u, float("nan"))
        rc, Gs, sel = wgrads(lambda Gs, wsb: call("hdmoe_conv_bwd6", h, dy, wd, dx, Gs, seg, E, wstride, N, R, R, C, C, list(ks), list(ks), pts, pts, alpha,
                                                  wsb, wsb.numel() * 4, 1))
        assert rc == 0 and "film_dgrad" not in sel, sel
        du, de = torch.empty_like(u), torch.zeros_like(e)
        if p > 0:
            call("hdmoe_film_silu_drop_bwd", du, de, dx, u, e, N, HW, C, SEED, None, p, 1)
        else:
            call("hdmoe_film_silu_bwd", du, de, dx, u, e, N, HW, C, 1)
        return dx, du, de, Gs

    def fused():
        du = torch.full_like(u, float("nan"))
        de = torch.full_like(e, float("nan"))                       # written, not accumulated
        rc, Gs, sel = wgrads(lambda Gs, wsb: call("hdmoe_conv_bwd6_film", h, dy, wd, du, Gs, seg, E, wstride, N, R, R, C, C, list(ks), list(ks), pts, pts,
                                                  alpha, wsb, wsb.numel() * 4, u, e, mask, de, p, 1))
        return rc, du, de, Gs, sel

    s = dict(N=N, R=R, C=C, HW=HW, p=p, u=u, e=e, h=h, h0=h0, mask=mask, unfused=(unfused(), unfused()), fused=fused)
    torch.cuda.synchronize()
    _cache[(case, p)] = s
    return s


def _de_fp64(s, g):
    """(de, sum |g'| |u|) in fp64 from the bf16 tensors: g = dx of the plain launch, keep bits unpacked from the mask."""
    u, e = s["u"].double(), s["e"].double()
    t = g.double()
    if s["mask"] is not None:
        bits = (s["mask"].view(-1, 1).int() >> torch.arange(8, device="cuda").view(1, 8)) & 1
        t = t * bits.view(u.shape).double() * float(torch.tensor(1.0 / (1.0 - s["p"]), dtype=torch.float32))
    t = t * _silu_grad64(u * e[:, None, None, :]) * u
    return t.sum(dim=(1, 2)), t.abs().sum(dim=(1, 2))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_mask_forward_and_standalone_backward(gpu, case, p=0.2):
    """Check 1: out bit-identical with the mask output; the mask's bits are the keep decisions (du of the mask backward == du of the
    Philox backward, bit for bit); de of the two agrees to the atomics' spread."""
    from hdmoe_hip._lib import call
    s = _setup(case, p)
    assert torch.equal(s["h"], s["h0"])
    kept = float((s["h"] != 0).float().mean())
    bits = (s["mask"].view(-1, 1).int() >> torch.arange(8, device="cuda").view(1, 8)) & 1
    assert abs(float(bits.float().mean()) - (1 - p)) < 0.01 and kept < float(bits.float().mean()) + 1e-6      # (u == 0 kept but h == 0)
    zero_kept = (s["u"] == 0) & (bits.view(s["u"].shape) == 1)
    assert int(zero_kept.sum()) > 0
    (dx, du, de, _), (_, _, de2, _) = s["unfused"]
    du_m, de_m = torch.empty_like(du), torch.zeros_like(de)
    call("hdmoe_film_silu_mask_bwd", du_m, de_m, dx, s["u"], s["e"], s["mask"], s["N"], s["HW"], s["C"], p, 1)
    assert torch.equal(du_m, du)
    assert float((du[zero_kept].float() != 0).float().mean()) > 0.5      # exact zeros of u carry a gradient
    ref, norm = _de_fp64(s, dx)
    err = lambda d: float(((d.double() - ref).abs() / norm).max())
    print(f"case {case} p {p}: standalone de err {err(de):.3e}, mask variant {err(de_m):.3e}, run-to-run {float(((de - de2).double().abs() / norm).max()):.3e}")
    assert err(de_m) <= 2 * max(err(de), err(de2), float(((de - de2).double().abs() / norm).max()))


@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_fused_epilogue_against_the_two_launches(gpu, case, p):
    """Checks 2 - 5: du bit-identical, weight gradients within the two-launch form's own run-to-run difference, de against fp64,
    two fused runs bit-identical, HDMOE_SEL_FILM_DGRAD counted once per fused launch and not at all outside the domain."""
    s = _setup(case, p)
    (dx, du, de, Gs), (_, du2, de2, Gs2) = s["unfused"]
    assert torch.equal(du, du2)
    rc, du_f, de_f, Gs_f, sel = s["fused"]()
    if not CASES[case][5]:
        assert rc == 1 and sel == {}, (rc, sel)                      # declined: nothing launched, no counter moved
        return
    assert rc == 0 and sel.get("film_dgrad") == 1, sel
    assert sel.get("bwd7_32" if s["R"] == 32 else "bwd7_16_ot2") == 1, sel
    rc2, du_f2, de_f2, _, sel2 = s["fused"]()
    torch.cuda.synchronize()
    assert rc2 == 0 and sel2.get("film_dgrad") == 1
    assert torch.isfinite(du_f.float()).all() and torch.isfinite(de_f).all()
    assert torch.equal(du_f, du), f"du differs in {int((du_f != du).sum())} elements"
    assert torch.equal(du_f2, du) and torch.equal(de_f2, de_f)
    for a, b, c in zip(Gs_f, Gs, Gs2):
        assert float((a - b).abs().max()) <= float((b - c).abs().max()), "weight gradient moved by more than the two-launch run-to-run difference"
    ref, norm = _de_fp64(s, dx)
    err = lambda d: float(((d.double() - ref).abs() / norm).max())
    spread = float(((de - de2).double().abs() / norm).max())
    print(f"case {case} p {p}: de err fused {err(de_f):.3e}, standalone {err(de):.3e} / {err(de2):.3e}, standalone run-to-run {spread:.3e}")
    assert err(de_f) <= 2 * max(err(de), err(de2), spread)


@pytest.mark.parametrize("train", [True, False])
def test_unet_block_backward_fused_against_unfused(gpu, train):
    """Check 6: unet_block_bank_forward at case a's size with ops.FILM_DGRAD on and off -- dx and the conv weight gradients as in checks
    2 and 3, the FiLM vector's gradient as in check 4 (fp64 from the tensors of the unfused run)."""
    import hdmoe_hip
    from hdmoe_hip import ops, bank as wbank
    from models.model_components import Unet_block, unet_block_bank_forward
    N, R, C, ks, split, _ = CASES["a"]
    torch.manual_seed(7)
    blocks = torch.nn.ModuleList([Unet_block(C, C, (k, k), 64, Type="enc", Dropout=0.2) for k in ks]).cuda()
    blocks.train(train)
    x = torch.randn(N, R, R, C, device="cuda").bfloat16()
    film = 1.0 + 0.3 * torch.randn(N, C, device="cuda")
    gy = torch.randn(N, R, R, C, device="cuda").bfloat16()
    seg = torch.tensor([0] + list(split), dtype=torch.int32, device="cuda")
    params = [q for b in blocks for q in (b.conv_res1.weights, b.conv_res2.weights)]
    out, cap = {}, {}
    saved = ops.FILM_DGRAD
    try:
        for mode in ("warm", "fused", "unfused", "unfused2"):
            ops.FILM_DGRAD = mode == "fused"
            hdmoe_hip.manual_seed(31)
            ops.STATS.clear()
            before = ops.kernel_selections()
            wbank.bank_for(blocks).begin_step(False)
            xx, ff = x.clone().requires_grad_(True), film.clone().requires_grad_(True)
            orig = ops.mp_conv_film

            def spy(*a, **k):
                h = orig(*a, **k)
                cap["rec"] = h._film_rec
                h.register_hook(lambda g: cap.__setitem__("g", g.detach().clone()))
                return h
            ops.mp_conv_film = spy if mode == "unfused" else orig
            try:
                y = unet_block_bank_forward(list(blocks), xx, None, seg, film=ff)
            finally:
                ops.mp_conv_film = orig
            y.backward(gy)
            wbank.deactivate()
            torch.cuda.synchronize()
            sel = _delta(before, ops.kernel_selections())
            assert sel.get("film_dgrad", 0) == (1 if mode == "fused" else 0) and ops.STATS["film_dgrad"] == (1 if mode == "fused" else 0), (mode, sel)
            out[mode] = (y.detach().clone(), xx.grad.clone(), ff.grad.clone(), [q.grad.clone() for q in params])
            for q in params:
                q.grad = None
    finally:
        ops.FILM_DGRAD = saved
    (y1, dx1, de1, dw1), (y2, dx2, de2, dw2), (_, _, de3, dw3) = out["fused"], out["unfused"], out["unfused2"]
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    for a, b, c in zip(dw1, dw2, dw3):
        assert float((a - b).abs().max()) <= float((b - c).abs().max())
    rec = cap["rec"]
    s = dict(u=rec.u, e=rec.e, mask=rec.mask, p=rec.p)
    assert (rec.mask is not None) == train
    ref, norm = _de_fp64(s, cap["g"])
    err = lambda d: float(((d.double() - ref).abs() / norm).max())
    spread = float(((de2 - de3).double().abs() / norm).max())
    print(f"block train={train}: de err fused {err(de1):.3e}, unfused {err(de2):.3e} / {err(de3):.3e}, run-to-run {spread:.3e}")
    assert err(de1) <= 2 * max(err(de2), err(de3), spread)


# ------------------------------------------------------------------------------------------------ the hand-off between the two nodes
# ops._FilmRec carries du / de from the conv layer's backward launch to the FiLM node.  The paths below are the ones beside the
# ordinary single consumer: all at case a's size, bf16, weight bank active, film_silu and mp_conv called directly.
class _Handoff:
    """h = film_silu(u, e, p) followed by bank conv layers (kernels of case a) over fresh leaves; every step draws the same dropout bits."""

    def __init__(self, p):
        import hdmoe_hip
        from hdmoe_hip import ops, bank as wbank
        N, R, C, ks, split, _ = CASES["a"]
        g = torch.Generator().manual_seed(77)
        self.ops, self.wbank, self.hd, self.p = ops, wbank, hdmoe_hip, p
        self.u = torch.randn(N, R, R, C, generator=g).bfloat16().cuda()
        self.e = (1.0 + 0.3 * torch.randn(N, C, generator=g)).cuda()
        self.gy = torch.randn(N, R, R, C, generator=g).bfloat16().cuda()
        self.seg = torch.tensor([0] + list(split), dtype=torch.int32, device="cuda")
        self.mod = torch.nn.ModuleList([torch.nn.ParameterList([torch.nn.Parameter(torch.randn(C, C, k, k, generator=g).cuda()) for k in ks])
                                        for _ in range(2)])
        self.step(lambda t: None, convs=2)                          # registers the layers: the bank has them ready from the next step on

    def step(self, backward, film_dgrad=True, convs=1):
        """(h, outputs of ``convs`` conv layers over h, the leaves u and e) handed to ``backward``; returns (du, de, STATS, entry points called)."""
        from hdmoe_hip import _lib
        ops = self.ops
        saved = ops.FILM_DGRAD
        ops.FILM_DGRAD = film_dgrad
        self.hd.manual_seed(31)
        ops.STATS.clear()
        self.wbank.bank_for(self.mod).begin_step(False)
        uu, ee = self.u.clone().requires_grad_(True), self.e.clone().requires_grad_(True)
        _lib.CALL_LOG = []
        try:
            h = ops.film_silu(uu, ee, self.p, True)
            ys = [ops.mp_conv(h, list(self.mod[i]), 1.0, seg=self.seg) for i in range(convs)]
            backward(dict(h=h, ys=ys, u=uu, e=ee, gy=self.gy))
            torch.cuda.synchronize()
            names = [n for n, _ in _lib.CALL_LOG]
        finally:
            _lib.CALL_LOG = None
            ops.FILM_DGRAD = saved
            self.wbank.deactivate()
        return uu.grad, ee.grad, dict(ops.STATS), names


def _full(t):
    torch.autograd.backward(t["ys"], [t["gy"]] * len(t["ys"]))


@pytest.mark.parametrize("p", P_DROP)
def test_two_conv_consumers_leave_the_film_backward_to_its_node(gpu, p):
    """h feeds two bank conv layers: neither backward launch takes the FiLM epilogue, the FiLM node runs its own kernel, and du is that of
    the same graph with ops.FILM_DGRAD off, bit for bit.  de is NOT compared bit for bit: the node's own kernel sums it with float atomics
    and two runs of one setting already differ (measured 4.6e-5 .. 6.5e-5 absolute here, with and without this hand-off code); it is held
    to the fp64 evaluation as in check 4 above."""
    s = _Handoff(p)
    cap = {}

    def spied(t):
        cap["rec"] = t["h"]._film_rec
        t["h"].register_hook(lambda g: cap.__setitem__("g", g.detach().clone()))
        _full(t)
    du, de, stats, names = s.step(spied, convs=2)
    du0, de0, stats0, names0 = s.step(_full, film_dgrad=False, convs=2)
    _, de1, _, _ = s.step(_full, film_dgrad=False, convs=2)
    own = "hdmoe_film_silu_mask_bwd" if p > 0 else "hdmoe_film_silu_bwd"
    assert stats.get("film_dgrad", 0) == 0 and stats.get("bwd6") == 2, stats
    assert names.count(own) == 1 and "hdmoe_conv_bwd6_film" not in names and names.count("hdmoe_conv_bwd6") == 2
    assert names == names0 and stats == stats0
    assert torch.isfinite(du.float()).all() and torch.isfinite(de).all()
    assert torch.equal(du, du0), f"du differs in {int((du != du0).sum())} elements"
    rec = cap["rec"]
    with torch.no_grad():
        ref, norm = _de_fp64(dict(u=rec.u, e=rec.e, mask=rec.mask, p=rec.p), cap["g"])
    err = lambda d: float(((d.double() - ref).abs() / norm).max())
    spread = float(((de0 - de1).double().abs() / norm).max())
    print(f"two consumers p {p}: max |de - de0| {float((de - de0).abs().max()):.3e}; de err {err(de):.3e}, FILM_DGRAD off {err(de0):.3e} / {err(de1):.3e}, run-to-run {spread:.3e}")
    assert err(de) <= 2 * max(err(de0), err(de1), spread)


def test_foreign_second_consumer_raises_and_leaves_the_next_step_alone(gpu):
    """h feeds one bank conv layer and h.float().sum(): the backward raises the error that names ops.FILM_DGRAD, and an ordinary step on
    fresh tensors afterwards gives what a step that never saw the error gives, bit for bit."""
    s = _Handoff(0.2)
    du0, de0, stats0, _ = s.step(_full)
    assert stats0.get("film_dgrad") == 1, stats0

    def foreign(t):
        z = t["h"].float().sum()
        torch.autograd.backward([t["ys"][0], z], [t["gy"], torch.ones_like(z)])
    with pytest.raises(RuntimeError, match=r"ops\.FILM_DGRAD"):
        s.step(foreign)
    du, de, stats, _ = s.step(_full)
    assert stats.get("film_dgrad") == 1, stats
    assert torch.equal(du, du0) and torch.equal(de, de0)


def test_partial_pass_leaves_nothing_behind(gpu):
    """autograd.grad(y, h) ends before the FiLM node and leaves the conv launch's hand-off unclaimed; the full backward over the same graph
    then returns du (bit for bit) and de (within its run-to-run spread) of a graph that never saw the partial pass."""
    s = _Handoff(0.2)
    du0, de0, _, _ = s.step(_full)
    du1, de1, _, _ = s.step(_full)

    def partial_then_full(t):
        torch.autograd.grad(t["ys"][0], t["h"], t["gy"], retain_graph=True)
        assert t["u"].grad is None and t["e"].grad is None
        _full(t)
    du, de, stats, names = s.step(partial_then_full)
    assert stats.get("film_dgrad") == 2 and names.count("hdmoe_conv_bwd6_film") == 2, (stats, names)
    assert "hdmoe_film_silu_mask_bwd" not in names
    spread = float((de0 - de1).abs().max())
    print(f"partial pass: du differs in {int((du != du0).sum())} elements, max |de - de0| {float((de - de0).abs().max()):.3e}, run-to-run {spread:.3e}")
    assert torch.equal(du, du0)
    assert float((de - de0).abs().max()) <= spread


def test_two_backward_passes_over_one_graph(gpu):
    """Two full backward passes with retain_graph: the same du bit for bit, and both take the FiLM epilogue."""
    s = _Handoff(0.2)
    got = []

    def twice(t):
        for keep in (True, False):
            torch.autograd.backward(t["ys"], [t["gy"]], retain_graph=keep)
            got.append(t["u"].grad.clone())
            t["u"].grad = None
    _, _, stats, names = s.step(twice)
    assert stats.get("film_dgrad") == 2 and names.count("hdmoe_conv_bwd6_film") == 2, (stats, names)
    assert torch.isfinite(got[0].float()).all() and torch.equal(got[0], got[1])
