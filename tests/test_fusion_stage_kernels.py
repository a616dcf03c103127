"""The fused token-local chains of the fusion stage (csrc/fusion.hip: hdmoe_fusion_in_fwd / _bwd, hdmoe_fusion_out_fwd / _bwd) -- GPU.

Each fused entry point and the unfused launches it replaces run on the same inputs and the same weight images, and both are compared
with a float64 evaluation of the chain on the CPU that rounds to bf16 wherever the unfused chain stores a tensor.
in chain:
  forward   t = fv - fu, d = sw[n] t, query = fu + d, ctx = fv - d, q = Wq query, k = Wk ctx, v = Wv ctx
  backward  dqx = Wq^T dq, dquery = dqx + gquery, dkx = Wk^T dk, dvx = Wv^T dv, dctx = dkx + dvx, dd = dquery - dctx, dt = sw[n] dd,
            dfu = dquery - dt, dfv = dctx + dt, dsw[n] = sum over the sample's rows and channels of dd t
  unfused: hdmoe_axpby, hdmoe_scale_rows_fwd, hdmoe_conv_fwd; hdmoe_pw_bwd (its input gradient), torch's bf16 `+` for the gradient
  fan-ins (what autograd launches), hdmoe_axpby and hdmoe_scale_rows_bwd.
out chain:
  forward   at = ao Wo o2 + bo a, a2 = a + alpha (at - a), cat = [wa U | wb a2], g1 = W1 cat, s = mp_silu(g1), l = W2 s, gate = softmax(l),
            mixed = k (U + gate0 U + gate1 a2)
  backward  gate_mix backward -> dU', dA', dl; ds = W2^T dl, dg1 = ds mp_silu'(g1), dcat = W1^T dg1, dU = dU' + wa dcat[:32],
            da2 = dA' + wb dcat[32:], dat = alpha da2, dalpha = <da2, at - a>, do2 = ao Wo^T dat, da = (1 - alpha) da2 + bo dat
  unfused: hdmoe_conv_fwd (with and without the residual epilogue, and on gate2's flipped image), hdmoe_lerp_param_*, hdmoe_cat2_*,
  hdmoe_mp_silu_*, hdmoe_gate_mix_*, hdmoe_pw_bwd, hdmoe_axpby, torch's bf16 `+`.

Bound.  Both chains differ from the float64 evaluation only where an fp32 value lies so close to a bf16 rounding boundary that its fp32
error decides the rounding: the element then moves by one bf16 ulp, and what is computed from it moves with it.  The elementwise
arithmetic of the in chain is the same in both, so query and ctx must agree bit for bit between them.  The projections may add their 32
or 64 products in another order, so other elements may flip; per output tensor the fused kernel's largest error may be MARGIN = 2 times
the unfused chain's own largest error (measured in the same run, never taken from the fused output).  Where the unfused chain happens to
meet float64 in every element (the one-tile shapes) there is no such error to scale: every element must then lie within one bf16 ulp of
its own reference value, 2^-7 |r|.  The kernels are built to form their sums as the unfused kernels do (same MFMA shape and operand order,
the gate row sums and the residual epilogue in those kernels' order), so in addition every bf16 output must be bit-equal to the unfused
chain's: the count of differing elements is asserted to be 0.  For the
reductions (dsw, dalpha) the bound is MARGIN times the unfused launch's error plus the reduction bound of
tests/test_elementwise_kernels.py, 8 u (|r| + sum |terms|),
u = 2^-24: their terms carry the flips above, so against the float64 sum of the REFERENCE's terms they can be held to the unfused
launches' own error and the reduction's, not to the reduction's alone.  Held to the reduction's bound alone they are on exact data,
below.
Measured on the MI355X, largest error over max|reference| per output, worst over the shapes, unfused / fused:
  query, ctx 0 / 0 (bit-equal);  q 7.4e-4 / 7.4e-4;  k 1.4e-3 / 1.4e-3;  v 1.7e-4 / 1.7e-4;  dfu 1.8e-3 / 1.8e-3;  dfv 1.9e-3 / 1.9e-3;
  dsw 3.1e-5 / 3.1e-5;  a2 1.5e-3 / 1.5e-3;  cat 1.4e-3 / 1.4e-3;  g1 2.8e-3 / 2.8e-3;  s 1.7e-3 / 1.7e-3;  gate 1.7e-3 / 1.7e-3;
  mixed 3.0e-3 / 3.0e-3;  dl 2.5e-3 / 2.5e-3;  dg1 2.1e-3 / 2.1e-3;  dU 2.3e-3 / 2.3e-3;  dat 4.1e-3 / 4.1e-3;  do2 2.4e-3 / 2.4e-3;
  da 4.0e-3 / 4.0e-3;  dalpha 3.9e-5 / 1.5e-5.
Every bf16 output's fused error equals the unfused one and no element differed between the two chains at any shape; only the fp32
reductions dsw and dalpha differ in their last bits.  So the margin in use is 1; 2 leaves room for another summation order in the
float64 comparison should the bit-equality assertion ever be lifted.

Both reductions are also checked on data where the terms are the same numbers in the kernel and in float64, against the float64 sum
within 8 u (|r| + sum |terms|) alone.  dsw: values in {-2, 0, 2} for the gradients and fu / fv, weight images with entries in
{-1, 0, 1} and sw = 0.5 make every intermediate an integer below 256, exact in bf16 (measured: exact).  dalpha: see
test_dalpha_reduction_on_exact_data (measured: exact as well).

Shapes (C = 32).  in chain: (B, S) = (1, 32) one tile of 32 rows; (3, 100) 300 rows -- a partial last tile and sample boundaries
inside tiles, so sw[n] / dsw[n] indexing matters; (2, 1024) 64 tiles, 16 workgroups; each with and without sw and with and without
gquery / gctx.  out chain: 32, 300 and 2048 rows, with and without dgate.  The grid is capped at 2048 workgroups of four tiles (1024
for the out backward), so the grid-stride loops (and the in kernels' prefetch of the next tile) run only above 262,144 rows:
(260, 1024) = 266,240 rows = 8320 tiles, once per chain, on the full chain.
Every tensor lives in an allocation with guard rows on either side: inputs must be unchanged, the guards of outputs keep their fill.
A base pointer 8 bytes off must be refused (return 1) with nothing written.

End to end: _fusion_tail forward + backward at B = 2 on the wide_config1 fixture's weights with ops.FUSION_FUSED True and False:
outputs within 3e-2 and the cross_attn* / gate* / alpha_txt gradients within 6e-2 of the tensor's maximum (the bf16 tolerances of
tests/test_hip_parity.py test_full_model_real_widths), the four selection counters moving on the fused run only.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
MARGIN = 2.0
GUARD = 8                                                    # rows
FILL = 1234.0                                                # exactly representable in bf16
SHAPES = [(1, 32), (3, 100), (2, 1024), (260, 1024)]


@pytest.fixture(scope="module")
def call():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    return call


class Guarded:
    """A (rows, 32) bf16 tensor inside an allocation with GUARD rows of FILL on either side."""

    def __init__(self, rows, value=None):
        self.buf = torch.full((rows + 2 * GUARD, 32), FILL, dtype=BF16, device=DEV)
        self.t = self.buf[GUARD:GUARD + rows]
        if value is not None:
            self.t.copy_(value)
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int16), self.before.view(torch.int16))

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        return bool((g == FILL).all())


def rb(x):
    """float64 -> the float64 value of its bf16 rounding (a storage point of the chain)."""
    return x.to(BF16).double()


def _inputs(B, S, seed, exact=False):
    g = torch.Generator().manual_seed(seed)
    rows = B * S
    if exact:
        draw = lambda *s: 2.0 * torch.randint(-1, 2, s, generator=g).to(F32)
        w = lambda: torch.randint(-1, 2, (32, 32), generator=g).to(F32)
        sw = torch.full((B,), 0.5)
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
        w = lambda: torch.randn(32, 32, generator=g) / 32 ** 0.5
        sw = torch.rand(B, generator=g)
    d = {n: draw(rows, 32).to(BF16) for n in ("fu", "fv", "dq", "dk", "dv", "gquery", "gctx")}
    d.update({n: w().to(BF16) for n in ("wq", "wk", "wv")})
    d["sw"] = sw.to(F32)
    return d


def _reference(d, B, S, use_sw, use_g):
    """The chain in float64 with bf16 rounding at the storage points."""
    f = {k: v.double() for k, v in d.items()}
    swr = f["sw"].repeat_interleave(S)[:, None]
    if use_sw:
        t = rb(f["fv"] - f["fu"])
        dd_ = rb(swr * t)
        query, ctx = rb(f["fu"] + dd_), rb(f["fv"] - dd_)
    else:
        query, ctx = f["fu"], f["fv"]
    out = dict(query=query, ctx=ctx, q=rb(query @ f["wq"].T), k=rb(ctx @ f["wk"].T), v=rb(ctx @ f["wv"].T))
    dquery = rb(f["dq"] @ f["wq"])
    if use_g:
        dquery = rb(dquery + f["gquery"])
    dctx = rb(rb(f["dk"] @ f["wk"]) + rb(f["dv"] @ f["wv"]))
    if use_g:
        dctx = rb(dctx + f["gctx"])
    if use_sw:
        dd = rb(dquery - dctx)
        dt = rb(swr * dd)
        out.update(dfu=rb(dquery - dt), dfv=rb(dctx + dt), dsw=(dd * t).reshape(B, S * 32).sum(1),
                   dsw_scale=(dd * t).abs().reshape(B, S * 32).sum(1))
    else:
        out.update(dfu=dquery, dfv=dctx)
    return out


def _fused(call, T, W, sw, rows, S, use_g):
    o = {n: Guarded(rows) for n in ("query", "ctx", "q", "k", "v", "dfu", "dfv")}
    has = sw is not None
    rc = call("hdmoe_fusion_in_fwd", T["fu"].t, T["fv"].t, sw, W["wq"], W["wk"], W["wv"], o["query"].t if has else None,
              o["ctx"].t if has else None, o["q"].t, o["k"].t, o["v"].t, rows, S, 32, 1.0, 1.0, 1.0, 1)
    assert rc == 0, "hdmoe_fusion_in_fwd declined a shape of its domain"
    dsw = torch.zeros(sw.numel() + 2, dtype=F32, device=DEV) if has else None
    rc = call("hdmoe_fusion_in_bwd", T["dq"].t, T["dk"].t, T["dv"].t, T["gquery"].t if use_g else None, T["gctx"].t if use_g else None,
              T["fu"].t if has else None, T["fv"].t if has else None, sw, W["wdq"], W["wdk"], W["wdv"], o["dfu"].t, o["dfv"].t,
              dsw[1:-1] if has else None, rows, S, 32, 1.0, 1.0, 1.0, 1)
    assert rc == 0, "hdmoe_fusion_in_bwd declined a shape of its domain"
    torch.cuda.synchronize()
    for n, gt in o.items():
        assert gt.guards_intact(), f"fused: guard rows of {n} overwritten"
    if not has:
        assert o["query"].unchanged() and o["ctx"].unchanged(), "fused: query / ctx written without sw"
    res = {n: gt.t.clone() for n, gt in o.items() if has or n not in ("query", "ctx")}
    if has:
        assert float(dsw[0]) == 0.0 and float(dsw[-1]) == 0.0, "fused: dsw written out of range"
        res["dsw"] = dsw[1:-1].clone()
    return res


def _unfused(call, T, W, sw, rows, S, use_g):
    """The launches ops.py makes for the same chain today, on the same buffers."""
    new = lambda: torch.empty(rows, 32, dtype=BF16, device=DEV)
    n = rows * 32
    fu, fv = T["fu"].t, T["fv"].t
    has = sw is not None

    def conv(x, w):
        y = new()
        call("hdmoe_conv_fwd", x, w, y, None, 1.0, 0.0, None, 1, 1024, 1, 1, rows, 1, rows, 32, 32, 32, 32, 32, 1, 0, [1], [1], [0], [0], 1)
        return y

    def dgrad(x, dy, wd):
        dx, G = new(), torch.zeros(1024, dtype=F32, device=DEV)
        assert call("hdmoe_pw_bwd", x, dy, wd, dx, [G], None, 1, 1024, 1, rows, 32, 32, 1.0, 1) == 0
        return dx

    def axpby(x, y, a, b):
        o = new()
        call("hdmoe_axpby", o, x, y, a, b, n, 1)
        return o

    res = {}
    if has:
        t = axpby(fv, fu, 1.0, -1.0)
        d = new()
        call("hdmoe_scale_rows_fwd", d, t, sw, sw.numel(), S * 32, 1)
        query, ctx = axpby(fu, d, 1.0, 1.0), axpby(fv, d, 1.0, -1.0)
        res.update(query=query, ctx=ctx)
    else:
        query, ctx = fu, fv
    res.update(q=conv(query, W["wq"]), k=conv(ctx, W["wk"]), v=conv(ctx, W["wv"]))
    dquery = dgrad(query, T["dq"].t, W["wdq"])
    if use_g:
        dquery = dquery + T["gquery"].t
    dctx = dgrad(ctx, T["dk"].t, W["wdk"]) + dgrad(ctx, T["dv"].t, W["wdv"])
    if use_g:
        dctx = dctx + T["gctx"].t
    if has:
        dd = dquery + axpby(dctx, None, -1.0, 0.0)
        dt, dsw = new(), torch.zeros_like(sw)
        call("hdmoe_scale_rows_bwd", dt, dsw, dd, t, sw, sw.numel(), S * 32, 1)
        res.update(dfu=dquery + axpby(dt, None, -1.0, 0.0), dfv=dctx + dt, dsw=dsw)
    else:
        res.update(dfu=dquery, dfv=dctx)
    torch.cuda.synchronize()
    return res


def _setup(B, S, seed, exact=False):
    d = _inputs(B, S, seed, exact)
    rows = B * S
    T = {n: Guarded(rows, d[n].to(DEV)) for n in ("fu", "fv", "dq", "dk", "dv", "gquery", "gctx")}
    W = {n: d[n].to(DEV).contiguous() for n in ("wq", "wk", "wv")}
    W.update({"wd" + n[1]: d[n].t().contiguous().to(DEV) for n in ("wq", "wk", "wv")})       # the flipped image [I][O]
    return d, T, W, d["sw"].to(DEV), rows


def _check_output(tag, n, fused, plain, r, red_scale):
    """One output of a fused kernel against the float64 reference r, bounded by the unfused launches' own error (docstring, `Bound`)."""
    f64 = fused.cpu().double().reshape(r.shape)
    ef = float((f64 - r).abs().max())
    eu = float((plain.cpu().double().reshape(r.shape) - r).abs().max())
    mx = float(r.abs().max())
    ndiff = int((fused.reshape(-1) != plain.reshape(-1)).sum())
    assert torch.isfinite(fused).all(), tag
    if red_scale is not None:                                    # fp32 reduction (dsw, dalpha)
        bound = MARGIN * eu + float((8 * U * (r.abs() + red_scale)).max())
        print(f"{tag}: max|ref| {mx:.3e}  unfused err {eu:.3e} ({eu / mx:.2e})  fused err {ef:.3e} ({ef / mx:.2e})  bound {bound:.3e}")
        assert ef <= bound, (tag, ef, eu, bound)
        return
    print(f"{tag}: max|ref| {mx:.3e}  unfused err {eu:.3e} ({eu / mx:.2e})  fused err {ef:.3e} ({ef / mx:.2e})  "
          f"elements that differ from the unfused chain's: {ndiff}")
    if fused.dtype == BF16:
        assert ndiff == 0, f"{tag}: {ndiff} elements differ from the unfused chain's"
    if eu > 0.0:
        assert ef <= MARGIN * eu, (tag, ef, eu)
    else:                                                        # the unfused chain met float64 everywhere: one ulp of the element
        assert bool(((f64 - r).abs() <= 2.0 ** -7 * r.abs() + 2.0 ** -126).all()), (tag, ef)


CASES = [(B, S, use_sw, use_g) for (B, S) in SHAPES[:3] for use_sw in (True, False) for use_g in (True, False)] + [SHAPES[3] + (True, True)]


@pytest.mark.parametrize("B,S,use_sw,use_g", CASES, ids=[f"B{B}-S{S}-{'sw' if a else 'nosw'}-{'fanin' if b else 'nofanin'}" for B, S, a, b in CASES])
def test_fused_head_against_fp64_and_the_unfused_chain(call, B, S, use_sw, use_g):
    d, T, W, sw, rows = _setup(B, S, 1000 * B + S)
    sw_arg = sw if use_sw else None
    fused = _fused(call, T, W, sw_arg, rows, S, use_g)
    plain = _unfused(call, T, W, sw_arg, rows, S, use_g)
    for n, gt in T.items():
        assert gt.unchanged(), f"input {n} or its guard rows changed"
    ref = _reference(d, B, S, use_sw, use_g)
    assert set(fused) == set(plain)
    if use_sw:
        for n in ("query", "ctx"):
            assert torch.equal(fused[n].view(torch.int16), plain[n].view(torch.int16)), f"{n}: the elementwise arithmetic differs from the unfused chain's"
    for n in sorted(fused):
        _check_output(f"B={B} S={S} sw={use_sw} fanin={use_g} {n}", n, fused[n], plain[n], ref[n], ref.get("dsw_scale") if n == "dsw" else None)


@pytest.mark.parametrize("B,S", [(3, 100), (2, 1024)])
def test_dsw_reduction_on_exact_data(call, B, S):
    """Small-integer data: every intermediate is exact in bf16, so dsw is the fp32 reduction of exactly the float64 terms."""
    d, T, W, sw, rows = _setup(B, S, 77 * B + S, exact=True)
    fused = _fused(call, T, W, sw, rows, S, True)
    ref = _reference(d, B, S, True, True)
    for n in ("query", "ctx", "q", "k", "v", "dfu", "dfv"):
        assert torch.equal(fused[n].cpu().double(), ref[n]), f"{n}: exact data, inexact result"
    err = (fused["dsw"].cpu().double() - ref["dsw"]).abs()
    bound = 8 * U * (ref["dsw"].abs() + ref["dsw_scale"]) + 2.0 ** -126
    print(f"B={B} S={S} dsw: worst |err| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (err, bound)


def test_misaligned_base_is_refused(call):
    B, S = 1, 40
    d, T, W, sw, rows = _setup(B, S, 5)
    big = {n: torch.full((rows * 32 + 8,), FILL, dtype=BF16, device=DEV) for n in ("fu", "q", "dfu")}
    off = {n: v[4:4 + rows * 32] for n, v in big.items()}                            # 8 bytes off a 16-byte boundary
    outs = {n: Guarded(rows) for n in ("query", "ctx", "q", "k", "v", "dfu", "dfv")}
    a = lambda n: outs[n].t
    assert call("hdmoe_fusion_in_fwd", off["fu"], T["fv"].t, sw, W["wq"], W["wk"], W["wv"], a("query"), a("ctx"), a("q"), a("k"), a("v"),
                rows, S, 32, 1.0, 1.0, 1.0, 1) == 1
    assert call("hdmoe_fusion_in_fwd", T["fu"].t, T["fv"].t, sw, W["wq"], W["wk"], W["wv"], a("query"), a("ctx"), off["q"], a("k"), a("v"),
                rows, S, 32, 1.0, 1.0, 1.0, 1) == 1
    dsw = torch.zeros(B, dtype=F32, device=DEV)
    assert call("hdmoe_fusion_in_bwd", T["dq"].t, T["dk"].t, T["dv"].t, None, None, T["fu"].t, T["fv"].t, sw, W["wdq"], W["wdk"], W["wdv"],
                off["dfu"], a("dfv"), dsw, rows, S, 32, 1.0, 1.0, 1.0, 1) == 1
    # outside the domain for another reason: fp32 tensors, 64 channels
    assert call("hdmoe_fusion_in_fwd", T["fu"].t, T["fv"].t, sw, W["wq"], W["wk"], W["wv"], a("query"), a("ctx"), a("q"), a("k"), a("v"),
                rows, S, 32, 1.0, 1.0, 1.0, 0) == 1
    assert call("hdmoe_fusion_in_fwd", T["fu"].t, T["fv"].t, sw, W["wq"], W["wk"], W["wv"], a("query"), a("ctx"), a("q"), a("k"), a("v"),
                rows // 2, S, 64, 1.0, 1.0, 1.0, 1) == 1
    torch.cuda.synchronize()
    assert all(o.unchanged() for o in outs.values()) and float(dsw.abs().sum()) == 0.0
    assert all(bool((v == FILL).all()) for v in big.values())


# ------------------------------------------------------------------------------------------------------------------ the out chain
def _f32(v):
    return float(torch.tensor(float(v), dtype=F32))


AO = BO = _f32(0.5 / (0.5 ** 2 + 0.5 ** 2) ** 0.5)          # out_proj's alpha, beta at attn_balance 0.5, as the C ABI passes them
WA = WB = 1.0                                                # mp_cat(U, a2, 0.5) of two 32-channel tensors
GK = _f32(0.70710678118654752)
AL = _f32(0.3)                                               # alpha_txt
DIV = 0.596


def _out_inputs(rows, seed):
    g = torch.Generator().manual_seed(seed)
    d = {n: torch.randn(rows, 32, generator=g).to(BF16) for n in ("o2", "a", "U", "dmixed")}
    d["dgate"] = torch.randn(rows, 2, generator=g)
    d["wo"] = (torch.randn(32, 32, generator=g) / 32 ** 0.5).to(BF16)
    d["w1"] = (torch.randn(32, 64, generator=g) / 8).to(BF16)
    d["w2"] = (torch.randn(2, 32, generator=g) / 32 ** 0.5).to(BF16)
    return d


def _out_reference(d, use_dgate, ao=None, bo=None, al=None):
    AO, BO, AL = (globals()["AO"] if ao is None else ao), (globals()["BO"] if bo is None else bo), (globals()["AL"] if al is None else al)
    f = {k: v.double() for k, v in d.items()}
    sig = lambda x: 1.0 / (1.0 + torch.exp(-x))
    at = rb(AO * (f["o2"] @ f["wo"].T) + BO * f["a"])
    a2 = rb(f["a"] + AL * (at - f["a"]))
    cat = torch.cat([rb(WA * f["U"]), rb(WB * a2)], 1)
    g1 = rb(cat @ f["w1"].T)
    s = rb(g1 * sig(g1) / DIV)
    lg = rb(s @ f["w2"].T)
    gate = torch.softmax(lg, 1)
    g0, gg1 = gate[:, :1], gate[:, 1:]
    out = dict(mixed=rb(GK * (f["U"] + g0 * f["U"] + gg1 * a2)), gate=gate, a2=a2, g1=g1, cat=cat, s=s)
    go = GK * f["dmixed"]
    dUm, dAm = rb(go * (1 + g0)), rb(go * gg1)
    dd = torch.stack([(go * f["U"]).sum(1), (go * a2).sum(1)], 1) + (f["dgate"] if use_dgate else 0.0)
    dot = (dd * gate).sum(1, keepdim=True)
    dl = rb(gate * (dd - dot))
    ds = rb(dl @ f["w2"])
    sg = sig(g1)
    dg1 = rb(ds * sg * (1 + g1 * (1 - sg)) / DIV)
    dcat = rb(dg1 @ f["w1"])
    dU = rb(dUm + rb(WA * dcat[:, :32]))
    da2 = rb(dAm + rb(WB * dcat[:, 32:]))
    dat = rb(AL * da2)
    terms = da2 * (at - f["a"])
    out.update(dl=dl, dg1=dg1, dU=dU, dat=dat, do2=rb(AO * (dat @ f["wo"])), da=rb(rb((1 - AL) * da2) + rb(BO * dat)),
               dalpha=terms.sum().reshape(1), dalpha_scale=terms.abs().sum().reshape(1))
    return out


def _out_setup(rows, seed):
    d = _out_inputs(rows, seed)
    T, W = _out_tensors(d, rows)
    return d, T, W, d["dgate"].to(DEV).contiguous(), torch.tensor([AL], dtype=F32, device=DEV)


def _out_tensors(d, rows):
    T = {n: Guarded(rows, d[n].to(DEV)) for n in ("o2", "a", "U", "dmixed")}
    W = dict(wo=d["wo"].to(DEV).contiguous(), w1=d["w1"].to(DEV).contiguous(), w2=d["w2"].to(DEV).contiguous(),
             wdo=d["wo"].t().contiguous().to(DEV), wd1=d["w1"].t().contiguous().to(DEV))
    wd2 = torch.zeros(32, 16, dtype=BF16)                    # the flipped image pads its output channels to 16
    wd2[:, :2] = d["w2"].t()
    W["wd2"] = wd2.to(DEV)
    return T, W


def _out_fused(call, T, W, dgate, alpha, rows, ao=AO, bo=BO):
    o = {n: Guarded(rows) for n in ("mixed", "a2", "g1", "s", "do2", "da", "dU", "dat", "dg1")}
    cat = torch.full((rows + 2 * GUARD, 64), FILL, dtype=BF16, device=DEV)
    gate = torch.full((rows + 2, 2), FILL, dtype=F32, device=DEV)
    dl = torch.full((rows + 2, 2), FILL, dtype=BF16, device=DEV)
    dal = torch.zeros(3, dtype=F32, device=DEV)
    k = (32, ao, bo, WA, WB, 1.0, 1.0, 1)
    t = lambda n: o[n].t
    assert call("hdmoe_fusion_out_fwd", T["o2"].t, T["a"].t, T["U"].t, alpha, W["wo"], W["w1"], W["w2"], t("mixed"), gate[1:-1], t("a2"),
                t("g1"), cat[GUARD:-GUARD], t("s"), rows, *k) == 0, "hdmoe_fusion_out_fwd declined a shape of its domain"
    assert call("hdmoe_fusion_out_bwd", T["dmixed"].t, dgate, gate[1:-1], T["U"].t, t("a2"), t("g1"), T["o2"].t, T["a"].t, alpha, W["wo"],
                W["wdo"], W["wd1"], W["wd2"], t("do2"), t("da"), t("dU"), t("dat"), t("dg1"), dl[1:-1], dal[1:2], rows, *k) == 0, \
        "hdmoe_fusion_out_bwd declined a shape of its domain"
    torch.cuda.synchronize()
    for n, gt in o.items():
        assert gt.guards_intact(), f"fused: guard rows of {n} overwritten"
    assert bool((cat[:GUARD] == FILL).all() and (cat[-GUARD:] == FILL).all()), "fused: guard rows of cat overwritten"
    assert bool((gate[0] == FILL).all() and (gate[-1] == FILL).all() and (dl[0] == FILL).all() and (dl[-1] == FILL).all())
    assert float(dal[0]) == 0.0 and float(dal[2]) == 0.0
    res = {n: gt.t.clone() for n, gt in o.items()}
    res.update(cat=cat[GUARD:-GUARD].clone(), gate=gate[1:-1].clone(), dl=dl[1:-1].clone(), dalpha=dal[1:2].clone())
    return res


def _out_unfused(call, T, W, dgate, alpha, rows):
    new = lambda c=32, dt=BF16: torch.empty(rows, c, dtype=dt, device=DEV)
    n = rows * 32
    o2, a, U, dm = T["o2"].t, T["a"].t, T["U"].t, T["dmixed"].t

    def conv(x, w, res, al, be, I, Ipad, O):
        y = new(O)
        call("hdmoe_conv_fwd", x, w, y, res, al, be, None, 1, w.numel(), 1, 1, rows, 1, rows, I, I, Ipad, O, O, 1, 0, [1], [1], [0], [0], 1)
        return y

    def pw_bwd(x, dy, wd, I, O, al):
        dx, G = new(I), torch.zeros(I * O, dtype=F32, device=DEV)
        assert call("hdmoe_pw_bwd", x, dy, wd, dx, [G], None, 1, I * O, 1, rows, I, O, al, 1) == 0
        return dx

    at = conv(o2, W["wo"], a, AO, BO, 32, 32, 32)
    a2 = new()
    call("hdmoe_lerp_param_fwd", a2, a, at, alpha, n, 1)
    cat = new(64)
    call("hdmoe_cat2_fwd", cat, U, a2, WA, WB, 32, 32, rows, 1)
    g1 = conv(cat, W["w1"], None, 1.0, 0.0, 64, 64, 32)
    s = new()
    call("hdmoe_mp_silu_fwd", s, g1, n, 1)
    lg = conv(s, W["w2"], None, 1.0, 0.0, 32, 32, 2)
    mixed, gate = new(), new(2, F32)
    call("hdmoe_gate_mix_fwd", mixed, gate, lg, U, a2, rows, 32, 1)
    dUm, dAm, dl = new(), new(), new(2)
    call("hdmoe_gate_mix_bwd", dUm, dAm, dl, dm, dgate, gate, U, a2, rows, 32, 1)
    ds = new()                                                   # gate2's input gradient: the general conv kernel on the flipped image
    call("hdmoe_conv_fwd", dl, W["wd2"], ds, None, 1.0, 0.0, None, 1, 512, 1, 1, rows, 1, rows, 2, 2, 16, 32, 32, 1, 0, [1], [1], [0], [0], 1)
    dg1 = new()
    call("hdmoe_mp_silu_bwd", dg1, ds, g1, n, 1)
    dcat = pw_bwd(cat, dg1, W["wd1"], 64, 32, 1.0)
    dUc, dAc = new(), new()
    call("hdmoe_cat2_bwd", dUc, dAc, dcat, WA, WB, 32, 32, rows, 1)
    dU, da2 = dUm + dUc, dAm + dAc
    dal_, dat, dalpha = new(), new(), torch.zeros(1, dtype=F32, device=DEV)
    call("hdmoe_lerp_param_bwd", dal_, dat, dalpha, da2, a, at, alpha, n, 1)
    do2 = pw_bwd(o2, dat, W["wdo"], 32, 32, AO)
    dres = new()
    call("hdmoe_axpby", dres, dat, None, BO, 0.0, n, 1)
    torch.cuda.synchronize()
    return dict(mixed=mixed, gate=gate, a2=a2, g1=g1, cat=cat, s=s, dl=dl, dg1=dg1, dU=dU, dat=dat, do2=do2, da=dal_ + dres, dalpha=dalpha)


OUT_CASES = [(32, True), (300, True), (300, False), (2048, True), (2048, False), (266240, True)]


@pytest.mark.parametrize("rows,use_dgate", OUT_CASES, ids=[f"rows{r}-{'dgate' if g else 'nodgate'}" for r, g in OUT_CASES])
def test_fused_tail_against_fp64_and_the_unfused_chain(call, rows, use_dgate):
    d, T, W, dgate, alpha = _out_setup(rows, 31 * rows + 7)
    dg = dgate if use_dgate else None
    fused = _out_fused(call, T, W, dg, alpha, rows)
    plain = _out_unfused(call, T, W, dg, alpha, rows)
    for n, gt in T.items():
        assert gt.unchanged(), f"input {n} or its guard rows changed"
    ref = _out_reference(d, use_dgate)
    assert set(fused) == set(plain)
    for n in sorted(fused):
        _check_output(f"rows={rows} dgate={use_dgate} {n}", n, fused[n], plain[n], ref[n], ref["dalpha_scale"] if n == "dalpha" else None)


def test_dalpha_reduction_on_exact_data(call):
    """Data on which the terms of dalpha = <da2, at - a> are the same numbers in the kernel and in float64, so that dalpha is held to the
    reduction bound alone: o2, a, U, dmixed in {-2, 0, 2}, out_proj's image in {-1, 0, 1} with alpha = beta = 1 (at = Wo o2 + a, an
    integer below 256), alpha_txt = 0.5 (a2 and dat exact), gate1's image zero (g1 = 0, both logits 0, the gate exactly 1/2, no share of
    mp_cat in da2), no dgate: da2 = bf16(k dmixed / 2) is one of 0, +-bf16(k), k = 0.7071..., nowhere near a rounding boundary."""
    rows = 2048
    g = torch.Generator().manual_seed(91)
    draw = lambda *sh: 2.0 * torch.randint(-1, 2, sh, generator=g).to(F32)
    d = {n: draw(rows, 32).to(BF16) for n in ("o2", "a", "U", "dmixed")}
    d["dgate"] = torch.zeros(rows, 2)
    d["wo"] = torch.randint(-1, 2, (32, 32), generator=g).to(BF16)
    d["w1"] = torch.zeros(32, 64, dtype=BF16)
    d["w2"] = (torch.randn(2, 32, generator=g) / 32 ** 0.5).to(BF16)
    T, W = _out_tensors(d, rows)
    alpha = torch.tensor([0.5], dtype=F32, device=DEV)
    fused = _out_fused(call, T, W, None, alpha, rows, ao=1.0, bo=1.0)
    ref = _out_reference(d, False, ao=1.0, bo=1.0, al=0.5)
    for n in ("a2", "dat", "da", "do2", "g1", "s"):
        assert torch.equal(fused[n].cpu().double(), ref[n]), f"{n}: exact data, another result than float64's"
    assert float(ref["dalpha_scale"]) > 100.0                     # (the case is not empty)
    err = float((fused["dalpha"].cpu().double() - ref["dalpha"]).abs())
    bound = 8 * U * float(ref["dalpha"].abs() + ref["dalpha_scale"]) + 2.0 ** -126
    print(f"rows={rows} dalpha {float(ref['dalpha']):.6e}: |err| {err:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}")
    assert err <= bound, (err, bound)


def test_fused_tail_misaligned_base_is_refused(call):
    rows = 40
    d, T, W, dgate, alpha = _out_setup(rows, 3)
    outs = {n: Guarded(rows) for n in ("mixed", "a2", "g1", "s", "do2", "da", "dU", "dat", "dg1")}
    cat, gate, dl = torch.empty(rows, 64, dtype=BF16, device=DEV), torch.zeros(rows, 2, dtype=F32, device=DEV), torch.zeros(rows, 2, dtype=BF16, device=DEV)
    dal = torch.zeros(1, dtype=F32, device=DEV)
    big = torch.full((rows * 32 + 8,), FILL, dtype=BF16, device=DEV)
    off = big[4:4 + rows * 32]                                                      # 8 bytes off a 16-byte boundary
    k = (32, AO, BO, WA, WB, 1.0, 1.0, 1)
    t = lambda n: outs[n].t
    assert call("hdmoe_fusion_out_fwd", off, T["a"].t, T["U"].t, alpha, W["wo"], W["w1"], W["w2"], t("mixed"), gate, t("a2"), t("g1"), cat, t("s"),
                rows, *k) == 1
    assert call("hdmoe_fusion_out_fwd", T["o2"].t, T["a"].t, T["U"].t, alpha, W["wo"], W["w1"], W["w2"], off, gate, t("a2"), t("g1"), cat, t("s"),
                rows, *k) == 1
    assert call("hdmoe_fusion_out_bwd", T["dmixed"].t, None, gate, T["U"].t, t("a2"), t("g1"), T["o2"].t, T["a"].t, alpha, W["wo"], W["wdo"], W["wd1"],
                W["wd2"], t("do2"), off, t("dU"), t("dat"), t("dg1"), dl, dal, rows, *k) == 1
    assert call("hdmoe_fusion_out_fwd", T["o2"].t, T["a"].t, T["U"].t, alpha, W["wo"], W["w1"], W["w2"], t("mixed"), gate, t("a2"), t("g1"), cat, t("s"),
                rows, 32, AO, BO, WA, WB, 1.0, 1.0, 0) == 1                          # fp32: outside the domain
    torch.cuda.synchronize()
    assert all(o.unchanged() for o in outs.values()) and bool((big == FILL).all()) and float(dal) == 0.0 and float(gate.abs().sum()) == 0.0


def _tail_run(fused_flag):
    import hdmoe_hip
    from hdmoe_hip import bank as wbank
    from hdmoe_hip import ops
    from conftest import wide_setup
    g = torch.load(os.path.join(ROOT, "tests", "golden", "wide_config1.pt"), weights_only=False)
    hdmoe_hip.set_compute_dtype(BF16)
    old = ops.FUSION_FUSED
    ops.FUSION_FUSED = fused_flag
    try:
        variant, model, kw, state, inp = wide_setup(g)
        model.load_state_dict(state)
        model = model.to(DEV).train()
        net = model.net
        B, R, C = 2, kw["IN_img_resolution"], net.internal_channels
        gen = torch.Generator().manual_seed(11)
        mk = lambda *s: torch.randn(*s, generator=gen).to(DEV)
        out_u, out_v = mk(B, R, R, C).to(BF16).requires_grad_(True), mk(B, R, R, C).to(BF16).requires_grad_(True)
        s_vit, s_unet = (1.0 + 0.1 * mk(B)).requires_grad_(True), (1.0 - 0.1 * mk(B)).requires_grad_(True)
        text = mk(B, 77, kw["text_emb_dim"]).to(BF16)
        gy, ggate = mk(B, R, R, kw["IN_in_channels"]), mk(B, R, R, 2)
        sel0 = ops.kernel_selections()
        for step in range(2):                                     # the first step registers the layers with the weight bank
            for t in (out_u, out_v, s_vit, s_unet):
                t.grad = None
            model.zero_grad(set_to_none=False)
            wbank.bank_for(model).begin_step(True)
            try:
                out, gate = net._fusion_tail(out_u, out_v, s_vit, s_unet, text, alpha_routing=10)
            finally:
                wbank.deactivate()
            torch.autograd.backward([out, gate], [gy.to(out.dtype), ggate.to(gate.dtype)])
        torch.cuda.synchronize()
        sel1 = ops.kernel_selections()
        res = dict(out=out.detach().float().cpu(), gate=gate.detach().float().cpu(), d_out_u=out_u.grad.float().cpu(), d_out_v=out_v.grad.float().cpu(),
                   d_s_vit=s_vit.grad.float().cpu(), d_s_unet=s_unet.grad.float().cpu())
        for n, p in net.named_parameters():
            if n.split(".")[0] in ("cross_attn", "cross_attn_text", "gate1", "gate2", "alpha_txt") and p.grad is not None:
                res["grad:" + n] = p.grad.detach().float().cpu().clone()
        return res, {k: sel1[k] - sel0[k] for k in ("fusion_in", "fusion_in_bwd", "fusion_out", "fusion_out_bwd")}
    finally:
        ops.FUSION_FUSED = old
        hdmoe_hip.set_compute_dtype(F32)


def test_fusion_tail_fused_against_unfused():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    fused, sel_f = _tail_run(True)
    plain, sel_p = _tail_run(False)
    assert sel_f == {"fusion_in": 1, "fusion_in_bwd": 1, "fusion_out": 1, "fusion_out_bwd": 1}, sel_f       # the second step; the first one registers the layers
    assert not any(sel_p.values()), sel_p
    assert set(fused) == set(plain) and any(k.startswith("grad:cross_attn.q_proj") for k in fused) and "grad:alpha_txt" in fused
    for n in sorted(fused):
        a, b = fused[n], plain[n]
        rel = 3e-2 if n in ("out", "gate") else 6e-2
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{n}: max|unfused| {scale:.3e}  max diff {err:.3e} ({err / max(scale, 1e-30):.2e})")
        assert torch.isfinite(a).all() and err <= rel * scale + 1e-6, (n, err, scale)
