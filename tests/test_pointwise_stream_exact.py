"""The pointwise streaming kernels that share csrc/pw_stream.h (lwgrad.hip, pbwd.hip, kgemm.hip, the weight-gradient half of fusion.hip)
on SMALL-INTEGER operands, asserted for equality -- GPU.

Tensor values are integers in {-2 .. 2}, weights in {-1, 0, 1}, every alpha is 1 or a power of two, every slab starts as small integers.
Every product and every partial sum is then an integer far below 2^24, which fp32 holds exactly: the result does not depend on the order
in which MFMA chains, waves and float atomics add, so it can be compared with == against the same contraction in fp64 on the CPU.  bf16
outputs (dx, y1 / y2) are compared with torch's own round-to-nearest-even bf16 of the exact value (sums above 256 and the half-integers
alpha = 0.5 makes do round).  Each case asserts on the host that the fp64 magnitudes stay below 2^24 (and, in the fusion mid chain, that
every intermediate the kernel rounds to bf16 stays below 256, where bf16 holds integers exactly), so that "exact" holds.

What a dropped, doubled or misplaced slice, tile, wave or slab word does to such a result is an integer error: nothing hides below a
tolerance.  Shapes:
  positions P in {1, 63, 65, 257, 1025} (no full 64-position slice; a slice and a tail; several slots of four slices) in three expert
  groups, the middle one EMPTY, with a row outside every group on either side (seg = [1, 1 + P // 3, 1 + P // 3, 1 + P] of P + 2 rows):
  the empty group's slab and, for hdmoe_pw_bwd, dx of the outside rows must stay as they were; one larger P at which a workgroup gets
  more than four slices, so that a wave makes a second trip with a prefetch in flight (lwg: 33281 positions at 128 x 128 channels;
  pw_bwd: 65601 at 64 x 64);
  hdmoe_conv_wgrad on the lwg route, bf16 and fp32, (Cin, Cout) in {(32, 32), (64, 32), (32, 64), (64, 64), (96, 32)}; hdmoe_lwgrad2 at
  Cin = 64 and 128; hdmoe_pw_bwd at every admitted (Cout / 32, Cin / 32) with a product <= 8;
  hdmoe_kgemm2_fwd at M in {1, 33}, K in {512, 576} (one chunk per wave; a ninth chunk);
  hdmoe_fusion_in_bwd_wg without sw and hdmoe_fusion_mid_bwd with slabs at rows in {1, 33, 129} on the default grid.
Every output sits between guard elements, compared bit for bit with their fill; every element of every output is compared (the count of
compared elements is asserted to be the tensor's size).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {F32: 0, BF16: 1}
GUARD = 64
MARK = -4096.0                                               # guard fill: exact in bf16 and fp32, outside every result's range
PS = [1, 63, 65, 257, 1025]
LWG_SHAPES = [(32, 32), (64, 32), (32, 64), (64, 64), (96, 32)]            # (Cin, Cout)
PBW_TILES = [(ot, it) for ot in (1, 2, 3, 4) for it in (1, 2, 3, 4) if ot * it <= 8]
WG_LWG = 4                                                   # HDMOE_ROUTE_WGRAD_LWG


@pytest.fixture(scope="module")
def call():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    return call


def _ints(shape, lo, hi, gen, dtype):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(dtype)


class Out:
    """An output of `shape` between GUARD guard elements; `init` (CPU tensor) or the guard fill is what the kernel finds there."""

    def __init__(self, shape, dtype, init=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), MARK, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init.to(dtype))

    def equals(self, tag, ref):
        """Every element == ref (an fp64 CPU tensor of the output's shape), guards untouched."""
        torch.cuda.synchronize()
        got = self.t.cpu().double()
        assert got.shape == ref.shape, (tag, got.shape, ref.shape)
        same = got == ref
        assert same.numel() == self.t.numel(), f"{tag}: compared {same.numel()} of {self.t.numel()} elements"
        bad = int((~same).sum())
        assert bad == 0, f"{tag}: {bad} of {same.numel()} elements differ, first at {(~same).nonzero()[0].tolist()}: " \
                         f"got {got[~same][0].item()}, exact {ref[~same][0].item()}"
        g = self.buf.cpu()
        assert bool((g[:GUARD] == MARK).all() and (g[-GUARD:] == MARK).all()), f"{tag}: guard elements overwritten"


def _exact(*tensors):
    """fp32 holds every partial sum of these fp64 magnitude bounds exactly."""
    for t in tensors:
        assert t.numel() == 0 or float(t.abs().max()) < 2.0 ** 24


def _groups(P):
    """Three groups over rows 1 .. P of P + 2 rows, the middle one empty."""
    return [1, 1 + P // 3, 1 + P // 3, 1 + P]


def _dw_case(P, I, O, dtype, seed):
    """x [P + 2][I], dy [P + 2][O], the slabs' integer prefill [3][O][I] and the exact slabs after G[g] += dy_g^T x_g."""
    gen = torch.Generator().manual_seed(seed)
    x, dy = _ints((P + 2, I), -2, 2, gen, dtype), _ints((P + 2, O), -2, 2, gen, dtype)
    pre = _ints((3, O, I), -3, 3, gen, F32)
    seg = _groups(P)
    ref = pre.double().clone()
    for g in range(3):
        a, b = seg[g], seg[g + 1]
        ref[g] += dy[a:b].double().t() @ x[a:b].double()
    _exact(pre.double().abs() + 4.0 * P)
    return x, dy, pre, seg, ref


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("P", PS + [33281])
def test_lwg_slabs_are_exact(call, P, dtype):
    from hdmoe_hip._lib import lib
    for I, O in (LWG_SHAPES if P < 33281 else [(128, 128)]):
        r = (ctypes.c_int * 34)()
        one, zero = (ctypes.c_int * 3)(1, 1, 1), (ctypes.c_int * 3)(0, 0, 0)
        assert lib().hdmoe_conv_wgrad_route(ctypes.cast(r, ctypes.c_void_p), P + 2, 1, 1, 1, 1, I, I, O, 1, 0, 3, 1, one, one, zero, zero, DT[dtype], 1) == 0
        assert r[0] == WG_LWG, (P, I, O, r[0])
        x, dy, pre, seg, ref = _dw_case(P, I, O, dtype, 7 * P + I + 3 * O)
        G = [Out((O, I), F32, pre[g]) for g in range(3)]
        segd = torch.tensor(seg, dtype=torch.int32, device=DEV)
        rc = call("hdmoe_conv_wgrad", x.to(DEV), dy.to(DEV), [g.t for g in G], segd, 3, P + 2, 1, 1, 1, 1, I, I, O, 1, 0, [1] * 3, [1] * 3, [0] * 3,
                  [0] * 3, DT[dtype])
        assert rc == 0
        for g in range(3):
            G[g].equals(f"lwg P={P} {I}->{O} group {g}", ref[g])


@pytest.mark.parametrize("P", PS)
def test_lwgrad2_slabs_are_exact(call, P):
    for I in (64, 128):
        gen = torch.Generator().manual_seed(11 * P + I)
        x = _ints((P, I), -2, 2, gen, BF16)
        dy = [_ints((P, 32), -2, 2, gen, BF16) for _ in range(2)]
        pre = [_ints((32, I), -3, 3, gen, F32) for _ in range(2)]
        ref = [pre[i].double() + dy[i].double().t() @ x.double() for i in range(2)]
        _exact(*ref, torch.tensor(3.0 + 4.0 * P))
        G = [Out((32, I), F32, pre[i]) for i in range(2)]
        assert call("hdmoe_lwgrad2", x.to(DEV), dy[0].to(DEV), dy[1].to(DEV), G[0].t, G[1].t, P, I, 1) == 0, "hdmoe_lwgrad2 declined a shape of its domain"
        for i in range(2):
            G[i].equals(f"lwgrad2 P={P} Cin={I} layer {i}", ref[i])


@pytest.mark.parametrize("P", PS + [65601])
def test_pw_bwd_slabs_and_dx_are_exact(call, P):
    alpha = 0.5
    for OT, IT in (PBW_TILES if P < 65601 else [(2, 2)]):
        I, O = 32 * IT, 32 * OT
        x, dy, pre, seg, gref = _dw_case(P, I, O, BF16, 13 * P + I + 5 * O)
        gen = torch.Generator().manual_seed(P + I * O)
        w = _ints((3, O, I), -1, 1, gen, BF16)
        wd = w.transpose(1, 2).contiguous()                      # the flipped image of a 1 x 1 layer: [g][I][O]
        xref = torch.full((P + 2, I), MARK, dtype=torch.float64)     # rows outside every group keep what dx held
        for g in range(3):
            a, b = seg[g], seg[g + 1]
            v = alpha * (dy[a:b].double() @ w[g].double())
            _exact(v)
            xref[a:b] = v.to(BF16).double()                      # torch's round-to-nearest-even of the exact value
        G = [Out((O, I), F32, pre[g]) for g in range(3)]
        dx = Out((P + 2, I), BF16)
        segd = torch.tensor(seg, dtype=torch.int32, device=DEV)
        rc = call("hdmoe_pw_bwd", x.to(DEV), dy.to(DEV), wd.to(DEV), dx.t, [g.t for g in G], segd, 3, I * O, P + 2, 1, I, O, alpha, 1)
        assert rc == 0, f"hdmoe_pw_bwd declined {I}->{O}"
        dx.equals(f"pw_bwd P={P} {I}->{O} dx", xref)
        for g in range(3):
            G[g].equals(f"pw_bwd P={P} {I}->{O} group {g}", gref[g])


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("K", [512, 576])
def test_kgemm2_outputs_are_exact(call, M, K):
    gen = torch.Generator().manual_seed(M + K)
    x = _ints((M, K), -2, 2, gen, BF16)
    w = [_ints((32, K), -1, 1, gen, BF16) for _ in range(2)]
    al = (1.0, 0.5)
    y = [Out((M, 32), BF16) for _ in range(2)]
    assert call("hdmoe_kgemm2_fwd", x.to(DEV), w[0].to(DEV), w[1].to(DEV), y[0].t, y[1].t, M, K, al[0], al[1], 1) == 0, "hdmoe_kgemm2_fwd declined a shape of its domain"
    for i in range(2):
        v = al[i] * (x.double() @ w[i].double().t())
        _exact(v)
        y[i].equals(f"kgemm2 M={M} K={K} y{i + 1}", v.to(BF16).double())


@pytest.mark.parametrize("rows", [1, 33, 129])
def test_fusion_in_slabs_are_exact(call, rows):
    gen = torch.Generator().manual_seed(rows)
    T = {n: _ints((rows, 32), -2, 2, gen, BF16) for n in ("dq", "dk", "dv", "fu", "fv")}
    wd = [_ints((32, 32), -1, 1, gen, BF16).to(DEV) for _ in range(3)]
    pre = [_ints((32, 32), -3, 3, gen, F32) for _ in range(3)]
    D = {n: t.to(DEV) for n, t in T.items()}
    G = [Out((32, 32), F32, p) for p in pre]
    dfu, dfv = Out((rows, 32), BF16), Out((rows, 32), BF16)
    rc = call("hdmoe_fusion_in_bwd_wg", D["dq"], D["dk"], D["dv"], None, None, D["fu"], D["fv"], None, wd[0], wd[1], wd[2], dfu.t, dfv.t, None,
              G[0].t, G[1].t, G[2].t, 0, rows, rows, 32, 1.0, 1.0, 1.0, 1)
    assert rc == 0, "hdmoe_fusion_in_bwd_wg declined a shape of its domain"
    # without sw the forward's query and ctx are fu and fv
    for g, p, name, dy, x in zip(G, pre, ("Gq", "Gk", "Gv"), ("dq", "dk", "dv"), ("fu", "fv", "fv")):
        ref = p.double() + T[dy].double().t() @ T[x].double()
        _exact(ref)
        g.equals(f"fusion_in rows={rows} {name}", ref)


@pytest.mark.parametrize("rows", [1, 33, 129])
def test_fusion_mid_slabs_are_exact(call, rows):
    gen = torch.Generator().manual_seed(100 + rows)
    T = {n: _ints((rows, 32), -2, 2, gen, BF16) for n in ("da", "dq2", "a", "o1")}
    wo, wq = _ints((32, 32), -1, 1, gen, BF16), _ints((32, 32), -1, 1, gen, BF16)
    pre = [_ints((32, 32), -3, 3, gen, F32) for _ in range(2)]
    D = {n: t.to(DEV) for n, t in T.items()}
    Go, Gq = Out((32, 32), F32, pre[0]), Out((32, 32), F32, pre[1])
    do1, dres = Out((rows, 32), BF16), Out((rows, 32), BF16)
    rc = call("hdmoe_fusion_mid_bwd", D["da"], D["dq2"], D["a"], D["o1"], wo.t().contiguous().to(DEV), wq.t().contiguous().to(DEV), do1.t, dres.t,
              Go.t, Gq.t, 0, rows, 32, 1.0, 1.0, 1.0, 1)
    assert rc == 0, "hdmoe_fusion_mid_bwd declined a shape of its domain"
    # the gradient of a: da + (dq2 through q_proj), both rounded to bf16 by the kernel -- integers below 256, so exactly
    dq2x = T["dq2"].double() @ wq.double()
    dat = T["da"].double() + dq2x
    assert float(dq2x.abs().max()) < 256 and float(dat.abs().max()) < 256
    ref_o, ref_q = pre[0].double() + dat.t() @ T["o1"].double(), pre[1].double() + T["dq2"].double().t() @ T["a"].double()
    _exact(ref_o, ref_q, torch.tensor(3.0 + 2.0 * 66.0 * rows))
    Go.equals(f"fusion_mid rows={rows} Go", ref_o)
    Gq.equals(f"fusion_mid rows={rows} Gq", ref_q)
