"""The generic conv kernels of csrc/conv.hip, one case per template instantiation the launch plan can pick -- GPU.

hdmoe_conv_fwd / hdmoe_conv_wgrad are called directly on hand-built weight images [g][tap][Cout][Ipad] (not through ops.mp_conv), each
case first asserts with the route query (hdmoe_conv_generic_route / hdmoe_conv_wgrad_route) that its shape reaches the instantiation it
is named after, then compares with torch.nn.functional.conv2d and its weight gradient in fp64 on the CPU, computed from the same
(bf16-rounded) operands.  Tolerances are test_mp_conv_vs_oracle's: max|err| <= rel * max|ref| + 1e-6, rel = 1e-4 (fp32), 2e-2 (bf16).
The shapes are the smallest at which a swapped template argument gives wrong numbers: maps of 4 x 4 / 8 x 8 (one 8 x 64 for the block
tiles), 6 - 16 input channels, N = 2 or 3.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = 0, 1
FWD, FWD2, FWD3, FWD5 = 0, 1, 2, 3                           # HDMOE_ROUTE_CONV_*
WG_V2, WG_V1, WG_SWG, WG_TOWG, WG_LWG = 0, 1, 2, 3, 4         # HDMOE_ROUTE_WGRAD_*


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()


def _ints(v):
    return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)


def _fwd_route(N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout, Cstore, stride, ones, ks, dt):
    from hdmoe_hip._lib import lib
    r = (ctypes.c_int * 5)()
    assert lib().hdmoe_conv_generic_route(ctypes.cast(r, ctypes.c_void_p), N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout, Cstore, stride, ones, len(ks),
                                          _ints(ks), _ints(ks), dt, 1) == 0
    return tuple(r)


def _wgrad_route(N, H, W, Ho, Wo, Cin, Cphys, Cout, stride, ones, ks, has_seg, dt):
    from hdmoe_hip._lib import lib
    r = (ctypes.c_int * 34)()
    pads = [(k - 1) // 2 for k in ks]
    assert lib().hdmoe_conv_wgrad_route(ctypes.cast(r, ctypes.c_void_p), N, H, W, Ho, Wo, Cin, Cphys, Cout, stride, ones, len(ks), has_seg,
                                        _ints(ks), _ints(ks), _ints(pads), _ints(pads), dt, 1) == 0
    return r[0], [tuple(r[2 + 4 * k:6 + 4 * k]) for k in range(r[1])]


def _close(got, ref, rel, msg):
    err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
    print(f"{msg}: max err {err:.3e}, {err / scale:.3e} of max|ref| (bound {rel:g})")
    assert err <= rel * scale + 1e-6, f"{msg}: {err:.3e} > {rel:g} * {scale:.3e}"


# (name, route = (kernel, NT / NB, VEC, LEPI, NHR), dtype, H, W, k, stride, Cin, Cout, Cstore, ones, res)
FWD_CASES = [
    ("fwd_nb1_vec", (FWD, 1, 1, 0, 0), F32, 4, 4, 3, 1, 8, 8, 8, 0, False),
    ("fwd_nb2_vec", (FWD, 2, 1, 0, 0), F32, 4, 4, 3, 1, 8, 48, 48, 0, False),
    ("fwd_nb4_vec", (FWD, 4, 1, 0, 0), F32, 4, 4, 3, 1, 8, 72, 72, 0, True),
    ("fwd_nb1_novec", (FWD, 1, 0, 0, 0), F32, 4, 4, 3, 1, 6, 8, 8, 0, False),
    ("fwd_stride2", (FWD, 1, 1, 0, 0), F32, 8, 8, 3, 2, 8, 8, 8, 0, False),
    ("fwd5_nt1_lepi_7", (FWD5, 1, 1, 1, 7), F32, 8, 8, 3, 1, 8, 8, 8, 0, True),
    ("fwd5_nt2_lepi_7", (FWD5, 2, 1, 1, 7), F32, 8, 8, 3, 1, 8, 48, 48, 0, False),
    ("fwd5_nt1_nolepi_7", (FWD5, 1, 1, 0, 7), F32, 8, 8, 1, 1, 8, 8, 8, 0, False),
    ("fwd5_nt1_lepi_9", (FWD5, 1, 1, 1, 9), F32, 8, 64, 7, 1, 8, 8, 8, 0, False),
    ("fwd5_bf16", (FWD5, 1, 1, 1, 7), BF16, 8, 8, 3, 1, 8, 8, 8, 0, True),
    ("fwd3_nt1", (FWD3, 1, 1, 0, 0), F32, 8, 8, 3, 1, 8, 6, 6, 0, False),
    ("fwd3_nt2", (FWD3, 2, 1, 0, 0), F32, 8, 8, 3, 1, 8, 38, 38, 0, True),
    ("fwd3_ones", (FWD3, 1, 1, 0, 0), F32, 8, 8, 3, 1, 9, 8, 8, 1, False),
    ("fwd2_novec", (FWD2, 1, 0, 0, 0), F32, 8, 8, 3, 1, 6, 8, 8, 0, False),
    ("fwd2_vec", (FWD2, 1, 1, 0, 0), F32, 8, 32, 7, 1, 8, 6, 6, 0, False),     # (a 14 x 38 halo and a channel tail: neither fwd5 nor fwd3)
]


@pytest.mark.parametrize("name,route,dt,H,W,k,stride,Cin,Cout,Cstore,ones,res", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_generic_forward_instantiation(name, route, dt, H, W, k, stride, Cin, Cout, Cstore, ones, res):
    from hdmoe_hip._lib import call
    N, pad, alpha, beta = 3, (k - 1) // 2, 0.75, (-0.5 if res else 0.0)
    Cphys, Ipad = Cin - ones, (Cin + 15) // 16 * 16
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    assert _fwd_route(N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout, Cstore, stride, ones, [k], dt) == route
    tdt, rel = (torch.float32, 1e-4) if dt == F32 else (torch.bfloat16, 2e-2)
    gen = torch.Generator().manual_seed(len(name) * 1000 + Cin * 10 + Cout)
    x = torch.randn(N, H, W, Cphys, generator=gen).to(tdt)
    w = (torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5).to(tdt)
    r = torch.randn(N, Ho, Wo, Cstore, generator=gen).to(tdt)
    img = torch.zeros(k * k, Cout, Ipad, dtype=tdt)
    img[:, :, :Cin] = w.permute(2, 3, 0, 1).reshape(k * k, Cout, Cin)
    xd, wd, rd = x.to(DEV), img.to(DEV), r.to(DEV)
    y = torch.full((N, Ho, Wo, Cstore), float("nan"), dtype=tdt, device=DEV)
    call("hdmoe_conv_fwd", xd, wd, y, rd if res else None, alpha, beta, None, 1, k * k * Cout * Ipad, N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout,
         Cstore, stride, ones, [k], [k], [pad], [pad], dt)
    x64 = x.double().permute(0, 3, 1, 2)
    if ones:
        x64 = torch.cat([x64, torch.ones_like(x64[:, :1])], 1)
    ref = alpha * F.conv2d(x64, w.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)[..., :Cstore] + beta * r.double()
    _close(y.cpu(), ref, rel, name)


def test_grouped_fp32_linear_two_column_blocks():
    """glin_f32_kernel<2> (256 < Cin <= 512), the one column-block count the grouped-linear test does not reach."""
    from hdmoe_hip._lib import call
    N, Cin, Cout = 9, 512, 48
    gen = torch.Generator().manual_seed(5)
    x, w = torch.randn(N, Cin, generator=gen), torch.randn(Cout, Cin, generator=gen) / Cin ** 0.5
    y = torch.full((N, Cout), float("nan"), device=DEV)
    call("hdmoe_conv_fwd", x.to(DEV), w.to(DEV), y, None, 0.75, 0.0, None, 1, Cout * Cin, N, 1, 1, 1, 1, Cin, Cin, Cin, Cout, Cout, 1, 0,
         [1], [1], [0], [0], F32)
    _close(y.cpu(), 0.75 * x.double() @ w.double().T, 1e-4, "glin<2>")


# (name, route code, classes = [(passes, MAXT, OT, VEC)], dtype, k per group, stride, Cin, Cout)
WGRAD_CASES = [
    ("wg2_ot1_mt3", WG_V2, [(1, 3, 1, 1)], F32, [3], 1, 16, 8),
    ("wg2_ot2_mt3", WG_V2, [(1, 3, 2, 1)], F32, [3], 1, 16, 48),
    ("wg2_mt7", WG_V2, [(1, 7, 1, 1)], F32, [5], 1, 16, 8),
    ("wg2_two_passes", WG_V2, [(2, 7, 1, 1)], F32, [7], 1, 16, 8),
    ("wg2_novec", WG_V2, [(1, 3, 1, 0)], F32, [3], 1, 6, 8),
    ("wg2_bf16", WG_V2, [(1, 3, 1, 1)], BF16, [3], 1, 16, 8),
    ("wg2_two_classes", WG_V2, [(1, 3, 1, 1), (1, 7, 1, 1)], F32, [3, 5, 3], 1, 16, 8),
    ("wg_v1_stride2", WG_V1, [], F32, [3], 2, 16, 8),
    ("lwg_ot2_it1", WG_LWG, [], BF16, [1], 1, 32, 64),
    ("lwg_ot1_it2", WG_LWG, [], BF16, [1], 1, 64, 32),
]


@pytest.mark.parametrize("name,code,classes,dt,ks,stride,Cin,Cout", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_generic_wgrad_instantiation(name, code, classes, dt, ks, stride, Cin, Cout):
    from hdmoe_hip._lib import call
    G, H, W = len(ks), 8, 8
    N = 3 if G > 1 else 2                                     # grouped: one row per expert
    pads = [(k - 1) // 2 for k in ks]
    Ho, Wo = (H + 2 * pads[0] - ks[0]) // stride + 1, (W + 2 * pads[0] - ks[0]) // stride + 1
    assert _wgrad_route(N, H, W, Ho, Wo, Cin, Cin, Cout, stride, 0, ks, 1 if G > 1 else 0, dt) == (code, classes)
    tdt, rel = (torch.float32, 1e-4) if dt == F32 else (torch.bfloat16, 2e-2)
    gen = torch.Generator().manual_seed(len(name) * 1000 + Cin * 10 + Cout)
    x = torch.randn(N, H, W, Cin, generator=gen).to(tdt)
    dy = torch.randn(N, Ho, Wo, Cout, generator=gen).to(tdt)
    seg = torch.arange(G + 1, dtype=torch.int32, device=DEV) if G > 1 else None
    Gs = [torch.zeros(k * k, Cout, Cin, device=DEV) for k in ks]
    call("hdmoe_conv_wgrad", x.to(DEV), dy.to(DEV), Gs, seg, G, N, H, W, Ho, Wo, Cin, Cin, Cout, stride, 0, ks, ks, pads, pads, dt)
    for g, k in enumerate(ks):
        rows = slice(g, g + 1) if G > 1 else slice(0, N)
        w64 = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
        out = F.conv2d(x[rows].double().permute(0, 3, 1, 2), w64, stride=stride, padding=pads[g])
        (out * dy[rows].double().permute(0, 3, 1, 2)).sum().backward()
        _close(Gs[g].cpu().reshape(k, k, Cout, Cin).permute(2, 3, 0, 1), w64.grad, rel, f"{name}[{g}]")
