"""DMA addressing of the whole-image streaming kernels (csrc/conv7_body.h: conv7 and the dgrad program of the fused backward launch bwd7).

The kernels build every DMA offset from byte strides of the launch plan: the wave's part of an offset rides in the lane offset, the scalar
part advances by adding a stride from piece to piece, stage to stage, chunk to chunk and output block to output block, and a unit (image)
is decoded once from a small table in LDS.  These cases are the smallest shapes at which that arithmetic can go wrong and that
tests/test_streaming_kernels.py does not reach; the checks and tolerances are that file's (tools/conv6_check.check and
tools/conv7_check.check_bwd: torch's conv2d on the bf16-rounded operands, autograd of MP_Conv, reference models/model_internals.py:253-275).
The FiLM case is checked like tests/test_film_dgrad_epilogue.py: du bit-identical to the two-launch form, de within twice that form's error
against fp64, weight gradients within its run-to-run difference."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checks():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    argv, sys.argv = sys.argv, ["conv7_check.py"]            # (the tool is a script: no mode flags, it only defines its functions)
    try:
        import conv6_check
        import conv7_check
    finally:
        sys.argv = argv
    return conv6_check, conv7_check


FWD = [  # N, R, Cin, Cout, kernel sizes, segment ends, residual
    # 256 workgroups, three units each: the snake's third row, and the prefetch of a next unit that belongs to another group
    (600, 32, 32, 32, (3, 3, 5, 5), (130, 301, 433, 600), True),
    (196, 32, 256, 32, (3, 5), (95, 196), False),                 # eight chunks
    (196, 32, 32, 256, (3, 5), (95, 196), False),                 # four output blocks with CO = 2
    (200, 32, 64, 64, (7, 3, 5), (0, 90, 200), True),             # first expert empty: group order is not the descending sort; 7x7 weight strides
    (193, 16, 64, 128, (3, 5), (97, 193), True),                  # odd segment sizes: an absent second image; two output blocks
]


@pytest.mark.parametrize("N,R,Cin,Cout,ks,split,res", FWD, ids=[f"{c[0]}x{c[1]}_{c[2]}to{c[3]}_k{''.join(map(str, c[4]))}" for c in FWD])
def test_conv7_forward_dgrad_wgrad_match_conv2d(checks, N, R, Cin, Cout, ks, split, res):
    c6, _ = checks
    assert c6.check(N, R, Cin, Cout, ks, split, res, seed=N + R)


BWD = [  # N, R, Cin, Cout, kernel sizes, segment ends
    (200, 32, 96, 64, (3, 5), (90, 200)),                         # dgrad 64 -> 96: two chunks, three output blocks of 32
    (200, 32, 256, 128, (3,), (200,)),                            # 3x3 alone: dgrad 128 -> 256, four chunks, four output blocks of 64
    (520, 16, 64, 64, (3, 5), (251, 520)),                        # 16 x 16: more image pairs than workgroups (a second unit per workgroup)
]


@pytest.mark.parametrize("N,R,Cin,Cout,ks,split", BWD, ids=[f"{c[0]}x{c[1]}_{c[2]}to{c[3]}_k{''.join(map(str, c[4]))}" for c in BWD])
def test_fused_backward_launch_matches_conv2d(checks, N, R, Cin, Cout, ks, split):
    _, c7 = checks
    assert c7.check_bwd(N, R, Cin, Cout, ks, split, seed=N + Cin)


def _silu_grad64(x):
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s)) / 0.596


@pytest.mark.parametrize("R", [32, 16])
def test_film_epilogue_launch_against_the_two_launches(checks, R):
    """hdmoe_conv_bwd6_film at N = 200, 64 channels (no dropout): du bit for bit the two launches', two fused runs identical, de against fp64
    no further than twice the standalone kernel's error (or its run-to-run spread), weight gradients within the two-launch run-to-run difference."""
    from hdmoe_hip._lib import _int_array, call, lib
    from hdmoe_hip.bank import w6_record
    N, C, ks, split = 200, 64, (3, 5), (97, 200)
    g = torch.Generator().manual_seed(1000 * N + R + C)
    u = torch.randn(N, R, R, C, generator=g).bfloat16().cuda()
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
    h = torch.empty_like(u)
    call("hdmoe_film_silu_fwd", h, u, e, N, HW, C, 1)
    kib = lib().hdmoe_conv_wgrad6_ws_kib(E, N, R, R, C, C, ctypes.cast(_int_array(ks), ctypes.c_void_p), ctypes.cast(_int_array(ks), ctypes.c_void_p), 1)
    assert kib > 0
    pts = [(k - 1) // 2 for k in ks]
    alpha = 0.7

    def wgrads(launch):
        wsb = torch.full((2 * kib * 256,), float("nan"), dtype=torch.float32, device="cuda")
        Gs = [torch.zeros(k * k, C, C, device="cuda") for k in ks]
        assert launch(Gs, wsb) == 0
        call("hdmoe_conv_wgrad6_reduce_batch", Gs + [None] * (8 - E), [seg], [wsb], w6_record(E, N, R, R, C, C, 1, ks), 1)
        return Gs

    def unfused():
        dx = torch.full_like(u, float("nan"))
        Gs = wgrads(lambda Gs, wsb: call("hdmoe_conv_bwd6", h, dy, wd, dx, Gs, seg, E, wstride, N, R, R, C, C, list(ks), list(ks), pts, pts, alpha,
                                         wsb, wsb.numel() * 4, 1))
        du, de = torch.empty_like(u), torch.zeros_like(e)
        call("hdmoe_film_silu_bwd", du, de, dx, u, e, N, HW, C, 1)
        return dx, du, de, Gs

    def fused():
        du = torch.full_like(u, float("nan"))
        de = torch.full_like(e, float("nan"))                       # written, not accumulated
        Gs = wgrads(lambda Gs, wsb: call("hdmoe_conv_bwd6_film", h, dy, wd, du, Gs, seg, E, wstride, N, R, R, C, C, list(ks), list(ks), pts, pts,
                                         alpha, wsb, wsb.numel() * 4, u, e, None, de, 0.0, 1))
        return du, de, Gs

    (dx, du, de, Gs), (_, du2, de2, Gs2) = unfused(), unfused()
    du_f, de_f, Gs_f = fused()
    du_f2, de_f2, _ = fused()
    torch.cuda.synchronize()
    assert torch.equal(du, du2)
    assert torch.isfinite(du_f.float()).all() and torch.isfinite(de_f).all()
    assert torch.equal(du_f, du), f"du differs in {int((du_f != du).sum())} elements"
    assert torch.equal(du_f2, du) and torch.equal(de_f2, de_f)
    for a, b, c in zip(Gs_f, Gs, Gs2):
        assert float((a - b).abs().max()) <= float((b - c).abs().max()), "weight gradient moved by more than the two-launch run-to-run difference"
    t = dx.double() * _silu_grad64(u.double() * e.double()[:, None, None, :]) * u.double()
    ref, norm = t.sum(dim=(1, 2)), t.abs().sum(dim=(1, 2))
    err = lambda d: float(((d.double() - ref).abs() / norm).max())
    spread = float(((de - de2).double().abs() / norm).max())
    print(f"R {R}: de err fused {err(de_f):.3e}, standalone {err(de):.3e} / {err(de2):.3e}, standalone run-to-run {spread:.3e}")
    assert err(de_f) <= 2 * max(err(de), err(de2), spread)
