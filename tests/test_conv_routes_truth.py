"""hdmoe_conv_fwd_route tells the truth, and Python only asks it -- GPU.

One layer per forward kernel family (the smallest shapes that reach it: csrc/conv7.hip conv7_plan, conv6.hip conv6_plan, conv6s.hip
conv6s_plan, kgemm.hip, mlinear.hip glin_try_launch, conv.hip conv_fwd_plan): the family the query names must be the one whose
kernel-selection counter moves when hdmoe_conv_fwd is really called (kgemm, glin and the generic kernels have no counter: none moves),
and the output must match torch.nn.functional.conv2d in fp64 on the CPU from the same rounded operands -- max|err| <= rel * max|ref| +
1e-6 with test_generic_conv_routes' rel = 1e-4 (fp32), 2e-2 (bf16) and test_split_bf16_conv_vs_fp64's 2e-5 for split bf16.  Then: the
profiling records of ops.mp_conv name those kernels, and the unprofiled path makes no label.
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F32S = 0, 1, 2
FWD5, CONV7, CONV6, CONV6S, KGEMM, GLIN, NONE = 3, 4, 5, 6, 7, 8, 9     # HDMOE_ROUTE_CONV_*
COUNTED = {"conv7_32", "conv7_16", "conv6", "conv6s"}                    # the forward families with a HDMOE_SEL_* counter


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()


def _min_images():
    from hdmoe_hip._lib import lib
    return lib().hdmoe_conv7_min_images()


def _route(N, H, W, Cin, Ipad, Cout, ks, has_seg, has_res, wstride, dt):
    from hdmoe_hip._lib import lib
    ints = lambda v: ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)
    r = (ctypes.c_int * 5)()
    pads = [(k - 1) // 2 for k in ks]
    assert lib().hdmoe_conv_fwd_route(ctypes.cast(r, ctypes.c_void_p), N, H, W, H, W, Cin, Cin, Ipad, Cout, Cout, 1, 0, len(ks), has_seg, has_res, wstride,
                                      ints(ks), ints(ks), ints(pads), ints(pads), dt, 1) == 0
    return tuple(r)


# (name, route, counter that moves or None, dtype code, N (None: conv7's least batch + dN), dN, H, W, Cin, Cout, kernel size per expert, res)
CASES = [
    ("conv7_w16", (CONV7, 1, 3, 1, 0), "conv7_16", BF16, None, 0, 16, 16, 32, 32, [3], False),
    ("conv7_32", (CONV7, 1, 3, 0, 0), "conv7_32", BF16, None, 0, 32, 32, 32, 32, [3, 5], False),
    ("below_conv7", (CONV6, 1, 1, 0, 0), "conv6", BF16, None, -1, 16, 16, 32, 32, [3], False),
    ("conv6", (CONV6, 1, 1, 0, 0), "conv6", BF16, 2, 0, 8, 16, 32, 32, [3], False),
    ("conv6s", (CONV6S, 1, 0, 0, 0), "conv6s", F32S, 2, 0, 8, 16, 32, 32, [3], False),
    ("kgemm", (KGEMM, 1, 0, 0, 0), None, BF16, 1, 0, 1, 64, 512, 32, [1], False),
    ("glin", (GLIN, 1, 0, 0, 0), None, F32, 9, 0, 1, 1, 256, 48, [1, 1], False),
    ("generic_fwd5_nt1_lepi_7", (FWD5, 1, 1, 1, 7), None, F32, 3, 0, 8, 8, 8, 8, [3], True),    # test_generic_conv_routes.FWD_CASES
]


@pytest.mark.parametrize("name,route,counter,dt,N,dN,H,W,Cin,Cout,ks,res", CASES, ids=[c[0] for c in CASES])
def test_route_query_names_the_kernel_that_runs(name, route, counter, dt, N, dN, H, W, Cin, Cout, ks, res):
    from hdmoe_hip import ops
    from hdmoe_hip._lib import call
    N = _min_images() + dN if N is None else N
    G, alpha, beta = len(ks), 0.75, (-0.5 if res else 0.0)
    Ipad, taps = (Cin + 15) // 16 * 16, max(ks) ** 2
    wstride = taps * Cout * Ipad
    got = _route(N, H, W, Cin, Ipad, Cout, ks, G > 1, res, wstride, dt)
    assert got == route
    tdt, rel = {F32: (torch.float32, 1e-4), BF16: (torch.bfloat16, 2e-2), F32S: (torch.float32, 2e-5)}[dt]
    gen = torch.Generator().manual_seed(len(name) * 1000 + Cin * 10 + Cout)
    x = torch.randn(N, H, W, Cin, generator=gen).to(tdt)
    ws = [(torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5).to(tdt) for k in ks]
    r = torch.randn(N, H, W, Cout, generator=gen).to(tdt)
    bounds = [N * g // G for g in range(G + 1)]               # expert-contiguous rows
    img = torch.zeros(G, taps, Cout, Ipad, dtype=tdt)
    for g, (w, k) in enumerate(zip(ws, ks)):
        img[g, :k * k, :, :Cin] = w.permute(2, 3, 0, 1).reshape(k * k, Cout, Cin)
    if dt == F32S:                                            # [hi | lo] bf16 planes, each holding all groups
        hi = img.bfloat16()
        img = torch.stack([hi, (img - hi.float()).bfloat16()])
    seg = torch.tensor(bounds, dtype=torch.int32, device=DEV) if G > 1 else None
    y = torch.full((N, H, W, Cout), float("nan"), dtype=tdt, device=DEV)
    pads = [(k - 1) // 2 for k in ks]
    xd, wd, rd = x.to(DEV), img.to(DEV), r.to(DEV)
    ops.kernel_selections(reset=True)
    call("hdmoe_conv_fwd", xd, wd, y, rd if res else None, alpha, beta, seg, G, wstride, N, H, W, H, W, Cin, Cin, Ipad, Cout, Cout, 1, 0, ks, ks,
         pads, pads, dt)
    sel = ops.kernel_selections()
    moved = {k for k in COUNTED if sel[k]}
    assert moved == ({counter} if counter else set()) and (not counter or sel[counter] == 1), sel
    ref = torch.empty(N, H, W, Cout, dtype=torch.float64)
    for g, (w, k) in enumerate(zip(ws, ks)):
        rows = slice(bounds[g], bounds[g + 1])
        ref[rows] = F.conv2d(x[rows].double().permute(0, 3, 1, 2), w.double(), padding=pads[g]).permute(0, 2, 3, 1)
    ref = alpha * ref + beta * r.double()
    err, scale = float((y.cpu().double() - ref).abs().max()), float(ref.abs().max())
    print(f"{name}: route {got}, max err {err:.3e}, {err / scale:.3e} of max|ref| (bound {rel:g})")
    assert err <= rel * scale + 1e-6, f"{name}: {err:.3e} > {rel:g} * {scale:.3e}"


def test_split_layer_outside_conv6s_answers_none():
    """W = 24 is neither 16 nor a multiple of 32: the HDMOE_F32S query answers "none" (an answer, not an error), and ops._split_ok, which
    decides the weight image format by it, says no; the same layer at W = 16 is conv6s's."""
    from hdmoe_hip import ops
    w = torch.empty(32, 32, 3, 3)
    assert _route(2, 8, 24, 32, 32, 32, [3], 0, 0, 9 * 32 * 32, F32S)[0] == NONE
    assert ops._split_ok(2, 8, 24, 32, [w]) is False
    assert ops._split_ok(2, 8, 16, 32, [w]) is True


def _mp_conv_fwd_bwd(N, H, W, Cin, Cout, k, dtype):
    from hdmoe_hip import ops
    gen = torch.Generator().manual_seed(N + Cin)
    x = torch.randn(N, H, W, Cin, generator=gen).to(dtype).to(DEV).requires_grad_(True)
    w = torch.randn(Cout, Cin, k, k, generator=gen).to(DEV).requires_grad_(True)
    y = ops.mp_conv(x, w, 1.0)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad.float()).all() and torch.isfinite(w.grad).all()


# (kernel name the forward records start with, the dgrad's, N (None: conv7's least batch), H, W, Cin, Cout, k, dtype)
RECORD_CASES = [
    ("conv7_kernel<1, 3, true>", "conv7_kernel<1, 3, true>", None, 16, 16, 32, 32, 3, torch.bfloat16),
    ("kgemm_kernel<1>", "conv_fwd", 1, 1, 64, 512, 32, 1, torch.bfloat16),     # (the dgrad, 32 -> 512, is not kgemm's)
    ("conv_fwd5_kernel<float, 1, true, 7>", "conv_fwd", 3, 8, 8, 8, 8, 3, torch.float32),
]


@pytest.mark.parametrize("fwd,dgrad,N,H,W,Cin,Cout,k,dtype", RECORD_CASES, ids=["conv7_w16", "kgemm", "generic"])
def test_profile_records_name_the_kernel_that_ran(fwd, dgrad, N, H, W, Cin, Cout, k, dtype):
    from hdmoe_hip import ops
    assert ops.PROFILE is None and not ops.PROFILE_FUSED
    ops.PROFILE = []
    try:
        _mp_conv_fwd_bwd(_min_images() if N is None else N, H, W, Cin, Cout, k, dtype)
        recs = [info for kind, info, _, _ in ops.PROFILE if kind == "conv_fwd"]
        wrecs = [info for kind, info, _, _ in ops.PROFILE if kind == "conv_wgrad"]
    finally:
        ops.PROFILE = None
    print([r["fwd_name"] for r in recs], [r["wgrad_name"] for r in wrecs])
    assert len(wrecs) == 1 and wrecs[0]["wgrad_name"].startswith(("wgrad6_kernel", "lwg_bf16_kernel", "conv_wgrad2_kernel<float, "))
    assert len(recs) == 2                                     # the forward, and the dgrad through hdmoe_conv_fwd
    assert recs[0]["fwd_name"].startswith(fwd) and recs[1]["fwd_name"].startswith(dgrad), recs
    for r in recs:
        assert {"dtype", "seg", "N", "HW", "O", "I", "taps"} <= set(r), r


def test_no_label_work_when_profiling_is_off(monkeypatch):
    from hdmoe_hip import ops

    def boom(*a, **k):
        raise AssertionError("a kernel label was built with ops.PROFILE off")
    assert ops.PROFILE is None
    monkeypatch.setattr(ops, "_kernel_label", boom)
    monkeypatch.setattr(ops, "_route", boom)
    _mp_conv_fwd_bwd(3, 8, 8, 8, 8, 3, torch.float32)


def test_conv7_batch_threshold_comes_from_the_library():
    from hdmoe_hip import ops
    assert _min_images() == 192 and ops._c7_min_images() == 192
    assert not hasattr(ops, "C7_MINN") and "C7_MINN" not in open(os.path.abspath(ops.__file__)).read()     # (the copy ops.py used to keep)
