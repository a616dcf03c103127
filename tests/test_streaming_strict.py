"""The streaming conv kernels -- conv7 (forward / input gradient), the fused backward launch bwd7 with its weight-gradient programs (wgrad8
for 3x3 on 32 x 32 maps in each of its channel-chunk layouts, wgrad7 for 5x5, the wgrad6 programs with OT = 1 / 2 on 16 x 16 maps) and the
deferred slab reduction -- against an fp64 reference of the same operation, with ELEMENTWISE error bounds derived from the arithmetic, and
with the library's kernel-selection counters (include/hdmoe.h HDMOE_SEL_*) asserting that each case ran the kernel it names.

Reference: fp64 conv / dgrad / wgrad of the same bf16-rounded operands and segments, written as one fp64 matrix product per tap (``_conv``,
``_dgrad``, ``_wgrad`` below; torch's fp64 GEMM on the device -- the Cin = Cout = 256 cases are ~1 TFLOP of fp64 each, minutes on a CPU).
The same functions run on the CPU in the checker-sensitivity test.

Bounds.  bf16 products are exact in fp32, so the only error sources are fp32 accumulation and the final rounding:
  y, dx (stored bf16):  |got - ref| <= 2^-8 |ref| + C_BF16 * 2^-24 * T   -- round-to-nearest to 8 significant bits is within 2^-8 of the
                                                                              value; T = the fp64 conv of |x| and |w| (sum of |terms|)
  dW (fp32):            |got - ref| <= C_W * 2^-24 * T                     -- T = sum over the reduced positions of |x * dy|
An expert without rows must give an exactly zero weight gradient (T = 0).  C_BF16 / C_W are set from the worst measured values (written to
build/measurements/streaming_strict.json with each case's needed c): see the constants.  ``test_bound_rejects_injected_faults`` shows on the CPU
that the same bound function rejects a dropped image in a weight gradient at N = 200, a zeroed 32-channel output chunk, swapped images of
a 16 x 16 pair and a kernel-size group whose taps are shifted by one pixel -- faults that the earlier max-relative checks (2e-2 / 1e-3)
could pass."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "build", "measurements")     # measured errors (kept out of git: build/)
U24 = 2.0 ** -24
REL_BF16 = 2.0 ** -8
# Accumulation-term constants, from the worst needed c over every case below on an MI355X (build/measurements/streaming_strict.json "worst"):
# y / dx measured 0.88 (y, 200 x 32 x 32, 32 -> 96) and 0.77 (dx); dW measured 1.81 (the one-row 3x3 expert on 16 x 16 maps, where the
# sum of |terms| is smallest), 1.35 at Cin = Cout = 256, <= 0.4 elsewhere.  The bounds keep 4.5x and 6.6x of that.
C_BF16 = 4.0
C_W = 12.0
_measured = {}


# ---------------------------------------------------------------------------------------------------------------- fp64 reference
def _pad(x, k):
    p = (k - 1) // 2
    return F.pad(x, (0, 0, p, k - 1 - p, p, k - 1 - p))


def _conv(x, w, shift=0):
    """'same' k x k conv of channel-last x (n, H, W, I) with w (O, I, k, k), pad (k - 1) // 2 ahead; ``shift`` moves every tap's window
    by that many pixels to the right (a fault of the sensitivity test only)."""
    n, H, W, I = x.shape
    O, k = w.shape[0], w.shape[-1]
    xp = F.pad(_pad(x, k), (0, 0, 0, abs(shift), 0, 0)) if shift else _pad(x, k)
    y = x.new_zeros(n * H * W, O)
    for ky in range(k):
        for kx in range(k):
            y += xp[:, ky:ky + H, kx + shift:kx + shift + W, :].reshape(-1, I) @ w[:, :, ky, kx].T
    return y.view(n, H, W, O)


def _dgrad(dy, w):
    n, H, W, O = dy.shape
    I, k = w.shape[1], w.shape[-1]
    p = (k - 1) // 2
    dxp = dy.new_zeros(n, H + k - 1, W + k - 1, I)
    d2 = dy.reshape(-1, O)
    for ky in range(k):
        for kx in range(k):
            dxp[:, ky:ky + H, kx:kx + W, :] += (d2 @ w[:, :, ky, kx]).view(n, H, W, I)
    return dxp[:, p:p + H, p:p + W, :]


def _wgrad(x, dy, k):
    """[tap][O][I] = sum over (n, h, w) of dy[n, h, w, o] * xpad[n, h + ky, w + kx, i]."""
    n, H, W, I = x.shape
    O = dy.shape[-1]
    xp = _pad(x, k)
    d2t = dy.reshape(-1, O).T
    return torch.stack([d2t @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, I) for ky in range(k) for kx in range(k)])


def reference(x, dy, ws, seg, res=None, alpha=1.0, beta=0.0):
    """fp64 (y, |terms| of y, dx, |terms| of dx, [dW], [|terms| of dW]) of the grouped layer; operands as given (fp64, any device)."""
    ys, ya, dxs, dxa, gs, ga = [], [], [], [], [], []
    for g, w in enumerate(ws):
        a, b = seg[g], seg[g + 1]
        k = w.shape[-1]
        xs, ds = x[a:b], dy[a:b]
        ys.append(alpha * _conv(xs, w)); ya.append(abs(alpha) * _conv(xs.abs(), w.abs()))
        dxs.append(alpha * _dgrad(ds, w)); dxa.append(abs(alpha) * _dgrad(ds.abs(), w.abs()))
        gs.append(alpha * _wgrad(xs, ds, k)); ga.append(abs(alpha) * _wgrad(xs.abs(), ds.abs(), k))
    y, ta = torch.cat(ys), torch.cat(ya)
    if res is not None:
        y, ta = y + beta * res, ta + abs(beta) * res.abs()
    return y, ta, torch.cat(dxs), torch.cat(dxa), gs, ga


def needed_c(got, ref, terms, rel):
    """The smallest c for which |got - ref| <= rel |ref| + c 2^-24 terms holds at every element (inf: an element with terms = 0 differs)."""
    d = (got.double() - ref).abs() - rel * ref.abs()
    d = d.clamp(min=0.0)
    if bool(((terms == 0) & (d > 0)).any()):
        return float("inf")
    t = torch.where(terms > 0, terms, torch.ones_like(terms))
    return float((d / (U24 * t)).max()) if d.numel() else 0.0


def within(got, ref, terms, rel, c):
    return needed_c(got, ref, terms, rel) <= c


# ---------------------------------------------------------------------------------------------------------------- CPU-only checks
def _operands(N, R, Cin, Cout, ks, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, R, R, Cin, generator=g).bfloat16()
    ws = [(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16() for k in ks]
    dy = torch.randn(N, R, R, Cout, generator=g).bfloat16()
    return x, ws, dy


def test_bound_rejects_injected_faults():
    """The bound function applied to the fp64 reference itself: the correct result, rounded as the kernels store it, passes; each
    injected fault is rejected."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    N, R, seg, ks = 200, 16, [0, 97, 200], (3, 5)
    x, ws, dy = _operands(N, R, 32, 64, ks, 3)
    x64, dy64, w64 = x.double(), dy.double(), [w.double() for w in ws]
    y, ya, dx, dxa, gs, ga = reference(x64, dy64, w64, seg)
    # the correct results as stored: bf16 activations, fp32 weight gradients
    assert within(y.bfloat16(), y, ya, REL_BF16, C_BF16) and within(dx.bfloat16(), dx, dxa, REL_BF16, C_BF16)
    assert all(within(G.float(), G, T, 0.0, C_W) for G, T in zip(gs, ga))
    # 1. one image's contribution dropped from the weight gradient of a 200-image layer (one partial slab lost in a reduction)
    one = _wgrad(x64[150:151], dy64[150:151], 5)
    assert not within((gs[1] - one).float(), gs[1], ga[1], 0.0, C_W)
    assert not within((gs[1] + one).float(), gs[1], ga[1], 0.0, C_W)           # ... or counted twice
    # 2. one 32-channel chunk of one image's output zeroed
    bad = y.clone(); bad[17, :, :, 32:64] = 0
    assert not within(bad.bfloat16(), y, ya, REL_BF16, C_BF16)
    bad = dx.clone(); bad[120, :, :, 0:32] = 0
    assert not within(bad.bfloat16(), dx, dxa, REL_BF16, C_BF16)
    # 3. the two images of a 16 x 16 pair swapped
    bad = y.clone(); bad[[40, 41]] = bad[[41, 40]]
    assert not within(bad.bfloat16(), y, ya, REL_BF16, C_BF16)
    # 4. the taps of one kernel-size group shifted by one pixel
    bad = y.clone(); bad[97:200] = _conv(x64[97:200], w64[1], shift=1)
    assert not within(bad.bfloat16(), y, ya, REL_BF16, C_BF16)
    # 5. an expert without rows must have an exactly zero weight gradient
    z = torch.zeros_like(gs[0]); zt = torch.zeros_like(ga[0])
    assert within(z.float(), z, zt, 0.0, C_W) and not within((z + 1e-30).float(), z, zt, 0.0, C_W)


def test_kernel_selection_counters_read_and_reset():
    """The counters are host memory: readable and resettable without a GPU; the names come from include/hdmoe.h."""
    from hdmoe_hip import ops
    c = ops.kernel_selections(reset=True)
    assert {"conv7_32", "conv7_16", "conv6", "conv6s", "bwd7_32", "bwd7_32_wgrad8", "bwd7_32_wgrad7", "bwd7_16_ot1", "bwd7_16_ot2", "bwd6",
            "bwd6s", "wgrad6_direct", "wgrad6_defer", "blk6", "wgrad8_c11", "wgrad8_c12", "wgrad8_c21", "wgrad8_c22"} <= set(c)
    assert all(v == 0 for v in ops.kernel_selections().values())


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    yield
    if _measured:
        worst = {}
        for v in _measured.values():
            for k_, c in v.items():
                if k_.startswith("c_"):
                    worst[k_] = max(worst.get(k_, 0.0), c)
        os.makedirs(OUT_DIR, exist_ok=True)
        with open(os.path.join(OUT_DIR, "streaming_strict.json"), "w") as f:
            json.dump(dict(cases=_measured, worst=worst, bounds=dict(C_BF16=C_BF16, C_W=C_W)), f, indent=1, sort_keys=True)


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


OP = [  # N, R, Cin, Cout, kernel sizes, segment ends, residual, expected forward kernel ("conv7_32" / "conv7_16" / "conv6")
    (300, 32, 32, 32, (3, 3, 5, 5), (70, 150, 210, 300), True, "conv7_32"),
    (200, 32, 64, 64, (3, 5), (90, 200), True, "conv7_32"),
    (210, 32, 96, 32, (5, 3), (100, 210), False, "conv7_32"),
    (200, 32, 32, 96, (3, 3, 5, 5), (40, 40, 130, 200), True, "conv7_32"),      # an expert without rows; three 32-channel output blocks
    (196, 32, 32, 32, (3, 5, 7), (60, 130, 196), False, "conv7_32"),            # kernel-size set {3, 5, 7} (kmask 7)
    (301, 16, 64, 64, (3, 3, 5, 5), (70, 151, 210, 301), True, "conv7_16"),    # odd groups: pairs with an absent second image
    (200, 16, 128, 64, (3, 5), (99, 200), False, "conv7_16"),
    (191, 32, 64, 64, (3, 5), (90, 191), True, "conv6"),                        # one image below C7_MIN_IMAGES ...
    (192, 32, 64, 64, (3, 5), (90, 192), True, "conv7_32"),                     # ... and at it
    (201, 16, 64, 96, (3, 3, 5, 5), (1, 1, 100, 201), False, "conv7_16"),      # odd N on 16 x 16, experts with 1 and 0 rows, Cout = 96
    (192, 32, 256, 256, (3, 5), (100, 192), False, "conv7_32"),                 # the domain's upper edge
    (192, 16, 256, 256, (5, 3), (95, 192), True, "conv7_16"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,R,Cin,Cout,ks,split,res,kern", OP, ids=[f"{c[0]}x{c[1]}_{c[2]}to{c[3]}_k{''.join(map(str, c[4]))}" for c in OP])
def test_conv_op_forward_dgrad_wgrad_elementwise(gpu, N, R, Cin, Cout, ks, split, res, kern):
    """ops.mp_conv forward + backward without a weight bank: the forward and the input gradient through hdmoe_conv_fwd (conv7 or conv6), the
    weight gradient through hdmoe_conv_wgrad6 with its own reduction (the general kernel for 7x7)."""
    from hdmoe_hip import ops
    seg = [0] + list(split)
    x, ws, dy = _operands(N, R, Cin, Cout, ks, N + R + Cin)
    rs = torch.randn(N, R, R, Cout, generator=torch.Generator().manual_seed(N)).bfloat16() if res else None
    alpha, beta = (_f32(0.7), _f32(0.6)) if res else (1.0, 0.0)
    xd = x.cuda().requires_grad_(True)
    wd = [torch.nn.Parameter(w.float().cuda()) for w in ws]
    segd = torch.tensor(seg, dtype=torch.int32, device="cuda")
    before = ops.kernel_selections()
    y = ops.mp_conv(xd, wd, 1.0, seg=segd, res=None if rs is None else rs.cuda(), alpha=alpha, beta=beta, normalize=False)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    sel = _delta(before, ops.kernel_selections())
    # forward and input gradient: two launches of the expected conv program; weight gradient: wgrad6 (+ its reduction), or the general
    # kernel for a 7x7 class (outside wgrad6's domain); no fused backward here (no weight bank)
    assert sel.get(kern) == 2, sel
    assert sel.get("wgrad6_direct", 0) == (0 if 7 in ks else 1), sel
    assert not any(k.startswith("bwd") for k in sel), sel
    d = "cuda"
    ref = reference(x.double().to(d), dy.double().to(d), [w.double().to(d) for w in ws], seg,
                    None if rs is None else rs.double().to(d), alpha, beta)
    yr, ya, dxr, dxa, gs, ga = ref
    m = {"c_y": needed_c(y.detach(), yr, ya, REL_BF16), "c_dx": needed_c(xd.grad, dxr, dxa, REL_BF16)}
    for g, k in enumerate(ks):
        got = wd[g].grad.permute(2, 3, 0, 1).reshape(k * k, Cout, Cin)     # (O, I, k, k) -> [tap][O][I]
        m[f"c_w{g}"] = needed_c(got, gs[g], ga[g], 0.0)
    m["selections"] = sel
    _measured[f"op_{N}x{R}_{Cin}to{Cout}_k{''.join(map(str, ks))}"] = m
    assert m["c_y"] <= C_BF16 and m["c_dx"] <= C_BF16, m
    assert all(m[f"c_w{g}"] <= C_W for g in range(len(ks))), m


BWD = [  # N, R, Cin, Cout, kernel sizes, segment ends, expected counters
    (300, 32, 32, 32, (3, 3, 5, 5), (70, 150, 210, 300), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c11", "bwd7_32_wgrad7")),
    (210, 32, 64, 64, (3, 3, 5, 5), (50, 110, 160, 210), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c22", "bwd7_32_wgrad7")),
    (200, 32, 128, 128, (3,), (200,), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c22")),              # one class alone (router-trunk shape)
    (200, 32, 64, 128, (3, 3), (80, 200), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c22")),
    (200, 32, 32, 64, (3, 5), (100, 200), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c12", "bwd7_32_wgrad7")),
    (200, 32, 128, 32, (5, 3), (90, 200), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c21", "bwd7_32_wgrad7")),
    (200, 32, 96, 32, (5, 3), (200, 200), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c11", "bwd7_32_wgrad7")),   # the 3x3 expert without rows
    (200, 32, 32, 32, (5,), (200,), ("bwd7_32", "bwd7_32_wgrad7")),                               # wgrad7 alone
    (300, 16, 64, 64, (3, 5), (140, 300), ("bwd7_16_ot2",)),
    (201, 16, 64, 32, (3, 3, 5, 5), (1, 1, 100, 201), ("bwd7_16_ot1",)),                         # odd N, experts with 1 and 0 rows
    (200, 16, 32, 96, (5, 3), (99, 200), ("bwd7_16_ot1",)),
    (191, 32, 64, 64, (3, 5), (90, 191), ("bwd6",)),                                              # below C7_MIN_IMAGES: the conv6 dgrad
    (192, 32, 64, 64, (3, 5), (90, 192), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c22", "bwd7_32_wgrad7")),
    (192, 32, 256, 256, (3, 5), (100, 192), ("bwd7_32", "bwd7_32_wgrad8", "wgrad8_c22", "bwd7_32_wgrad7")),
    (192, 16, 256, 256, (5, 3), (95, 192), ("bwd7_16_ot2",)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,R,Cin,Cout,ks,split,expect", BWD, ids=[f"{c[0]}x{c[1]}_{c[2]}to{c[3]}_k{''.join(map(str, c[4]))}" for c in BWD])
def test_fused_backward_elementwise(gpu, N, R, Cin, Cout, ks, split, expect):
    """hdmoe_conv_bwd6 (dgrad program + weight-gradient programs in one grid, partial slabs deferred) followed by
    hdmoe_conv_wgrad6_reduce_batch, as the weight bank issues them."""
    import ctypes
    from hdmoe_hip import ops
    from hdmoe_hip._lib import _int_array, call, lib
    from hdmoe_hip.bank import w6_record
    seg = [0] + list(split)
    x, ws, dy = _operands(N, R, Cin, Cout, ks, N + Cin + 7)
    E, O, I = len(ks), Cout, Cin
    Opad = (O + 15) // 16 * 16
    taps = max(k * k for k in ks)
    wstride, wdstride = taps * O * I, taps * I * Opad
    wf = torch.empty(E * wstride, dtype=torch.bfloat16, device="cuda")
    wdi = torch.empty(E * wdstride, dtype=torch.bfloat16, device="cuda")
    call("hdmoe_wprep_fwd", [w.float().cuda() for w in ws], None, 1.0, list(ks), list(ks), E, O, I, I, Opad, wf, wstride, wdi, wdstride, 0, 0, 1, 1)
    kib = lib().hdmoe_conv_wgrad6_ws_kib(E, N, R, R, I, O, ctypes.cast(_int_array(ks), ctypes.c_void_p), ctypes.cast(_int_array(ks), ctypes.c_void_p), 1)
    assert kib > 0
    wsb = torch.full((2 * kib * 256,), float("nan"), dtype=torch.float32, device="cuda")   # every slab the reduction reads must be written
    Gs = [torch.zeros(k * k, O, I, device="cuda") for k in ks]
    segd = torch.tensor(seg, dtype=torch.int32, device="cuda")
    xd, dyd = x.cuda(), dy.cuda()
    dx = torch.full_like(xd, float("nan"))
    pts = [(k - 1) // 2 for k in ks]
    before = ops.kernel_selections()
    rc = call("hdmoe_conv_bwd6", xd, dyd, wdi, dx, Gs, segd, E, wdstride, N, R, R, I, O, list(ks), list(ks), pts, pts, 1.0, wsb, wsb.numel() * 4, 1)
    assert rc == 0
    call("hdmoe_conv_wgrad6_reduce_batch", Gs + [None] * (8 - E), [segd], [wsb], w6_record(E, N, R, R, I, O, 1, ks), 1)
    torch.cuda.synchronize()
    sel = _delta(before, ops.kernel_selections())
    assert sel == {k: 1 for k in expect}, sel
    _, _, dxr, dxa, gs, ga = reference(x.double().cuda(), dy.double().cuda(), [w.double().cuda() for w in ws], seg)
    m = {"c_dx": needed_c(dx, dxr, dxa, REL_BF16)}
    for g in range(E):
        m[f"c_w{g}"] = needed_c(Gs[g], gs[g], ga[g], 0.0)
    m["selections"] = sel
    _measured[f"bwd_{N}x{R}_{Cin}to{Cout}_k{''.join(map(str, ks))}"] = m
    assert m["c_dx"] <= C_BF16, m
    assert all(m[f"c_w{g}"] <= C_W for g in range(E)), m


@pytest.mark.gpu
def test_fused_backward_declines_7x7(gpu):
    """bwd7 / bwd6 have no 7x7 weight-gradient program: a {3, 5, 7} layer is outside hdmoe_conv_bwd6's domain (rc 1, nothing launched,
    no counter moves) and the caller takes conv7 for the input gradient plus the general weight gradient (test_conv_op_... k357)."""
    import ctypes
    from hdmoe_hip import ops
    from hdmoe_hip._lib import _int_array, call, lib
    ks, N, R, C = (3, 5, 7), 196, 32, 32
    assert lib().hdmoe_conv_wgrad6_ws_kib(3, N, R, R, C, C, ctypes.cast(_int_array(ks), ctypes.c_void_p), ctypes.cast(_int_array(ks), ctypes.c_void_p), 1) == 0
    x = torch.zeros(N, R, R, C, dtype=torch.bfloat16, device="cuda")
    wd = torch.zeros(3 * 49 * C * C, dtype=torch.bfloat16, device="cuda")
    Gs = [torch.zeros(k * k, C, C, device="cuda") for k in ks]
    segd = torch.tensor([0, 60, 130, N], dtype=torch.int32, device="cuda")
    wsb = torch.zeros(1 << 20, device="cuda")
    before = ops.kernel_selections()
    rc = call("hdmoe_conv_bwd6", x, x, wd, torch.empty_like(x), Gs, segd, 3, 49 * C * C, N, R, R, C, C, list(ks), list(ks), [1, 2, 3], [1, 2, 3],
              1.0, wsb, wsb.numel() * 4, 1)
    assert rc == 1 and _delta(before, ops.kernel_selections()) == {}
