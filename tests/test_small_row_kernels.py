"""The small-batch fp32 kernels of the serial conditioning stages against float64 on the CPU -- GPU.

* rowlin_f32_kernel (csrc/rowlin.hip): pointwise fp32 layers on at most 2048 positions, forward and input gradient (the same kernel on
  the flipped image [g][I][Opad]).  Every case first asks hdmoe_conv_fwd_route that the shape reaches it (Cin = 516 on one-position rows
  is glin_f32_kernel's by the order of the walk: asserted as such, and held to the same bound).  Bound per output, derived and not tuned: the products are exact fp32 and the K = Cin of them are summed in fp32 in some order, so
  |err| <= 2 K 2^-24 (|alpha| sum_i |x_i w_i| + |beta res|)   (the epilogue's two terms join the magnitudes the sum passes through).
  The padding columns of the weight image hold NaN: a read past Cin shows.  Row 0 of a P = 256 call equals the same row computed in a
  call of its own, bit for bit.
* lwg_f32_kernel on few positions (csrc/lwgrad.hip; 1 .. 256 positions, where its slices leave most waves idle): the same bound with
  K = P, into a non-zero slab.
* swg_f32_kernel (csrc/lwgrad.hip), the stem's weight gradient, in its 4-wave and 16-wave forms; hdmoe_wbank_prep's images and mutation.
* groupnorm_rows_bwd_kernel (csrc/norm.hip): GroupNorm(1, C) on single-position rows through ops.group_norm (the forward runs the image
  kernels), with the references, scales and K of tests/test_norm_kernels.py (imported, not restated).  The dispatch sits inside
  hdmoe_groupnorm_bwd (S == 1, G == 1, fp32, C % 4 == 0, C <= 1024, aligned pointers) and has no route query; C = 8, 512, 1024 are its
  1, 2 and 4 float4 pieces per lane.
"""
import ctypes

import pytest
import torch

import test_norm_kernels as TN
from test_weight_finish_kernels import SPLIT_REL

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
F32 = 0
FWD, FWD2, FWD3, FWD5, KGEMM, GLIN, ROWLIN = 0, 1, 2, 3, 7, 8, 10          # HDMOE_ROUTE_CONV_*
WG_LWG = 4                                                                # HDMOE_ROUTE_WGRAD_LWG


@pytest.fixture(scope="module")
def call():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    return call


def _ints(v):
    return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)


def _fwd_route(N, H, W, Cin, Ipad, Cout, G, has_seg, has_res, wstride, aligned=1):
    from hdmoe_hip._lib import lib
    r = (ctypes.c_int * 5)()
    one, zero = [1] * G, [0] * G
    assert lib().hdmoe_conv_fwd_route(ctypes.cast(r, ctypes.c_void_p), N, H, W, H, W, Cin, Cin, Ipad, Cout, Cout, 1, 0, G, has_seg, has_res, wstride,
                                      _ints(one), _ints(one), _ints(zero), _ints(zero), F32, aligned) == 0
    return tuple(r)


def _pad16(c):
    return (c + 15) // 16 * 16


def _linear_case(call, P, I, O, variant, gen, dgrad, hw=1):
    """One pointwise layer on P positions through hdmoe_conv_fwd; returns (y, ref, bound) on the CPU in fp64 (y as computed)."""
    G = 3 if variant & 2 else 1
    res_on = bool(variant & 1)
    alpha, beta = (0.75, -0.5) if res_on else (1.0, 0.0)
    if G == 1:                                                # ungrouped: one long row of P positions, the form ops.mp_conv presents a linear layer in
        N, hw = 1, P
    N = P // hw
    assert N * hw == P
    # glin_f32_kernel stands in front of the row GEMM in the walk and keeps its domain (one-position rows, 256 <= Cin <= 1024): there the
    # query must name it, and the result is held to the same bound
    want = (GLIN, (I + 255) // 256) if hw == 1 and 256 <= I <= 1024 else (ROWLIN, 32)
    x = torch.randn(P, I, generator=gen)
    if dgrad:                                                 # the layer maps O -> I channels, weight [I][O]; x is its dy, and its flipped
        w = (torch.randn(G, I, O, generator=gen) / I ** 0.5).transpose(1, 2).contiguous()   # image [g][tap'][O][pad16(I)] holds the transpose
    else:
        w = torch.randn(G, O, I, generator=gen) / I ** 0.5
    res = torch.randn(P, O, generator=gen)
    Ipad = _pad16(I)
    img = torch.full((G, 1, O, Ipad), float("nan"))
    img[:, 0, :, :I] = w
    wstride = O * Ipad
    b = N // 2 + 1 if N > 1 else 1                            # groups: [0, b), empty, [b, N): the boundary falls inside a 32-row tile
    bounds = [0, b, b, N]
    seg = torch.tensor(bounds, dtype=torch.int32, device=DEV) if G > 1 else None
    route = _fwd_route(N, 1, hw, I, Ipad, O, G, G > 1, res_on, wstride)
    assert route[:2] == want, (P, I, O, variant, route)
    y = torch.full((P, O), float("nan"), device=DEV)
    one, zero = [1] * G, [0] * G
    call("hdmoe_conv_fwd", x.to(DEV), img.to(DEV), y, res.to(DEV) if res_on else None, alpha, beta, seg, G, wstride, N, 1, hw, 1, hw, I, I, Ipad, O, O,
         1, 0, one, one, zero, zero, F32)
    xd, wd = x.double(), w.double()
    ref, mag = torch.empty(P, O, dtype=torch.float64), torch.empty(P, O, dtype=torch.float64)
    for g in range(G):
        rows = slice(bounds[g] * hw, bounds[g + 1] * hw) if G > 1 else slice(0, P)
        ref[rows] = xd[rows] @ wd[g].T
        mag[rows] = xd[rows].abs() @ wd[g].abs().T
    ref = alpha * ref + beta * res.double()
    bound = 2.0 * I * U * (abs(alpha) * mag + abs(beta) * res.double().abs())
    return y.cpu().double(), ref, bound


ROW_PS = [1, 31, 33, 256, 2048]
ROW_IS = [32, 36, 128, 516]
ROW_OS = [1, 2, 31, 32, 33, 96]


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("P", ROW_PS)
def test_row_gemm_matches_fp64(call, P, dgrad):
    gen = torch.Generator().manual_seed(1000 + P + (7 if dgrad else 0))
    worst = 0.0
    for ii, I in enumerate(ROW_IS):
        for oi, O in enumerate(ROW_OS):
            variant = (ii + oi + (1 if dgrad else 0)) % 4      # 0 plain, 1 res + alpha + beta, 2 seg over 3 groups, 3 both
            hw = 4 if (variant & 2) and P % 4 == 0 and oi % 2 else 1     # (seg counts rows of H * W positions)
            y, ref, bound = _linear_case(call, P, I, O, variant, gen, dgrad, hw)
            assert torch.isfinite(y).all(), (P, I, O, variant)
            ratio = float(((y - ref).abs() / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"P={P} I={I} O={O} variant={variant} hw={hw}: |err| / bound = {ratio:.3f}"
    print(f"row gemm {'dgrad' if dgrad else 'fwd'} P={P}: worst |err| / bound = {worst:.4f}")


def test_row_gemm_all_variants_at_every_tile_edge(call):
    """Each of the four variants (res, seg) at the shapes around the tile edges, which the rotation above gives one variant each."""
    gen = torch.Generator().manual_seed(77)
    for P in (33, 256):
        for I, O in ((36, 33), (128, 2), (516, 96)):
            for variant in range(4):
                y, ref, bound = _linear_case(call, P, I, O, variant, gen, False, 4 if (variant & 2) and P % 4 == 0 else 1)
                ratio = float(((y - ref).abs() / bound.clamp_min(1e-300)).max())
                assert torch.isfinite(y).all() and ratio <= 1.0, (P, I, O, variant, ratio)


def test_row_gemm_rows_outside_every_group_stay_untouched(call):
    P, I, O, G = 70, 64, 40, 2
    gen = torch.Generator().manual_seed(5)
    x, w = torch.randn(P, I, generator=gen), torch.randn(G, 1, O, I, generator=gen)
    seg = torch.tensor([3, 40, 66], dtype=torch.int32, device=DEV)
    assert _fwd_route(P, 1, 1, I, I, O, G, 1, 0, O * I)[0] == ROWLIN
    y = torch.full((P, O), -7.0, device=DEV)
    call("hdmoe_conv_fwd", x.to(DEV), w.to(DEV), y, None, 1.0, 0.0, seg, G, O * I, P, 1, 1, 1, 1, I, I, I, O, O, 1, 0, [1, 1], [1, 1], [0, 0], [0, 0], F32)
    y = y.cpu()
    assert bool((y[:3] == -7.0).all()) and bool((y[66:] == -7.0).all())
    for g, (a, b) in enumerate(((3, 40), (40, 66))):
        ref, mag = x[a:b].double() @ w[g, 0].double().T, x[a:b].double().abs() @ w[g, 0].double().abs().T
        assert bool(((y[a:b].double() - ref).abs() <= 2.0 * I * U * mag).all())


def test_row_gemm_is_batch_independent(call):
    gen = torch.Generator().manual_seed(11)
    for I, O in ((32, 2), (516, 33), (128, 96)):
        Ipad = _pad16(I)
        x = torch.randn(256, I, generator=gen).to(DEV)
        w = torch.zeros(1, 1, O, Ipad)
        w[0, 0, :, :I] = torch.randn(O, I, generator=gen)
        w = w.to(DEV)
        ys = []
        for P in (256, 1):
            H = 2 if P == 1 and 256 <= I <= 1024 else 1       # (one position of Cin = 516 is glin's as a 1 x 1 map; as half of a 2 x 1 map it is not)
            assert _fwd_route(1, H, P, I, Ipad, O, 1, 0, 0, O * Ipad)[0] == ROWLIN
            y = torch.empty(H * P, O, device=DEV)
            xs = x[:H * P].contiguous()
            call("hdmoe_conv_fwd", xs, w, y, None, 1.0, 0.0, None, 1, O * Ipad, 1, H, P, H, P, I, I, Ipad, O, O, 1, 0, [1], [1], [0], [0], F32)
            ys.append(y.cpu())
        assert torch.equal(ys[0][:1], ys[1][:1]), (I, O)


def test_shapes_outside_the_row_gemm_answer_another_family(call):
    others = {FWD, FWD2, FWD3, FWD5, KGEMM, GLIN}
    assert _fwd_route(2049, 1, 1, 64, 64, 64, 1, 0, 0, 64 * 64)[0] in others          # P > 2048
    assert _fwd_route(256, 1, 1, 30, 32, 64, 1, 0, 0, 64 * 32)[0] in others           # Cin < 32 and Cin % 4
    assert _fwd_route(256, 1, 1, 64, 64, 64, 1, 0, 0, 64 * 64, aligned=0)[0] in others  # a misaligned pointer
    assert _fwd_route(256, 1, 1, 64, 64, 64, 1, 0, 0, 64 * 64)[0] == ROWLIN
    # and the misaligned call still computes the layer (on the family the query named)
    gen = torch.Generator().manual_seed(3)
    P, I, O = 40, 64, 64
    x, w = torch.randn(P, I, generator=gen), torch.randn(O, I, generator=gen)
    base = torch.zeros(P * I + 8, device=DEV)
    base[1:1 + P * I] = x.reshape(-1).to(DEV)
    xv = base[1:1 + P * I].view(P, I)
    assert xv.data_ptr() % 16 != 0
    y = torch.full((P, O), float("nan"), device=DEV)
    call("hdmoe_conv_fwd", xv, w.to(DEV), y, None, 1.0, 0.0, None, 1, O * I, P, 1, 1, 1, 1, I, I, I, O, O, 1, 0, [1], [1], [0], [0], F32)
    ref, mag = x.double() @ w.double().T, x.double().abs() @ w.double().abs().T
    assert bool(((y.cpu().double() - ref).abs() <= 2.0 * I * U * mag).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient on few positions
WG_SHAPES = [(32, 32), (64, 128), (512, 1024)]


@pytest.mark.parametrize("grouped", [False, True], ids=["one-group", "grouped"])
@pytest.mark.parametrize("P", [1, 64, 65, 256])
def test_pointwise_wgrad_few_positions(call, P, grouped):
    from hdmoe_hip._lib import lib
    gen = torch.Generator().manual_seed(200 + P + (1 if grouped else 0))
    G = 3 if grouped else 1
    b = P // 2 + 1 if P > 1 else 1
    bounds = [0, b, b, P] if grouped else [0, P]
    for I, O in WG_SHAPES:
        r = (ctypes.c_int * 34)()
        one, zero = [1] * G, [0] * G
        assert lib().hdmoe_conv_wgrad_route(ctypes.cast(r, ctypes.c_void_p), P, 1, 1, 1, 1, I, I, O, 1, 0, G, int(grouped), _ints(one), _ints(one),
                                            _ints(zero), _ints(zero), F32, 1) == 0
        assert r[0] == WG_LWG, (P, I, O, r[0])
        x, dy = torch.randn(P, I, generator=gen), torch.randn(P, O, generator=gen)
        pre = torch.randn(G, O, I, generator=gen)
        slabs = [pre[g].clone().to(DEV) for g in range(G)]
        seg = torch.tensor(bounds, dtype=torch.int32, device=DEV) if grouped else None
        call("hdmoe_conv_wgrad", x.to(DEV), dy.to(DEV), slabs, seg, G, P, 1, 1, 1, 1, I, I, O, 1, 0, one, one, zero, zero, F32)
        for g in range(G):
            rows = slice(bounds[g], bounds[g + 1])
            ref = dy[rows].double().T @ x[rows].double()
            mag = dy[rows].double().abs().T @ x[rows].double().abs()
            err = (slabs[g].cpu().double() - (pre[g].double() + ref)).abs()
            bound = 2.0 * P * U * (mag + pre[g].double().abs())   # (the slab's own value is one more term of the sum)
            ratio = float((err / bound.clamp_min(1e-300)).max())
            assert ratio <= 1.0, f"P={P} I={I} O={O} group {g}: |err| / bound = {ratio:.3f}"


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm(1, C) on single-position rows
def _gn_rows_inputs(N, C, act, seed):
    """Inputs of TN._gn_make; under ReLU the elements whose fp64 pre-activation lies within twice the forward bound of zero are moved
    (a handful among N * C), until none is left -- the condition TN._gn_check asserts."""
    x, gm, bt, g = TN._gn_make(N, 1, C, 1, act, torch.float32, seed)
    if act != TN.RELU:
        return x, gm, bt, g
    for _ in range(16):
        z = TN._gn_ref(x, gm, bt, g, 1, act)["z"]
        tau = TN.K_Y * TN.U * (z.abs() + 1.0 + float(z.abs().max()))
        near = z.abs() <= 4 * tau
        if not bool(near.any()):
            return x, gm, bt, g
        x = torch.where(near, x + 0.05, x).float()
    raise AssertionError("no ReLU-safe inputs")


@pytest.mark.parametrize("act", [TN.NONE, TN.RELU], ids=["none", "relu"])
@pytest.mark.parametrize("C", [8, 512, 1024])
@pytest.mark.parametrize("N", [1, 3, 256])
def test_group_norm_single_position_rows(call, N, C, act):
    x, gm, bt, g = _gn_rows_inputs(N, C, act, 900 + N + C)
    tag = f"group_norm rows {(N, C, act)}"
    got = TN._gn_hip(x, gm, bt, g, 1, act, torch.float32)
    TN._gn_check(tag, got, x, gm, bt, g, 1, act, torch.float32)


def test_group_norm_rows_add_to_existing_grads(call):
    for N, C in ((3, 8), (256, 512), (11, 1024)):
        x, gm, bt, g = TN._gn_make(N, 1, C, 1, TN.NONE, torch.float32, 47 + C)
        ref, sc = TN._gn_ref(x, gm, bt, g, 1, TN.NONE), TN._gn_scales(x, gm, bt, g, 1, TN.NONE)
        xd = x.to(DEV).requires_grad_(True)
        gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
        for _ in range(2):
            TN._ops().group_norm(xd, gd, bd, 1, TN.NONE, TN.EPS).backward(g.to(DEV))
        TN._match(gd.grad, 2 * ref["dg"], TN._bound(2 * ref["dg"], 2 * sc["dg"], TN.K_SUM), f"rows {(N, C)}: dgamma after two backwards")
        TN._match(bd.grad, 2 * ref["db"], TN._bound(2 * ref["db"], 2 * sc["db"], TN.K_SUM), f"rows {(N, C)}: dbeta after two backwards")


# ---------------------------------------------------------------------------------------------------------------------------------
# weight-bank prepare (csrc/wbank.hip): several tensors in one launch
WB_FANS = [(36, 1), (36, 9), (576, 1), (576, 9), (3200, 1), (3200, 25), (3201, 1)]        # (fan-in, taps = kh * kw): I = fan-in / taps
WB_OS = [2, 16, 17, 33]
WB_DTYPES = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "split": (2, torch.bfloat16)}


def _bf16_ulp(r):
    return torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(1e-300))) - 7.0)


@pytest.mark.parametrize("mutate", [0, 1], ids=["keep", "mutate"])
@pytest.mark.parametrize("normalize", [1, 0], ids=["norm", "plain"])
@pytest.mark.parametrize("dt", list(WB_DTYPES))
def test_bank_prepare_images(call, dt, normalize, mutate):
    """Every (fan-in, taps, O) tensor in ONE launch.  The forward image [tap][O][Ipad] and the flipped image [tap'][I][Opad] must hold the
    same bits at corresponding indices (any relayout error shows without a reference); the rows must match the fp64 normalisation to
    4 * 2^-24 relative (fp32 images) or one bf16 ulp (bf16 images and the hi plane of split), hi + lo of split to SPLIT_REL; a mutating prepare must leave w_raw rows
    of the fp64 computation's norm to 1e-6, and its images are held to the fp64 normalisation of the rows it stored -- the parameter is
    the forward's input, as in the reference; measured from the rows BEFORE the mutation instead, the stored rows' own fp32 rounding adds
    to the error and the worst fp32 element came out at 4.17 * 2^-24.
    One tensor lists only its rows 5 .. O - 1: the others stay as they were (zero)."""
    import numpy as np
    from hdmoe_hip.bank import _DESC
    code, idt = WB_DTYPES[dt]
    planes = 2 if dt == "split" else 1
    gen = torch.Generator().manual_seed(17 + code)
    gain = 1.75                                              # (exact in fp32, the type the descriptor carries it in)
    tens, rows = [], []
    descs = np.zeros(len(WB_FANS) * len(WB_OS), dtype=_DESC)
    for fan, taps in WB_FANS:
        for O in WB_OS:
            I, k = fan // taps, int(round(taps ** 0.5))
            Ipad, Opad = _pad16(I), _pad16(O)
            w = (torch.randn(O, I, k, k, generator=gen) * (0.2 + 2.0 * torch.rand(O, 1, 1, 1, generator=gen))).to(DEV)
            wf = torch.zeros(planes * taps * O * Ipad, dtype=idt, device=DEV)
            wd = torch.zeros(planes * taps * I * Opad, dtype=idt, device=DEV)
            first = 5 if (fan, taps, O) == (576, 9, 33) else 0
            di = len(tens)
            d = descs[di]
            d["w_raw"], d["wf"], d["wd"] = w.data_ptr(), wf.data_ptr(), wd.data_ptr()
            d["O"], d["I"], d["kh"], d["kw"], d["Ipad"], d["Opad"] = O, I, k, k, Ipad, Opad
            d["dtype"], d["normalize"], d["mutate_ok"], d["gain"], d["out_scale"] = code, normalize, 1, gain, 1.0
            d["wf_plane"], d["wd_plane"] = taps * O * Ipad, taps * I * Opad
            rows.extend((di, o) for o in range(first, O))
            tens.append((fan, taps, O, I, Ipad, Opad, first, w, w.detach().cpu().double().reshape(O, fan), wf, wd))
    dd = torch.from_numpy(descs.view(np.uint8).copy()).to(DEV)
    rr = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).contiguous().to(DEV)
    call("hdmoe_wbank_prep", dd, rr, len(rows), mutate)
    torch.cuda.synchronize()
    worst = 0.0
    for fan, taps, O, I, Ipad, Opad, first, w, w0, wf, wd in tens:
        tag = f"{dt} fan {fan} taps {taps} O {O}"
        f = wf.view(planes, taps, O, Ipad).cpu()
        b = wd.view(planes, taps, I, Opad).cpu()
        # the same bits in both images: wf[t][o][i] == wd[taps - 1 - t][i][o]; pads and unlisted rows zero
        fb, bb = f.view(torch.int16 if idt == torch.bfloat16 else torch.int32), b.view(torch.int16 if idt == torch.bfloat16 else torch.int32)
        assert torch.equal(fb[:, :, :, :I], bb.flip(1)[:, :, :, :O].transpose(2, 3)), f"{tag}: forward and flipped image differ"
        assert not bool(fb[:, :, :, I:].any()) and not bool(bb[:, :, :, O:].any()) and not bool(fb[:, :, :first].any()), f"{tag}: pads / unlisted rows written"
        c = fan ** -0.5
        ref = w0.clone()
        if normalize:
            inv = 1.0 / (1e-4 + w0.norm(dim=1, keepdim=True) * c)
            if mutate:
                wm = w0 * inv
                stored = w.detach().cpu().double().reshape(O, fan)
                got_n, want_n = stored[first:].norm(dim=1), wm[first:].norm(dim=1)
                assert bool(((got_n - want_n).abs() <= 1e-6 * want_n).all()), f"{tag}: norm of the mutated rows"
                assert torch.equal(stored[:first], w0[:first]), f"{tag}: unlisted rows mutated"
                # the forward's weight is the normalisation of the parameter AS STORED (reference model_internals.py:254-259: copy_ the
                # normalised weights into the fp32 parameter, then normalise the parameter): fp64 from the stored rows
                wm = torch.cat([w0[:first], stored[first:]])
                inv = 1.0 / (1e-4 + wm.norm(dim=1, keepdim=True) * c)
                ref = wm * inv * gain * c
            else:
                ref = w0 * inv * gain * c
        if not (normalize and mutate):
            assert torch.equal(w.detach().cpu().double().reshape(O, fan), w0), f"{tag}: w_raw changed"
        ref = ref.view(O, I, taps).permute(2, 0, 1)[:, first:]            # [tap][o][i]
        got = f[0, :, first:, :I].double()
        if dt == "fp32":
            ratio = float(((got - ref).abs() / (4.0 * U * ref.abs()).clamp_min(1e-300)).max())
        else:
            ratio = float(((got - ref).abs() / _bf16_ulp(ref)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
        if dt == "split":
            # the lo plane against the reference: two roundings to nearest leave at most 2^-17 |v| of the fp32 value v (attained), and v is
            # within 4 * 2^-24 of the reference -- the derivation stands at SPLIT_REL in tests/test_weight_finish_kernels.py.  (The flipped
            # image's lo plane is tied to this one bit for bit above.)
            lo = f[1, :, first:, :I].double()
            r_lo = float(((got + lo - ref).abs() / (SPLIT_REL * ref.abs()).clamp_min(1e-300)).max())
            assert r_lo <= 1.0, f"{tag}: |hi + lo - ref| / (SPLIT_REL |ref|) = {r_lo:.3f}"
    print(f"bank prepare {dt} normalize={normalize} mutate={mutate}: worst |err| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# stem weight gradient (swg_f32_kernel, csrc/lwgrad.hip)
WG_SWG = 2                                                                # HDMOE_ROUTE_WGRAD_SWG
STEM_MAPS = [(2, 8, 8), (2, 8, 40), (2, 32, 32), (64, 32, 32)]            # (N, H, W); the last: 256 pixels per workgroup, its 16-wave form


@pytest.mark.parametrize("Cin", [3, 4])
@pytest.mark.parametrize("N,H,W", STEM_MAPS, ids=["x".join(map(str, m)) for m in STEM_MAPS])
def test_stem_weight_gradient(call, N, H, W, Cin):
    """fp32 3 x 3 "same" layer Cin -> 32: G[tap][o][i] += sum_p dy[p][o] x[p + tap][i] into a non-zero slab, against fp64 autograd; bound as
    for the row GEMM with K = N H W terms per output."""
    import torch.nn.functional as F
    from hdmoe_hip._lib import lib
    O = 32
    r = (ctypes.c_int * 34)()
    assert lib().hdmoe_conv_wgrad_route(ctypes.cast(r, ctypes.c_void_p), N, H, W, H, W, Cin, Cin, O, 1, 0, 1, 0, _ints([3]), _ints([3]), _ints([1]),
                                        _ints([1]), F32, 1) == 0
    assert r[0] == WG_SWG, r[0]
    gen = torch.Generator().manual_seed(300 + N + H + W + Cin)
    x, dy = torch.randn(N, H, W, Cin, generator=gen), torch.randn(N, H, W, O, generator=gen)
    pre = torch.randn(9, O, Cin, generator=gen)
    slab = pre.clone().to(DEV)
    call("hdmoe_conv_wgrad", x.to(DEV), dy.to(DEV), [slab], None, 1, N, H, W, H, W, Cin, Cin, O, 1, 0, [3], [3], [1], [1], F32)

    def wgrad(xx, dd):
        w = torch.zeros(O, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx.permute(0, 3, 1, 2), w, padding=1).backward(dd.permute(0, 3, 1, 2))
        return w.grad.permute(2, 3, 0, 1).reshape(9, O, Cin)
    ref, mag = wgrad(x.double(), dy.double()), wgrad(x.double().abs(), dy.double().abs())
    err = (slab.cpu().double() - (pre.double() + ref)).abs()
    bound = 2.0 * (N * H * W) * U * (mag + pre.double().abs())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"stem wgrad {(N, H, W, Cin)}: worst |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0
