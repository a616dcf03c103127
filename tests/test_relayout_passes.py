"""Data-movement passes around the expert banks, 16-byte forms (csrc/relayout.hip) -- GPU.

Every new kernel is run next to the kernel it replaces (kept as the fallback) on the same inputs, and its output is compared BIT FOR BIT:

* hdmoe_patch_relayout_tiled against hdmoe_patch_relayout, order 1 (PixelShuffle), both directions, at the bench shapes (B = 256,
  32 x 32 and 16 x 16 maps, C = 32, bf16) for the patch sizes of its domain (8, 16), in fp32, and on images that do not divide into
  patches (zero-filled tokens one way, cropped image the other); guard regions around the outputs must stay untouched;
* hdmoe_combine_rows_fwd_vec / _bwd_vec against hdmoe_combine_rows_fwd / _bwd on ragged plans (an expert without rows, samples routed to
  fewer than kcap experts or to none), with and without weights: out and dys bit for bit;
* the selection counters (ops.kernel_selections) assert which kernel ran, in the direct calls and through the autograd functions, and that
  the declined shapes (p = 4 in bf16, C not a multiple of the vector width, order 0, L not a whole number of vectors) launch nothing
  new and take the old kernel.

dsparse of the combine backward is a dot product whose per-(row, chunk) partial sums meet through a float atomic, so two runs of ONE kernel
may differ.  The yardstick is measured in the test: `spread` = the largest difference between two runs of the predecessor on the same
input, and each kernel's largest error against fp64 (from the same rounded operands), both relative to sum_i |dout||ys| of the element.
The new kernel's error must not exceed twice the predecessor's.  Every figure is printed before the assertion (run with -s).
Measured on an MI355X at B = 256, kcap = 2, L = 32768, bf16 (relative to sum_i |dout||ys|, largest over the 320 routed entries):
predecessor run-to-run spread 2.9e-9, predecessor error against fp64 2.1e-9 (so the bound is 4.2e-9, the size of one fp32 rounding of a
partial sum, not a vacuous one); new kernel error against fp64 2.6e-9, new run-to-run spread 1.5e-9.
"""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
_measured = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    yield
    if _measured:
        print("\nrelayout_passes measured: " + json.dumps(_measured, sort_keys=True))


def _guarded(n, dtype, mark):
    buf = torch.full((GUARD + n + GUARD,), mark, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n, mark):
    return bool((buf[:GUARD] == mark).all()) and bool((buf[GUARD + n:] == mark).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _relayout_pair(N, H, W, C, p, dtype, to_img, order=1):
    """Runs the tiled and the old kernel on the same input.  Returns (rc of the tiled call, new output, old output, counter delta)."""
    from hdmoe_hip._lib import call, dtype_code
    from hdmoe_hip import ops
    hp, wp = -(-H // p), -(-W // p)
    gen = torch.Generator().manual_seed(N * 131 + H * 17 + p)
    n_img, n_tok = N * H * W * C, N * hp * wp * C * p * p
    src = torch.randn(n_tok if to_img else n_img, generator=gen).to(dtype).to(DEV)
    n_out = n_img if to_img else n_tok
    mark = 777.0
    outs = []
    before = ops.kernel_selections()["relayout_tiled"]
    rc = None
    for name in ("hdmoe_patch_relayout_tiled", "hdmoe_patch_relayout"):
        buf, out = _guarded(n_out, dtype, mark)
        if not to_img and name == "hdmoe_patch_relayout":
            out.zero_()                                        # (as _PatchRelayoutFn.backward does for the padded canvas; the tiled
                                                               #  kernel must write the zeros of out-of-image positions itself)
        r = call(name, out, src, N, H, W, C, p, hp, wp, order, 1 if to_img else 0, dtype_code(dtype))
        torch.cuda.synchronize()
        assert _guards_ok(buf, n_out, mark), f"{name}: wrote outside its output"
        if rc is None:
            rc = r
        else:
            assert r == 0
        outs.append(out)
    return rc, outs[0], outs[1], ops.kernel_selections()["relayout_tiled"] - before, src


def _relayout_definition(src, N, H, W, C, p, to_img):
    """The order-1 relayout by torch indexing (on the device, exact): tok[b][ph][pw][c][i][j] <-> img[b][ph*p+i][pw*p+j][c]."""
    hp, wp = -(-H // p), -(-W // p)
    if to_img:
        t = src.view(N, hp, wp, C, p, p).permute(0, 1, 4, 2, 5, 3).reshape(N, hp * p, wp * p, C)
        return t[:, :H, :W].contiguous().view(-1)
    canvas = torch.zeros((N, hp * p, wp * p, C), dtype=src.dtype, device=src.device)
    canvas[:, :H, :W] = src.view(N, H, W, C)
    return canvas.view(N, hp, p, wp, p, C).permute(0, 1, 3, 5, 2, 4).contiguous().view(-1)


@pytest.mark.parametrize("to_img", [False, True], ids=["to_tokens", "to_image"])
@pytest.mark.parametrize("N,H,W,C,p,dtype", [
    (256, 32, 32, 32, 8, torch.bfloat16), (256, 32, 32, 32, 16, torch.bfloat16),       # the bench shapes of the domain
    (256, 16, 16, 32, 8, torch.bfloat16), (256, 16, 16, 32, 16, torch.bfloat16),
    (64, 32, 32, 32, 4, torch.float32), (64, 32, 32, 32, 8, torch.float32), (16, 16, 16, 32, 16, torch.float32),
    (5, 20, 27, 8, 8, torch.bfloat16),                          # image does not divide: zero-filled tokens / cropped image
    (3, 24, 72, 16, 8, torch.bfloat16),                         # a token row of more than one tile, the last one shorter
    (3, 48, 40, 8, 24, torch.bfloat16),                         # p outside the compile-time set
    (3, 10, 9, 8, 4, torch.float32),
], ids=lambda v: str(v).replace("torch.", ""))
def test_tiled_relayout_is_bit_identical(N, H, W, C, p, dtype, to_img):
    rc, new, old, ran, src = _relayout_pair(N, H, W, C, p, dtype, to_img)
    assert rc == 0 and ran == 1, "the tiled kernel declined a shape of its domain"
    assert torch.equal(_bits(new), _bits(old))
    assert torch.equal(_bits(new), _bits(_relayout_definition(src, N, H, W, C, p, to_img)))


@pytest.mark.parametrize("to_img", [False, True], ids=["to_tokens", "to_image"])
@pytest.mark.parametrize("N,H,W,C,p,dtype,order", [
    (256, 32, 32, 32, 4, torch.bfloat16, 1),                   # bench patch size 4: p % 8 != 0 in bf16
    (4, 16, 16, 12, 8, torch.bfloat16, 1),                     # C not a multiple of the vector width
    (4, 16, 16, 6, 4, torch.float32, 1),
    (4, 16, 16, 32, 8, torch.bfloat16, 0),                     # order 0 is a plain vector copy already
    (2, 32, 32, 32, 32, torch.bfloat16, 1),                    # one token = 64 KiB, above the tile limit
], ids=lambda v: str(v).replace("torch.", ""))
def test_tiled_relayout_declines_outside_its_domain(N, H, W, C, p, dtype, order, to_img):
    rc, new, old, ran, src = _relayout_pair(N, H, W, C, p, dtype, to_img, order)
    assert rc == 1 and ran == 0
    untouched = torch.full_like(new, 777.0)
    assert torch.equal(_bits(new), _bits(untouched)), "a declined call must launch nothing"
    if order == 1:
        assert torch.equal(_bits(old), _bits(_relayout_definition(src, N, H, W, C, p, to_img)))


def test_autograd_dispatch_takes_the_tiled_kernel_and_falls_back():
    from hdmoe_hip import ops
    N, H, W, C = 8, 32, 32, 32
    for p, dtype, tiled in ((8, torch.bfloat16, 1), (16, torch.bfloat16, 1), (4, torch.bfloat16, 0), (4, torch.float32, 1)):
        hp, wp = H // p, W // p
        gen = torch.Generator().manual_seed(p)
        tok = torch.randn(N, hp * wp, C * p * p, generator=gen).to(dtype).to(DEV).requires_grad_(True)
        g = torch.randn(N, H, W, C, generator=gen).to(dtype).to(DEV)
        before = ops.kernel_selections()["relayout_tiled"]
        img = ops.pixel_shuffle_tokens(tok, H, W, C, p)
        img.backward(g)
        torch.cuda.synchronize()
        assert ops.kernel_selections()["relayout_tiled"] - before == 2 * tiled, (p, dtype)
        assert torch.equal(_bits(img.detach().view(-1)), _bits(_relayout_definition(tok.detach().view(-1), N, H, W, C, p, True)))
        assert torch.equal(_bits(tok.grad.view(-1)), _bits(_relayout_definition(g.view(-1), N, H, W, C, p, False)))
    # the patch embedding of an image that divides into patches: image -> tokens forward, tokens -> image backward
    p, E = 8, 64
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(N, H, W, C, generator=gen).to(torch.bfloat16).to(DEV).requires_grad_(True)
    w = (torch.randn(E, C, p, p, generator=gen) / (C * p * p) ** 0.5).to(DEV).requires_grad_(True)
    b = torch.zeros(E, device=DEV, requires_grad=True)
    before = ops.kernel_selections()["relayout_tiled"]
    y = ops.patch_embed(x, w, b)
    y.float().square().sum().backward()
    torch.cuda.synchronize()
    assert ops.kernel_selections()["relayout_tiled"] - before == 2
    assert bool(torch.isfinite(x.grad.float()).all())


# ------------------------------------------------------------------------------------------------ combine_rows
def _ragged_plan(B, E, kcap, seed):
    """A plan with an expert without rows (the last), samples routed to kcap, to fewer, and to no expert."""
    from hdmoe_hip import ops
    gen = torch.Generator().manual_seed(seed)
    sparse = torch.zeros(B, E)
    for b in range(B):
        k = (0, 1, kcap, kcap)[b % 4] if b % 16 else 0
        sel = torch.randperm(E - 1, generator=gen)[:k]
        if k:
            sparse[b, sel] = torch.softmax(torch.randn(k, generator=gen), 0)
    plan = ops.DispatchPlan(sparse.to(DEV), kcap)
    torch.cuda.synchronize()
    assert int(plan.seg[E] - plan.seg[E - 1]) == 0 and bool((plan.perm < 0).any()) and bool((plan.inv < 0).any())
    return plan, sparse


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no_weights"])
@pytest.mark.parametrize("B,E,kcap,L,dtype", [
    (256, 4, 2, 32 * 32 * 32, torch.bfloat16),                 # bench: B = 256, 32 x 32 x 32 maps, top-2
    (64, 4, 2, 16 * 16 * 32, torch.float32),
    (33, 5, 3, 8 * 1000 + 8, torch.bfloat16),                  # a last chunk with a partial pass
    (7, 3, 1, 40, torch.bfloat16),                             # a row shorter than one pass of a workgroup
], ids=lambda v: str(v).replace("torch.", ""))
def test_combine_rows_vec_is_bit_identical(B, E, kcap, L, dtype, weighted):
    from hdmoe_hip._lib import call, dtype_code
    from hdmoe_hip import ops
    plan, _ = _ragged_plan(B, E, kcap, B + L)
    gen = torch.Generator().manual_seed(L)
    ys = torch.randn(plan.R, L, generator=gen).to(dtype).to(DEV)
    dout = torch.randn(B, L, generator=gen).to(dtype).to(DEV)
    row_w = plan.row_w if weighted else None
    dt = dtype_code(dtype)
    res = {}
    for tag, fwd, bwd in (("new", "hdmoe_combine_rows_fwd_vec", "hdmoe_combine_rows_bwd_vec"),
                          ("old", "hdmoe_combine_rows_fwd", "hdmoe_combine_rows_bwd")):
        before = ops.kernel_selections()
        obuf, out = _guarded(B * L, dtype, 555.0)
        dbuf, dys = _guarded(plan.R * L, dtype, 555.0)
        dsp = torch.zeros(B, E, dtype=torch.float32, device=DEV)
        assert call(fwd, out, ys, plan.inv, row_w, B, kcap, L, dt) == 0
        assert call(bwd, dys, dsp, dout, ys, plan.perm, plan.row_expert, row_w, plan.R, E, L, dt) == 0
        dbuf2, dys2 = _guarded(plan.R * L, dtype, 555.0)
        assert call(bwd, dys2, None, dout, ys, plan.perm, plan.row_expert, row_w, plan.R, E, L, dt) == 0   # no dsparse wanted
        torch.cuda.synchronize()
        after = ops.kernel_selections()
        n = 1 if tag == "new" else 0
        assert after["combine_fwd_vec"] - before["combine_fwd_vec"] == n and after["combine_bwd_vec"] - before["combine_bwd_vec"] == 2 * n
        assert _guards_ok(obuf, B * L, 555.0) and _guards_ok(dbuf, plan.R * L, 555.0) and _guards_ok(dbuf2, plan.R * L, 555.0)
        assert torch.equal(_bits(dys), _bits(dys2))
        res[tag] = (out, dys, dsp)
    assert torch.equal(_bits(res["new"][0]), _bits(res["old"][0])), "combine forward differs"
    assert torch.equal(_bits(res["new"][1]), _bits(res["old"][1])), "dys differs"
    # dsparse is bounded in test_dsparse_error_against_fp64; here: the same entries are non-zero
    assert torch.equal(res["new"][2] != 0, res["old"][2] != 0)


@pytest.mark.parametrize("L,dtype", [(100, torch.bfloat16), (30, torch.float32)], ids=lambda v: str(v).replace("torch.", ""))
def test_combine_rows_vec_declines_partial_vectors(L, dtype):
    from hdmoe_hip._lib import call, dtype_code
    from hdmoe_hip import ops
    B, E, kcap = 32, 4, 2
    plan, sparse = _ragged_plan(B, E, kcap, L)
    gen = torch.Generator().manual_seed(L)
    ys = torch.randn(plan.R, L, generator=gen).to(dtype).to(DEV)
    before = ops.kernel_selections()
    out = torch.full((B, L), 555.0, dtype=dtype, device=DEV)
    dys = torch.full((plan.R, L), 555.0, dtype=dtype, device=DEV)
    assert call("hdmoe_combine_rows_fwd_vec", out, ys, plan.inv, plan.row_w, B, kcap, L, dtype_code(dtype)) == 1
    assert call("hdmoe_combine_rows_bwd_vec", dys, None, out, ys, plan.perm, plan.row_expert, plan.row_w, plan.R, E, L, dtype_code(dtype)) == 1
    torch.cuda.synchronize()
    assert bool((out == 555.0).all()) and bool((dys == 555.0).all())
    # through autograd the scalar kernels take over
    ysg = ys.clone().requires_grad_(True)
    sp = sparse.to(DEV).requires_grad_(True)
    o = ops.combine_rows(ysg, sp * 1.0, plan)
    o.float().sum().backward()
    torch.cuda.synchronize()
    after = ops.kernel_selections()
    assert after["combine_fwd_vec"] == before["combine_fwd_vec"] and after["combine_bwd_vec"] == before["combine_bwd_vec"]
    ref = torch.zeros(B, L, dtype=torch.float64)
    perm, rw = plan.perm.cpu(), plan.row_w.cpu().double()
    for r in range(plan.R):
        if perm[r] >= 0:
            ref[perm[r]] += rw[r] * ys[r].cpu().double()
    assert float((o.detach().cpu().double() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())


def test_autograd_dispatch_takes_the_vec_combine():
    from hdmoe_hip import ops
    B, E, kcap, L = 64, 4, 2, 4096
    plan, sparse = _ragged_plan(B, E, kcap, 5)
    x = torch.randn(B, L).to(torch.bfloat16).to(DEV).requires_grad_(True)
    sp = sparse.to(DEV).requires_grad_(True)
    before = ops.kernel_selections()
    ys = ops.gather_rows(x, plan)
    out = ops.combine_rows(ys * 1.0, sp * 1.0, plan)
    out.float().sum().backward()
    torch.cuda.synchronize()
    after = ops.kernel_selections()
    assert after["combine_fwd_vec"] - before["combine_fwd_vec"] == 2          # combine forward + the gather's backward
    assert after["combine_bwd_vec"] - before["combine_bwd_vec"] == 1
    assert bool(torch.isfinite(sp.grad).all()) and bool(torch.isfinite(x.grad.float()).all())


def test_dsparse_error_against_fp64():
    from hdmoe_hip._lib import call, BF16
    B, E, kcap, L = 256, 4, 2, 32 * 32 * 32
    plan, _ = _ragged_plan(B, E, kcap, 11)
    gen = torch.Generator().manual_seed(12)
    ys = torch.randn(plan.R, L, generator=gen).to(torch.bfloat16)
    dout = torch.randn(B, L, generator=gen).to(torch.bfloat16)
    perm, rex = plan.perm.cpu(), plan.row_expert.cpu()
    ref = torch.zeros(B, E, dtype=torch.float64)
    mag = torch.zeros(B, E, dtype=torch.float64)
    for r in range(plan.R):
        if perm[r] >= 0:
            g, y = dout[perm[r]].double(), ys[r].double()
            ref[perm[r], rex[r]] = (g * y).sum()
            mag[perm[r], rex[r]] = (g.abs() * y.abs()).sum()
    routed = mag > 0
    ysd, doutd = ys.to(DEV), dout.to(DEV)
    dys = torch.empty_like(ysd)

    def run(name):
        dsp = torch.zeros(B, E, dtype=torch.float32, device=DEV)
        assert call(name, dys, dsp, doutd, ysd, plan.perm, plan.row_expert, plan.row_w, plan.R, E, L, BF16) == 0
        torch.cuda.synchronize()
        return dsp.cpu().double()

    def rel(d):
        return float(((d - ref).abs()[routed] / mag[routed]).max())

    old_a, old_b, new_a, new_b = run("hdmoe_combine_rows_bwd"), run("hdmoe_combine_rows_bwd"), run("hdmoe_combine_rows_bwd_vec"), run("hdmoe_combine_rows_bwd_vec")
    fig = {"old_run_to_run_spread": float(((old_a - old_b).abs()[routed] / mag[routed]).max()),
           "new_run_to_run_spread": float(((new_a - new_b).abs()[routed] / mag[routed]).max()),
           "old_err_vs_fp64": max(rel(old_a), rel(old_b)), "new_err_vs_fp64": max(rel(new_a), rel(new_b))}
    _measured["dsparse"] = fig
    print("\ndsparse (relative to sum |dout||ys|): " + json.dumps(fig, sort_keys=True))
    assert bool((new_a[~routed] == 0).all()) and bool((old_a[~routed] == 0).all())
    assert fig["new_err_vs_fp64"] <= 2.0 * fig["old_err_vs_fp64"], fig
