"""hdmoe_tile_gather / hdmoe_tile_blend (csrc/tiles.hip) on the GPU: gather bit for bit against slicing (whole batch and a chunk), blend
against a float64 restatement on the plan's own fp32 tables, single-cover pixels bit for bit, placement, determinism, graph capture and
guard elements -- on the 16-byte arm, the scalar arm (odd sizes, three covers on x) and T = 1."""
import pytest
import torch

from hdmoe_hip import ops

DEV = "cuda"
pytestmark = pytest.mark.gpu

# (B, C, H, W, h, w, overlap)
SHAPES = {"vec_24x40": (2, 4, 24, 40, 16, 16, 8), "scalar_24x38": (2, 4, 24, 38, 16, 16, 8), "odd_9x17": (1, 3, 9, 17, 6, 10, (2, 3)),
          "one_tile": (2, 4, 16, 16, 16, 16, 0)}
WINDOWS = ["feather", "uniform"]


@pytest.fixture(scope="module")
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()


def _case(name, window="feather", seed=0):
    B, C, H, W, h, w, ov = SHAPES[name]
    plan = ops.tile_plan(H, W, h, w, ov, window)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, C, H, W, device=DEV, generator=gen)
    tiles = torch.randn(B * plan.T, C, h, w, device=DEV, generator=gen)
    return plan, x, tiles


def _slices(x, plan):
    """The tile batch by slicing, sample-major: r = (b Ty + ky) Tx + kx."""
    return torch.stack([x[b, :, oy:oy + plan.h, ox:ox + plan.w] for b in range(x.shape[0]) for oy in plan.oy.tolist()
                        for ox in plan.ox.tolist()])


def _cover(plan):
    """(H, W) int tensor: how many tiles lie over each position."""
    ny, nx = torch.from_numpy(plan.ny), torch.from_numpy(plan.nx)
    return ((ny > 0).sum(0)[:, None] * (nx > 0).sum(0)[None, :]).to(DEV)


def _blend64(tiles, plan, B):
    """float64 restatement of the blend on the plan's own fp32 tables; also the value of the last covering tile per pixel."""
    t64 = tiles.double().cpu()
    C = t64.shape[1]
    ny, nx = torch.from_numpy(plan.ny).double(), torch.from_numpy(plan.nx).double()
    out = torch.zeros(B, C, plan.H, plan.W, dtype=torch.float64)
    for b in range(B):
        for ky, oy in enumerate(plan.oy.tolist()):
            for kx, ox in enumerate(plan.ox.tolist()):
                wgt = ny[ky, oy:oy + plan.h, None] * nx[kx, None, ox:ox + plan.w]
                out[b, :, oy:oy + plan.h, ox:ox + plan.w] += wgt * t64[(b * plan.Ty + ky) * plan.Tx + kx]
    return out


def _last_tile_value(tiles, plan, B):
    """(B, C, H, W): the value of the last tile over each pixel, in tile-batch order -- on single-cover pixels, of the only one."""
    out = torch.empty(B, tiles.shape[1], plan.H, plan.W, device=tiles.device)
    for b in range(B):
        for ky, oy in enumerate(plan.oy.tolist()):
            for kx, ox in enumerate(plan.ox.tolist()):
                out[b, :, oy:oy + plan.h, ox:ox + plan.w] = tiles[(b * plan.Ty + ky) * plan.Tx + kx]
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_gather_is_slicing(_gpu, name):
    plan, x, _ = _case(name)
    ref = _slices(x, plan)
    n = ref.shape[0]
    assert torch.equal(ops.tile_gather(x, plan), ref)
    if n > 2:                                              # a chunk: row0 > 0, rows < B T, across a sample boundary where B > 1
        r0, rows = n // 2 - 1, 3
        assert torch.equal(ops.tile_gather(x, plan, r0, rows), ref[r0:r0 + rows])
        assert torch.equal(ops.tile_gather(x, plan, n - 1), ref[n - 1:])
    for r0 in range(n):                                    # every row on its own
        assert torch.equal(ops.tile_gather(x, plan, r0, 1), ref[r0:r0 + 1]), r0


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_blend_matches_fp64(_gpu, name, window):
    """|out - ref| <= (max_cover_y max_cover_x + 2) 2^-24 max|tiles|: one rounding of the weight product and one per fma, each at most
    half an ulp of a partial sum bounded by max|tiles| (the weights sum to 1 within the slack), plus the slack for that sum."""
    plan, _, tiles = _case(name, window, seed=1)
    B = SHAPES[name][0]
    out = ops.tile_blend(tiles, plan, B)
    ref = _blend64(tiles, plan, B)
    err = float((out.double().cpu() - ref).abs().max())
    bound = (plan.max_cover_y * plan.max_cover_x + 2) * 2.0 ** -24 * float(tiles.abs().max())
    print(f"{name} {window}: T = {plan.Ty}x{plan.Tx}, cover {plan.max_cover_y}x{plan.max_cover_x}, max err {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out).all() and err <= bound
    single = (_cover(plan) == 1).expand_as(out)
    assert bool(single.any())
    assert torch.equal(out[single], _last_tile_value(tiles, plan, B)[single]), "single-cover pixels are the tile's value bit for bit"
    if plan.T == 1:
        assert bool(single.all()) and torch.equal(out, tiles)


def test_blend_keeps_the_sign_of_zero(_gpu):
    plan, _, tiles = _case("one_tile")
    tiles[0, 0, 0, :4] = -0.0
    out = ops.tile_blend(tiles, plan, 2)
    assert torch.equal(out.view(torch.int32), tiles.view(torch.int32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_placement(_gpu, name):
    """Every tile holds its own row index: a pixel under one tile must hold exactly that index (row order, origins)."""
    plan, x, tiles = _case(name)
    B, n = SHAPES[name][0], tiles.shape[0]
    tiles = torch.arange(n, device=DEV, dtype=torch.float32).view(n, 1, 1, 1).expand_as(tiles).contiguous()
    out = ops.tile_blend(tiles, plan, B)
    single = (_cover(plan) == 1).expand_as(out)
    assert torch.equal(out[single], _last_tile_value(tiles, plan, B)[single])
    lo, hi = out.amin(dim=(1, 2, 3)).cpu(), out.amax(dim=(1, 2, 3)).cpu()                # a blend stays inside its sample's rows
    for b in range(B):
        assert b * plan.T - 1e-3 <= float(lo[b]) and float(hi[b]) <= (b + 1) * plan.T - 1 + 1e-3
    # and the round trip: gathering the coordinate image and blending it returns it (every tile agrees on every pixel)
    back = ops.tile_blend(ops.tile_gather(x, plan), plan, B)
    assert float((back - x).abs().max()) <= (plan.max_cover + 2) * 2.0 ** -24 * float(x.abs().max())


@pytest.mark.parametrize("name", ["vec_24x40", "scalar_24x38"])
def test_deterministic_and_captured(_gpu, name):
    plan, x, tiles = _case(name, seed=2)
    B = SHAPES[name][0]
    g1, b1 = ops.tile_gather(x, plan), ops.tile_blend(tiles, plan, B)
    g2, b2 = ops.tile_gather(x, plan), ops.tile_blend(tiles, plan, B)
    assert torch.equal(g1, g2) and torch.equal(b1, b2)
    sx, st, so = x.clone(), torch.empty_like(tiles), torch.empty_like(x)
    plan.device(DEV)

    def run():
        ops.tile_gather(sx, plan, out=st)
        ops.tile_blend(st, plan, B, out=so)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    eager = ops.tile_blend(ops.tile_gather(x, plan), plan, B)
    graph.replay()
    assert torch.equal(so, eager) and torch.equal(st, g1)
    x2 = torch.randn_like(x)
    sx.copy_(x2)
    graph.replay()
    assert torch.equal(so, ops.tile_blend(ops.tile_gather(x2, plan), plan, B))


@pytest.mark.parametrize("pad", [4, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_guard_elements(_gpu, name, pad):
    """Sentinels on both sides of tiles and out stay untouched, whole batch and chunk (pad 3 also takes the 16-byte arm's alignment away)."""
    plan, x, tiles = _case(name, seed=3)
    B, C = SHAPES[name][:2]
    SENT = 12345.0

    def padded(shape):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * pad,), SENT, device=DEV)
        return buf, buf[pad:pad + n].view(shape)

    def intact(buf, n, msg):
        assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all()), msg

    rows = max(1, tiles.shape[0] // 2)
    gbuf, gout = padded((rows, C, plan.h, plan.w))
    ops.call("hdmoe_tile_gather", gout, x, *plan.device(DEV)[:2], B, C, plan.H, plan.W, plan.h, plan.w, plan.Ty, plan.Tx, tiles.shape[0] - rows, rows)
    intact(gbuf, gout.numel(), "gather")
    assert torch.equal(gout, _slices(x, plan)[tiles.shape[0] - rows:])
    tbuf, tin = padded(tuple(tiles.shape))
    tin.copy_(tiles)
    obuf, out = padded((B, C, plan.H, plan.W))
    ops.call("hdmoe_tile_blend", out, tin, *plan.device(DEV), B, C, plan.H, plan.W, plan.h, plan.w, plan.Ty, plan.Tx)
    intact(obuf, out.numel(), "blend out")
    intact(tbuf, tin.numel(), "blend tiles")
    assert torch.equal(out, ops.tile_blend(tiles, plan, B)), "both arms give the same bits"


def test_wrappers_refuse(_gpu):
    plan, x, tiles = _case("vec_24x40")
    for bad in (dict(row0=-1), dict(row0=16), dict(rows=0), dict(row0=10, rows=7)):
        with pytest.raises(ValueError, match="tile_gather"):
            ops.tile_gather(x, plan, **bad)
    for t in (x[:, :, :16], x.double(), x.cpu(), x.permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match="tile_gather"):
            ops.tile_gather(t, plan)
    with pytest.raises(ValueError, match="tile_gather"):
        ops.tile_gather(x, plan, out=torch.empty(3, 4, 16, 16, device=DEV))
    for t, B in ((tiles[:15], 2), (tiles, 1), (tiles.double(), 2), (tiles[:, :, :8], 2)):
        with pytest.raises(ValueError, match="tile_blend"):
            ops.tile_blend(t, plan, B)
