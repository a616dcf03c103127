"""EDM_Sampler.sample(tile=...): tiled sampling of latents larger than the model's resolution.

Mock denoiser (it depends on where a tile sits and on which text row it got): the trajectory of every solver and conditioning against a
float64 restatement of solver plus tiling, eager against hipGraph replay bit for bit, chunked model calls (tile_batch), one capture for
several prompts, and tile == latent size against the untiled sampler.  Real model (config-2 golden weights): the same identities, and one
tiled evaluation against the float64 blend of sampler.denoise on the torch-sliced tile batch."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils"))

from EDM_sampler import EDM_Sampler  # noqa: E402
from hdmoe_hip import ops  # noqa: E402

DEV = "cuda"
pytestmark = pytest.mark.gpu
TP, SOFT = -1.2, 1.6
N, B, C, H, W, TILE, OV = 4, 2, 4, 24, 38, (16, 16), 8          # 2 x 4 tiles, the last x tile clamped: three covers on x
GAMMA_MAX = math.sqrt(2) - 1


class _MockDenoiser(torch.nn.Module):
    """den = scale x + P + 0.3 mean(text row), P a fixed (C, h, w) pattern: the output depends on the position inside the tile and on the
    text row, so a wrong origin, row order or row repeat shows.  Asserts the tile-batch shape it is given and records the batch sizes."""

    def __init__(self, scale, seed, num_experts=4, hw=TILE):
        super().__init__()
        self.num_experts, self.scale, self.expect, self.batches, self.unet_mask = num_experts, scale, None, [], None
        self.register_buffer("P", torch.randn(C, *hw, generator=torch.Generator().manual_seed(seed)))

    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, transition_point, softness, return_log_var=False):
        assert sigma.ndim == 0 and zeta == 0 and tuple(x.shape[1:]) == tuple(self.P.shape)
        assert self.expect is None or x.shape[0] == self.expect, (x.shape, self.expect)
        assert Unet_router_mask.shape == (x.shape[0], self.num_experts) and text_emb.shape[0] == x.shape[0]
        self.batches.append(x.shape[0])
        self.unet_mask = Unet_router_mask                  # of the last call
        # the row mean in float64, rounded once: the same bits whatever the batch size (a chunked call must reproduce the whole one)
        mean = text_emb.double().mean(dim=(1, 2)).float().view(-1, 1, 1, 1)
        return {"denoised": x * self.scale + self.P + 0.3 * mean}


def close_scaled(a, b, rel, msg="", atol=1e-6):
    """max|a-b| <= rel * max|b| + atol (the sampler tests' tolerance form)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{msg}: non-finite output"
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print(f"{msg}: max err {err:.3e}, bound {rel * scale + atol:.3e}")
    assert err <= rel * scale + atol, f"{msg}: max err {err:.3e} > {rel:.1e} * {scale:.3e} + {atol:.0e}"


def _known_exact(out, x0, mask, msg):
    keep = mask.expand_as(out) == 1
    assert bool(keep.any()) and bool((~keep).any())
    assert torch.equal(out[keep], x0[keep]), f"{msg}: known region is not init_latents bit-for-bit"


def schedule(n, sigma_min=0.002, sigma_max=80.0, rho=7):
    i = torch.arange(n, dtype=torch.float64)
    t = (sigma_max ** (1 / rho) + i / (n - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros(1, dtype=torch.float64)])


# ---- float64 restatement: tiling, then the solvers on the large latent
def slices(x, plan):
    return torch.stack([x[b, :, oy:oy + plan.h, ox:ox + plan.w] for b in range(x.shape[0]) for oy in plan.oy.tolist()
                        for ox in plan.ox.tolist()])


def blend64(tiles, plan, nb):
    """sum over the tiles of (ny[ky, y] nx[kx, x]) tile value, on the plan's own fp32 tables in float64."""
    ny, nx = torch.from_numpy(plan.ny).double(), torch.from_numpy(plan.nx).double()
    out = torch.zeros(nb, tiles.shape[1], plan.H, plan.W, dtype=torch.float64)
    for b in range(nb):
        for ky, oy in enumerate(plan.oy.tolist()):
            for kx, ox in enumerate(plan.ox.tolist()):
                wgt = ny[ky, oy:oy + plan.h, None] * nx[kx, None, ox:ox + plan.w]
                out[b, :, oy:oy + plan.h, ox:ox + plan.w] += wgt * tiles[(b * plan.Ty + ky) * plan.Tx + kx].double().cpu()
    return out


def tiled_den64(plan, model, gnet, text, unc, guide, interval):
    """den(x_big, sigma) in float64: every tile row through the mocks' formula with ITS sample's text, guided per sample inside the
    interval, blended."""
    T = plan.T
    mean = lambda tx: tx.double().cpu().mean(dim=(1, 2)).repeat_interleave(T).view(-1, 1, 1, 1)          # noqa: E731
    mt, mu = mean(text), mean(unc)
    active = torch.is_tensor(guide) or guide != 1.0
    g = guide.double().cpu().repeat_interleave(T).view(-1, 1, 1, 1) if torch.is_tensor(guide) else float(guide)
    one = lambda m, tl, mn: m.scale * tl + m.P.double().cpu() + 0.3 * mn                                  # noqa: E731

    def den(x, sigma):
        tl = slices(x, plan)
        d = one(model, tl, mt)
        if active and (interval is None or interval[0] <= float(sigma) <= interval[1]):
            d = (1.0 - g) * one(gnet, tl, mu) + g * d
        return blend64(d, plan, x.shape[0])
    return den


def restate(den, noise, solver="heun", strength=1.0, x0=None, m=None, seed=None, s_churn=0.0, s_min=0.0, s_max=float("inf"), s_noise=1.0,
            eta=1.0):
    """float64 restatement of sample() on the large latent (its docstring's rules); eps of stage i = ops.randn_keyed(noise, seed, i)."""
    t = schedule(N)
    i0 = N - math.ceil(strength * N)
    eps = lambda i: ops.randn_keyed(noise, seed, i).double().cpu()                                        # noqa: E731
    nz = noise.double().cpu()
    x0 = None if x0 is None else x0.double().cpu()
    m = None if m is None else m.double().cpu()
    blend = lambda x, s: x if m is None else m * (x0 + s * nz) + (1 - m) * x                              # noqa: E731
    x = t[i0] * nz if x0 is None else x0 + t[i0] * nz
    dp = None
    for i in range(i0, N):
        tc, tn = t[i], t[i + 1]
        if solver == "heun":
            gamma = min(s_churn / N, GAMMA_MAX) if s_churn > 0 and s_min <= float(tc) <= s_max else 0.0
            th = tc + gamma * tc
            xh = x + torch.sqrt(th * th - tc * tc) * s_noise * eps(i) if gamma > 0 else x
            d = den(xh, th)
            h = tn - th
            xn = blend(xh + h * (xh - d) / th, tn)
            x = xn if i == N - 1 else blend(xh + h * (0.5 * (xh - d) / th + 0.5 * (xn - den(xn, tn)) / tn), tn)
            continue
        d = den(x, tc)
        sde = solver == "dpmpp_2m_sde"
        e = torch.exp(-eta * torch.log(tc / tn)) if sde and tn > 0 else torch.tensor(1.0, dtype=torch.float64)
        a = tn / tc * e
        if tn == 0:
            xn = d.clone()
        elif i == i0:
            xn = a * x + (1 - a) * d
        else:
            r = torch.log(t[i - 1] / tc) / torch.log(tc / tn)
            xn = a * x + (1 - a) * ((1 + 1 / (2 * r)) * d - (1 / (2 * r)) * dp)
        if sde and eta > 0 and tn > 0:
            xn = xn + tn * torch.sqrt(1 - e * e) * s_noise * eps(i)
        x, dp = blend(xn, tn), d
    return x


@pytest.fixture(scope="module")
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    hdmoe_hip.set_compute_dtype(torch.float32)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


@pytest.fixture(scope="module")
def mock(_gpu):
    gen = torch.Generator(device=DEV).manual_seed(21)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)                                           # noqa: E731
    mask = torch.zeros(B, 1, H, W, device=DEV)
    mask[0, :, :, :19] = 1.0                               # across tile seams
    mask[1, :, 5:20, 9:30] = 1.0
    return dict(noise=rnd(B, C, H, W), x0=rnd(B, C, H, W), text=rnd(B, 5, 16), unc=rnd(B, 5, 16), text2=rnd(B, 5, 16), unc2=rnd(B, 5, 16),
                noise2=rnd(B, C, H, W), mask=mask, model=_MockDenoiser(0.9, 1).to(DEV), gnet=_MockDenoiser(0.5, 2).to(DEV),
                plan=ops.tile_plan(H, W, *TILE, OV, "feather"))


TILE_KW = dict(tile=TILE, tile_overlap=OV)
UM = torch.tensor([[1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 0.0]])          # one router mask row per sample
SEED = 12345
# name -> (constructor keywords, sample keywords, restatement keywords, per-sample guidance vector or None)
CASES = {
    "heun": (dict(), dict(), dict(), None),
    "dpmpp_2m": (dict(solver="dpmpp_2m"), dict(), dict(solver="dpmpp_2m"), None),
    "dpmpp_2m_sde": (dict(solver="dpmpp_2m_sde", eta=0.5, S_noise=1.0 + 2.0 ** -7), dict(seed=SEED),
                     dict(solver="dpmpp_2m_sde", eta=0.5, s_noise=1.0 + 2.0 ** -7, seed=SEED), None),
    "churn_on_device": (dict(S_churn=3.0, S_min=0.05, S_max=50.0, S_noise=1.007, churn_on_device=True), dict(seed=SEED),
                        dict(s_churn=3.0, s_min=0.05, s_max=50.0, s_noise=1.007, seed=SEED), None),
    "guidance_two_pass": (dict(guidance=2.0), dict(), dict(), None),
    "guidance_vector": (dict(), dict(um=True), dict(), [2.5, -0.5]),
    "guidance_interval": (dict(guidance=2.0, guidance_interval=(0.5, 10.0)), dict(), dict(), None),
    "strength": (dict(guidance=2.0), dict(strength=0.5, init=True), dict(strength=0.5), None),
    "inpaint": (dict(guidance=2.0, solver="dpmpp_2m"), dict(init=True, mask=True), dict(solver="dpmpp_2m"), None),
    "uniform_window": (dict(guidance=2.0), dict(tile_window="uniform"), dict(), None),
}


def _run(mock, case, use_graph, text="text", unc="unc", noise="noise", sampler=None, **tile_kw):
    ckw, skw, _, gvec = CASES[case]
    skw = dict(skw)
    if skw.pop("init", False):
        skw["init_latents"] = mock["x0"]
    if skw.pop("mask", False):
        skw["inpaint_mask"] = mock["mask"]
    if skw.pop("um", False):
        skw["Unet_router_mask"] = UM
    if gvec is not None:
        skw["guidance"] = torch.tensor(gvec)
    s = sampler or EDM_Sampler(mock["model"], mock["gnet"], num_solve_steps=N, use_graph=use_graph, **ckw)
    return s, s.sample(mock[noise], mock[text], TP, SOFT, mock[unc], **dict(TILE_KW, **tile_kw), **skw)


def _reference(mock, case, text="text", unc="unc", noise="noise"):
    ckw, skw, rkw, gvec = CASES[case]
    plan = ops.tile_plan(H, W, *TILE, OV, skw.get("tile_window", "feather"))
    guide = torch.tensor(gvec) if gvec is not None else ckw.get("guidance", 1.0)
    den = tiled_den64(plan, mock["model"], mock["gnet"], mock[text], mock[unc], guide, ckw.get("guidance_interval"))
    return restate(den, mock[noise], x0=mock["x0"] if skw.get("init") else None, m=mock["mask"] if skw.get("mask") else None, **rkw)


@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_matches_restatement_and_replay(mock, case):
    mock["model"].expect = mock["gnet"].expect = B * mock["plan"].T
    mock["model"].batches.clear()
    eager_s, eager = _run(mock, case, False)
    calls = list(mock["model"].batches)
    graph_s, graphed = _run(mock, case, True)
    assert eager.shape == (B, C, H, W) and (eager_s.fused_heun or eager_s.fused_dpm) and graph_s._stage is not None
    n_run = math.ceil(CASES[case][1].get("strength", 1.0) * N)
    assert calls == [B * mock["plan"].T] * (n_run if CASES[case][0].get("solver") else 2 * n_run - 1)
    close_scaled(eager, _reference(mock, case).float(), 1e-4, msg=f"{case}: tiled trajectory vs the float64 restatement")
    assert torch.equal(graphed, eager), f"{case}: replay differs from eager, max {float((graphed - eager).abs().max()):.3e}"
    if CASES[case][1].get("mask"):
        _known_exact(eager, mock["x0"], mock["mask"], "eager")
        _known_exact(graphed, mock["x0"], mock["mask"], "replay")
    if CASES[case][1].get("um"):                          # the router mask reached the model once per tile row of its sample
        assert torch.equal(mock["model"].unet_mask.cpu(), UM.repeat_interleave(mock["plan"].T, 0))
    if case == "guidance_interval":
        assert 0 < eager_s.last_evaluations["guided"] and 0 < eager_s.last_evaluations["plain"]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", ["guidance_two_pass", "guidance_vector", "dpmpp_2m_sde"])
def test_tile_batch_chunks_are_bit_identical(mock, case, use_graph):
    """tile_batch = B T / 2: two model calls per network and evaluation, each on its own rows of the text, the masks and the scales."""
    n = B * mock["plan"].T
    mock["model"].expect = mock["gnet"].expect = n
    _, full = _run(mock, case, use_graph)
    for m in (mock["model"], mock["gnet"]):
        m.expect = n // 2
        m.batches.clear()
    s, half = _run(mock, case, use_graph, tile_batch=n // 2)
    assert torch.equal(half, full)
    if not use_graph:                                      # replays do not call the modules
        evals = N if CASES[case][0].get("solver") else 2 * N - 1
        assert mock["model"].batches == [n // 2] * (2 * evals)
    else:
        assert s._stage["tile"]["buf"].shape == (n, C, *TILE) and s._stage["tile"]["xt"].shape == (n // 2, C, *TILE)
    with pytest.raises(ValueError, match="tile_batch"):
        _run(mock, case, use_graph, tile_batch=n // 2 + 1)


@pytest.mark.parametrize("case", ["guidance_two_pass", "inpaint"])
def test_one_capture_serves_other_prompts_and_inits(mock, case):
    mock["model"].expect = mock["gnet"].expect = B * mock["plan"].T
    s, first = _run(mock, case, True)
    stage, key = s._stage, s._stage["key"]
    graphs = list(stage["g_heun" if s.fused_heun else "g_dpm"])
    assert any(isinstance(k, tuple) and k and k[0] == "tile" for k in key)
    _, again = _run(mock, case, True, text="text2", unc="unc2", noise="noise2", sampler=s)
    assert s._stage is stage and s._stage["key"] == key and list(stage["g_heun" if s.fused_heun else "g_dpm"]) == graphs
    assert torch.equal(first, _run(mock, case, False)[1])
    assert torch.equal(again, _run(mock, case, False, text="text2", unc="unc2", noise="noise2")[1])
    close_scaled(again, _reference(mock, case, "text2", "unc2", "noise2").float(), 1e-4, msg=f"{case}: second prompt through the same capture")
    assert float((again - first).abs().max()) > 1e-2
    mock["model"].expect = mock["gnet"].expect = None
    _run(mock, case, True, sampler=s, tile_overlap=4)     # another tile spec is another capture
    assert s._stage is not stage


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp_2m"])
def test_tile_of_the_latent_size_is_the_untiled_sampler(_gpu, solver, use_graph):
    gen = torch.Generator(device=DEV).manual_seed(5)
    noise, text, unc = torch.randn(3, C, 16, 16, device=DEV, generator=gen), torch.randn(3, 5, 16, device=DEV, generator=gen), \
        torch.randn(3, 5, 16, device=DEV, generator=gen)
    model, gnet = _MockDenoiser(0.9, 1).to(DEV), _MockDenoiser(0.5, 2).to(DEV)
    mk = lambda: EDM_Sampler(model, gnet, num_solve_steps=N, guidance=2.0, solver=solver, use_graph=use_graph)      # noqa: E731
    plain_s = mk()
    plain = plain_s.sample(noise, text, TP, SOFT, unc)
    assert all(not (isinstance(k, tuple) and k and k[0] == "tile") for k in plain_s._stage["key"]) and plain_s._stage["tile"] is None
    assert torch.equal(mk().sample(noise, text, TP, SOFT, unc, tile=(16, 16), tile_overlap=8), plain)
    assert torch.equal(mk().sample(noise, text, TP, SOFT, unc, tile=(16, 16), tile_window="uniform", tile_batch=1), plain)


def test_host_loops_and_bf16(mock):
    """S_churn without churn_on_device and non-fp32 latents take the host loops: the eager branch of _eval and its captured evaluation."""
    mock["model"].expect = mock["gnet"].expect = None
    kw = dict(S_churn=3.0, S_min=0.05, S_max=50.0, S_noise=1.007)
    outs = []
    for use_graph in (False, True):
        s = EDM_Sampler(mock["model"], mock["gnet"], num_solve_steps=N, guidance=2.0, use_graph=use_graph, **kw)
        outs.append(s.sample(mock["noise"], mock["text"], TP, SOFT, mock["unc"], seed=SEED, **TILE_KW))
        assert not s.fused_heun and (s._graph is not None) == use_graph
    den = tiled_den64(mock["plan"], mock["model"], mock["gnet"], mock["text"], mock["unc"], 2.0, None)
    ref = restate(den, mock["noise"], seed=SEED, s_churn=3.0, s_min=0.05, s_max=50.0, s_noise=1.007)
    close_scaled(outs[0], ref.float(), 1e-4, msg="host loop with churn, tiled")
    assert torch.equal(outs[0], outs[1])
    s = EDM_Sampler(mock["model"], mock["gnet"], num_solve_steps=N, guidance=2.0, dtype=torch.bfloat16)
    out = s.sample(mock["noise"], mock["text"], TP, SOFT, mock["unc"], init_latents=mock["x0"], inpaint_mask=mock["mask"], **TILE_KW)
    assert out.dtype == torch.bfloat16 and out.shape == (B, C, H, W) and torch.isfinite(out).all() and not s.fused_heun
    _known_exact(out, mock["x0"].to(torch.bfloat16), mock["mask"], "bf16 host loop, tiled")


# ---- real model (config-2 golden weights)
@pytest.fixture(scope="module")
def real_model(_gpu):
    from models import model_config2
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    model = model_config2.preconditioned_HDMOEM(**g["cfg"])
    model.load_state_dict(g["state"])
    model = model.to(DEV).eval()
    R = g["cfg"]["IN_img_resolution"]
    gen = torch.Generator(device=DEV).manual_seed(0)
    EDM_Sampler(model, model, num_solve_steps=2).sample(torch.randn(2, 4, R, R, device=DEV, generator=gen), g["text"][:2].to(DEV), TP, SOFT)
    return model, g, R


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_real_model_tile_of_its_own_size(real_model, use_graph):
    model, g, R = real_model
    gen = torch.Generator(device=DEV).manual_seed(31)
    noise = torch.randn(2, 4, R, R, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    unc = torch.randn(text.shape, device=DEV, generator=gen)
    mk = lambda: EDM_Sampler(model, model, num_solve_steps=3, guidance=2.0, use_graph=use_graph)          # noqa: E731
    plain = mk().sample(noise, text, TP, SOFT, unc)
    tiled = mk().sample(noise, text, TP, SOFT, unc, tile=(R, R), tile_overlap=R // 2)
    assert torch.isfinite(plain).all()
    assert torch.equal(tiled, plain), f"max diff {float((tiled - plain).abs().max()):.3e}"


def _wide_inputs(g, R, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    noise = torch.randn(2, 4, R, R + R // 2, device=DEV, generator=gen)
    text = g["text"][:2].to(DEV)
    return noise, text, torch.randn(text.shape, device=DEV, generator=gen)


@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
def test_real_model_wide_latent_eager_vs_graph(real_model, shared):
    """R x (R + R/2) latents, overlap R/2: T = 2, and tile_batch = 2 makes two model calls of two rows per evaluation."""
    model, g, R = real_model
    noise, text, unc = _wide_inputs(g, R, 32)
    kw = dict(tile=(R, R), tile_overlap=R // 2, tile_batch=2)
    mk = lambda **o: EDM_Sampler(model, model, num_solve_steps=3, guidance=2.0, shared_guidance=shared, **o)          # noqa: E731
    eager_s, graph_s = mk(), mk(use_graph=True)
    eager = eager_s.sample(noise, text, TP, SOFT, unc, **kw)
    graphed = graph_s.sample(noise, text, TP, SOFT, unc, **kw)
    assert eager.shape == noise.shape and torch.isfinite(eager).all() and graph_s.fused_heun
    assert graph_s._stage["tile"]["plan"].T == 2 and graph_s._stage["text"].shape[0] == 4
    assert torch.equal(graphed, eager), f"max diff {float((graphed - eager).abs().max()):.3e}"
    plain = EDM_Sampler(model, model, num_solve_steps=3, guidance=1.0).sample(noise, text, TP, SOFT, unc, **kw)
    assert float((plain - eager).abs().max()) > 1e-4       # the guidance is in effect


@pytest.mark.parametrize("shared", [False, True], ids=["two_pass", "shared"])
def test_real_model_one_tiled_evaluation(real_model, shared):
    """One tiled evaluation, through the captured "eval" state and eagerly, against the float64 blend of sampler.denoise on the
    torch-sliced tile batch in the same chunking: within (max_cover_y max_cover_x + 2) 2^-24 max|tiles|, the blend kernel's bound."""
    model, g, R = real_model
    noise, text, unc = _wide_inputs(g, R, 33)
    x = 1.3 * noise
    sig = torch.tensor(1.3, device=DEV)
    with torch.no_grad():
        s = EDM_Sampler(model, model, num_solve_steps=3, guidance=2.0, shared_guidance=shared, use_graph=True)
        inp, tile = s._inputs(x, text, TP, SOFT, unc, ((R, R), R // 2, "feather", 2))
        plan = tile["plan"]
        text_r, unc_r = text.repeat_interleave(plan.T, 0), unc.repeat_interleave(plan.T, 0)
        sl = slices(x, plan)
        tiles = torch.cat([s.denoise(sl[r:r + 2].contiguous(), sig, text_r[r:r + 2], TP, SOFT, unc_r[r:r + 2]) for r in range(0, 4, 2)])
        ref = blend64(tiles, plan, 2)
        assert torch.equal(inp.text, text_r) and torch.equal(inp.unc, unc_r)
        eager = s._denoise_tiled(s._tile_bufs(tile, x), x, sig, inp, True)
        st = s._stage_state("eval", x, inp, tile)
        st["sig"].fill_(1.3)
        st["g_eval"][0].replay()
        replayed = st["out"].clone()
    bound = (plan.max_cover_y * plan.max_cover_x + 2) * 2.0 ** -24 * float(tiles.abs().max())
    for name, out in (("eager", eager), ("replay", replayed)):
        err = float((out.double().cpu() - ref).abs().max())
        print(f"{name} shared={shared}: max err {err:.3e}, bound {bound:.3e}")
        assert out.shape == x.shape and err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
