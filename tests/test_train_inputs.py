"""The fused training-input generator (csrc/traingen.hip, ops.train_inputs, Utils.utils.DeviceInputs) and the device-scalar scale of the
logit-noise kernel (hdmoe_randn_ds): RNG contract against ops.randn_keyed, the sigma mixture against its exact CDF, the shuffle, the masks
against the torch MaskGenerator on the generator's own sigma, determinism, the error paths."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234ABCD5678EF01
SMIN, SMAX = 0.002, 80.0
ATTRS = {3: [3, 5, 7], 4: [3, 3, 5, 5], 8: [4, 4, 8, 8, 8, 16, 16, 16], 9: list(range(9))}


def _mask_gens(E, min_active, p_mean, p_std, ubw, vbw):
    from Utils.utils import MaskGenerator
    mk = lambda bw, rng: MaskGenerator(expert_attributes=ATTRS[E], p_mean=p_mean, p_std=p_std, bandwidth=bw, max_bandwidth=bw,
                                       min_active=min_active, total_steps=10, noise_range=rng)
    return mk(ubw, (0.0, 0.6)), mk(vbw, (0.4, 1.0))


def _buffers(B, chw, E):
    f = dict(dtype=torch.float32, device=DEV)
    return {"x": torch.full((B,) + tuple(chw), -7.0, **f), "sigma": torch.full((B, 1, 1, 1), -7.0, **f), "unet_mask": torch.full((B, E), -7.0, **f),
            "vit_mask": torch.full((B, E), -7.0, **f), "zeta": torch.full((1,), -7.0, **f), "src": torch.full((B,), -7, dtype=torch.int32, device=DEV)}


def _x0(B, chw, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return 0.5 * torch.randn((B,) + tuple(chw), device=DEV, generator=g)


def _generate(B, chw, E, min_active, ep, step, p_mean=-0.4, p_std=1.0, ubw=0.3, vbw=0.3, seed=SEED, zeta=0.25, x0=None, buf=None):
    from hdmoe_hip import ops
    ug, vg = _mask_gens(E, min_active, p_mean, p_std, ubw, vbw)
    x0 = _x0(B, chw) if x0 is None else x0
    b = _buffers(B, chw, E) if buf is None else buf
    ops.train_inputs(b["x"], b["sigma"], b["unet_mask"], b["vit_mask"], b["zeta"], b["src"], x0, ug.expert_centers.to(DEV), vg.expert_centers.to(DEV),
                     seed, step, sigma_min=SMIN, sigma_max=SMAX, p_mean=p_mean, p_std=p_std, extreme_prob=ep, unet_bw=ubw, vit_bw=vbw,
                     min_active=min_active, zeta=zeta)
    return b, x0, ug, vg


# every value of B, (C,H,W), E, min_active, extreme_prob and bandwidth the generator is specified for appears at least once; B = 4096 is the
# LDS limit, (3,3,3) the scalar path (27 % 4 != 0), 250 a batch that is no multiple of 4
CASES = [(1, (4, 16, 16), 4, 1, 0.5, 0.05, 0.3), (1, (3, 3, 3), 3, 2, 1.0, 0.36, 0.9), (6, (3, 3, 3), 3, 2, 0.0, 0.3, 0.36),
         (6, (4, 16, 16), 8, 1, 0.5, 0.9, 0.05), (250, (4, 16, 16), 8, 2, 1.0, 0.36, 0.05), (250, (3, 3, 3), 4, 1, 0.5, 0.3, 0.9),
         (256, (3, 3, 3), 4, 2, 0.0, 0.05, 0.36), (256, (4, 16, 16), 3, 1, 0.5, 0.9, 0.3), (4096, (4, 16, 16), 8, 1, 0.5, 0.3, 0.05),
         (4096, (3, 3, 3), 3, 2, 0.5, 0.36, 0.9)]


@pytest.mark.parametrize("B,chw,E,min_active,ep,ubw,vbw", CASES, ids=[f"B{c[0]}-{'x'.join(map(str, c[1]))}-E{c[2]}-k{c[3]}-ep{c[4]}" for c in CASES])
def test_outputs_follow_the_rng_contract(B, chw, E, min_active, ep, ubw, vbw):
    from hdmoe_hip import ops
    step, p_mean, p_std = 11, -0.4, 1.0
    b, x0, ug, vg = _generate(B, chw, E, min_active, ep, step, p_mean, p_std, ubw, vbw)
    torch.cuda.synchronize()
    sigma = b["sigma"].flatten()
    src = b["src"].long()
    # shuffle: a permutation
    assert sorted(src.tolist()) == list(range(B))
    # zeta
    assert float(b["zeta"]) == float(torch.tensor(0.25, dtype=torch.float32))
    # sigma: log-normal part against the keyed draws, log-uniform part in range
    n_ln = int(B * (1 - ep))
    z = ops.randn_keyed(torch.empty(B, device=DEV), SEED, 4 * step + 1).double()
    want = torch.exp(p_mean + p_std * z[src]).clamp(SMIN, SMAX)
    ln = src < n_ln
    assert int(ln.sum()) == n_ln
    err = ((sigma.double() - want).abs() / want)[ln]
    print(f"sigma log-normal: max rel err {float(err.max()) if n_ln else 0.0:.3e} over {n_ln}")
    assert n_ln == 0 or float(err.max()) <= 1e-5
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert bool(((sigma >= f32(SMIN)) & (sigma <= f32(SMAX))).all())
    if n_ln < B:                                              # not the log-normal formula: the tail really is another draw
        assert not torch.allclose(sigma.double()[~ln], want[~ln], rtol=1e-3)
    # noise: (x - x0) / sigma is the r = 0 stream
    eps_ref = ops.randn_keyed(b["x"], SEED, 4 * step).double()
    sg = sigma.double().view(B, 1, 1, 1)
    eps = (b["x"].double() - x0.double()) / sg
    tol = 1e-5 * eps_ref.abs().clamp(min=1.0) / sg.clamp(max=1.0)
    ok = (eps - eps_ref).abs() <= tol
    xr = x0.double() + sg * eps_ref
    under = (sg * eps_ref).abs() < 2.0 ** -20 * x0.double().abs()          # sigma eps below the last bits of x0
    ok |= under & ((b["x"].double() - xr).abs() <= 1e-6 * xr.abs())
    print(f"noise: max |eps - ref| / tol = {float(((eps - eps_ref).abs() / tol).max()):.3e}")
    assert bool(ok.all())
    # masks: the torch MaskGenerator on the generator's own sigma
    total = bad = 0
    for key, gen, bw in (("unet_mask", ug, ubw), ("vit_mask", vg, vbw)):
        got = b[key]
        ref = gen(b["sigma"], step)
        assert bool(((got == 0) | (got == 1)).all())
        assert bool((got.sum(1) >= min_active).all())
        diff = got != ref
        total += diff.numel()
        bad += int(diff.sum())
        if bool(diff.any()):
            s64 = sigma.double()
            pct = (0.5 * (1 + torch.erf((torch.log(s64) - p_mean) / (p_std * math.sqrt(2))))).clamp(0, 1)
            dist = (pct.view(-1, 1) - gen.expert_centers.to(DEV).double().view(1, -1)).abs()
            assert float((dist[diff] - bw).abs().max()) < 1e-5
    print(f"masks: {bad} of {total} entries differ from the torch generator")
    assert bad <= 1e-3 * total
    # determinism: the same (seed, step) again, bit for bit
    b2, *_ = _generate(B, chw, E, min_active, ep, step, p_mean, p_std, ubw, vbw, x0=x0)
    for k in b:
        assert torch.equal(b[k], b2[k]), k


def test_shuffle_varies_and_mixes():
    B, chw = 256, (3, 3, 3)
    x0 = _x0(B, chw)
    srcs, share = [], 0
    for step in range(64):
        b, *_ = _generate(B, chw, 4, 1, 0.5, step, x0=x0)
        src = b["src"].clone()
        srcs.append(src)
        share += int((src[:128] < 128).sum())
    assert all(sorted(s.tolist()) == list(range(B)) for s in srcs[:4])
    assert not torch.equal(srcs[0], srcs[1])
    other, *_ = _generate(B, chw, 4, 1, 0.5, 0, x0=x0, seed=SEED + 1)
    assert not torch.equal(srcs[0], other["src"])
    share /= 64 * 128
    print(f"share of first-half positions holding a log-normal sample: {share:.4f}")
    assert abs(share - 0.5) <= 0.03                           # > 4 sigma of the hypergeometric spread over 8192 draws; no shuffle: 1.0


def _mixture_cdf(s, p_mean, p_std, w):
    """CDF of the clamped mixture w LogNormal(p_mean, p_std) + (1 - w) LogUniform(SMIN, SMAX) at s in [SMIN, SMAX] (float64)."""
    ls = torch.log(s)
    ln = 0.5 * (1 + torch.erf((ls - p_mean) / (p_std * math.sqrt(2))))
    lu = ((ls - math.log(SMIN)) / (math.log(SMAX) - math.log(SMIN))).clamp(0, 1)
    f = w * ln + (1 - w) * lu
    return torch.where(s >= SMAX, torch.ones_like(f), f)


@pytest.mark.parametrize("B", [256, 250])
@pytest.mark.parametrize("p_mean,p_std,ep", [(-0.4, 1.0, 0.5), (-1.2, 1.6, 0.5), (-0.4, 1.0, 0.2)])
def test_sigma_distribution_kolmogorov_smirnov(B, p_mean, p_std, ep):
    chw = (3, 3, 3)
    x0 = _x0(B, chw)
    pool = []
    for step in range(64):
        b, *_ = _generate(B, chw, 4, 1, ep, step, p_mean, p_std, x0=x0)
        pool.append(b["sigma"].flatten().clone())
    s = torch.sort(torch.cat(pool).double().cpu()).values
    n = s.numel()
    f = _mixture_cdf(s, p_mean, p_std, int(B * (1 - ep)) / B)
    i = torch.arange(1, n + 1, dtype=torch.float64)
    d = float(torch.maximum(i / n - f, f - (i - 1) / n).max())
    print(f"KS: D sqrt(n) = {d * math.sqrt(n):.3f} (n = {n})")
    assert d * math.sqrt(n) <= 2.2                            # p ~ 1e-4; the seed is fixed


def _device_inputs(seed, rank, mask_over=None):
    from Utils import configs
    from Utils.utils import DeviceInputs, MaskGenerator, ZetaScheduler
    mc = dict(configs.mask_configs, **(mask_over or {}))
    mcfg = dict(configs.model_configs, total_steps=4)
    mk = lambda attr, rng: MaskGenerator(expert_attributes=mc[attr], p_mean=mc["p_mean"], p_std=mc["p_std"], total_steps=mcfg["total_steps"],
                                         min_active=mc["min_active"], step_size=mc["step_size"], max_bandwidth=mc["max_BW"], bandwidth=mc["BW"],
                                         strat_band=mc["strat_band"], noise_range=mc[rng])
    zc = configs.zeta_configs
    zs = ZetaScheduler(total_steps=zc["total_schedule_steps"], max_zeta=zc["max_zeta"], min_zeta=zc["min_zeta"], strategy=zc["strategy"],
                       warmup_ratio=zc["warmup_ratio"])
    return DeviceInputs(mcfg, mc, zc, mk("unet_attr", "unet_noise_range"), mk("vit_attr", "vit_noise_range"), zs, seed=seed, rank=rank), zs


def test_device_inputs_owns_static_buffers_keyed_by_seed_rank_step():
    from hdmoe_hip import ops
    lat = _x0(6, (4, 16, 16))
    di, zs = _device_inputs(SEED, 0)
    a = di.generate(lat, 3)
    assert set(a) == {"sigma", "x", "unet_mask", "vit_mask", "zeta", "src"}
    ptrs = {k: v.data_ptr() for k, v in a.items()}
    first = {k: v.clone() for k, v in a.items()}
    assert float(a["zeta"]) == float(torch.tensor(zs.get_zeta(3), dtype=torch.float32))
    c = di.generate(lat, 4)
    assert {k: v.data_ptr() for k, v in c.items()} == ptrs                 # views of the same static buffers
    assert not torch.equal(c["sigma"], first["sigma"]) and not torch.equal(c["x"], first["x"])
    again = di.generate(lat, 3)
    for k in first:
        assert torch.equal(again[k], first[k]), k
    # the key is the seed alone: a second object with the same seed, and the raw call, give the same bits
    other, _ = _device_inputs(SEED, 0)
    assert torch.equal(other.generate(lat, 3)["x"], first["x"])
    eps_ref = ops.randn_keyed(lat, SEED, 4 * 3).double()
    eps = (first["x"].double() - lat.double()) / first["sigma"].double()
    assert bool(((eps - eps_ref).abs() <= 1e-5 * eps_ref.abs().clamp(min=1.0) / first["sigma"].double().clamp(max=1.0)).all())
    r1, _ = _device_inputs(SEED, 1)
    assert r1.seed == (SEED + 0x9E3779B97F4A7C15) % (1 << 64)
    assert not torch.equal(r1.generate(lat, 3)["sigma"], first["sigma"])
    with pytest.raises(ValueError):
        di.generate(_x0(5, (4, 16, 16)), 3)


def test_errors_raise_before_anything_is_written():
    def untouched(b):
        torch.cuda.synchronize()
        return all(bool((v == -7).all()) for v in b.values())

    for B, E, k in ((4097, 4, 1), (6, 9, 1), (6, 4, 5)):
        buf = _buffers(B, (3, 3, 3), E)
        with pytest.raises(ValueError):
            _generate(B, (3, 3, 3), E, k, 0.5, 0, buf=buf)
        assert untouched(buf), (B, E, k)
    buf = _buffers(6, (4, 16, 16), 4)
    x0 = _x0(6, (16, 16, 4)).permute(0, 3, 1, 2)               # (6, 4, 16, 16), not contiguous
    assert not x0.is_contiguous()
    with pytest.raises(ValueError):
        _generate(6, (4, 16, 16), 4, 1, 0.5, 0, x0=x0, buf=buf)
    assert untouched(buf)


@pytest.mark.parametrize("n", [5, 4 * 7, 6 * 4 + 3])
def test_tensor_scale_matches_float_scale_bit_for_bit(n):
    import hdmoe_hip
    from hdmoe_hip import ops
    x = torch.empty(n, device=DEV)
    hdmoe_hip.manual_seed(99)
    a = ops.randn_like(x, torch.tensor([0.37], device=DEV))
    hdmoe_hip.manual_seed(99)
    b = ops.randn_like(x, 0.37)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    with pytest.raises(ValueError):
        ops.randn_like(x, torch.tensor([0.37, 1.0], device=DEV))


def test_tensor_scale_is_live_under_graph_replay():
    import hdmoe_hip
    from hdmoe_hip import ops
    x = torch.empty(6, 4, device=DEV)
    zt = torch.ones(1, device=DEV)
    hdmoe_hip.manual_seed(7)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ops.randn_like(x, zt)                                 # library loaded, step counter allocated: nothing of that inside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.randn_like(x, zt)
    g.replay()
    torch.cuda.synchronize()
    base = out.clone()
    assert float(base.abs().min()) > 0
    zt.fill_(0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, 0.5 * base)
    zt.fill_(-3.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, -3.0 * base)
    zt.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert bool((out == 0).all())
