"""GPU tests of the post-hoc EMA reconstruction (hdmoe_hip/posthoc.py over hdmoe_mt_combine in csrc/ema.hip).

The reference project has no EMA, so the yardstick is the fp64 combination written out below.  The kernel keeps one fp64 fma chain per
element and target and rounds to fp32 once, so elementwise

    |kernel - ref64| <= 0.5 ulp_fp32(ref64) + nsrc 2^-52 sum_s |w_s| |x_s|

the first term being the final rounding, the second the rounding of two fp64 sums of nsrc terms (the kernel's chain and numpy's own, each at
most nsrc 2^-53 sum |w_s x_s|).  Nothing in the bound is fitted to what the kernel returns.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 4095, 4096, 4097, 70001)
ODD_VIEW = 5003                                     # elements of the tensors that are views one element into a larger buffer
GUARD = 777.0                                       # fills everything around a target
SHAPES = [(1, 1), (2, 3), (7, 8), (40, 8), (300, 5)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    hdmoe_hip.set_compute_dtype(torch.float32)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------ helpers
def combine(srcs, dsts, W, numel):
    """One hdmoe_mt_combine launch: flat fp32 device tensors (or views) srcs / dsts of `numel` elements, W fp64 [nsrc][ndst]."""
    from hdmoe_hip._lib import call
    assert W.shape == (len(srcs), len(dsts)) and all(t.numel() == numel and t.dtype == torch.float32 for t in list(srcs) + list(dsts))
    st = torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64).to(DEV)
    dt = torch.tensor([t.data_ptr() for t in dsts], dtype=torch.int64).to(DEV)
    w = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(DEV)
    call("hdmoe_mt_combine", st, dt, len(srcs), len(dsts), numel, w)
    torch.cuda.synchronize()


def bound_check(out, xs, W, what):
    """out: fp32 [ndst][n] from the kernel; xs: fp32 [nsrc][n]; W: fp64 [nsrc][ndst].  Prints the figures, then asserts the bound of the
    module docstring for every element of every target."""
    x64 = xs.astype(np.float64)
    ref = W.T @ x64
    mag = np.abs(W).T @ np.abs(x64)
    bound = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + W.shape[0] * 2.0 ** -52 * mag
    err = np.abs(out.astype(np.float64) - ref)
    worst = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    msg = (f"{what}: max err {err.max():.3e}, worst err/bound {err[worst] / bound[worst]:.3f} (err {err[worst]:.3e}, bound {bound[worst]:.3e}, "
           f"|ref| {abs(ref[worst]):.3e}), max |w| {np.abs(W).max():.3e}")
    print(msg)
    assert np.all(np.isfinite(out)) and np.all(err <= bound), msg


def solved_weights(nsrc, ndst):
    """Real solve_weights output for nsrc saved profiles and ndst targets at the last saved step."""
    from hdmoe_hip.ema import sigma_rel_to_gamma
    from hdmoe_hip.posthoc import solve_weights
    tracked = {1: (0.05,), 2: (0.05, 0.10), 7: (0.10,), 40: (0.05, 0.10), 300: (0.05, 0.10, 0.20)}[nsrc]
    nsteps = nsrc // len(tracked)
    every = 20 if nsrc == 300 else 50
    steps = [every * (i + 1) for i in range(nsteps) for _ in tracked]
    gammas = [sigma_rel_to_gamma(s) for _ in range(nsteps) for s in tracked]
    targets = [0.075, 0.15, 0.03, 0.20, 0.06, 0.12, 0.25, 0.04][:ndst]
    X, _ = solve_weights(steps, gammas, [steps[-1]] * ndst, [sigma_rel_to_gamma(s) for s in targets])
    assert X.shape == (nsrc, ndst)
    return X


def adversarial_weights(nsrc, ndst, seed):
    """Alternating signs, magnitudes log-uniform in [1e-3, 1e3] with the largest pinned to 1e3: heavy cancellation."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-3.0, 3.0, size=(nsrc, ndst))
    mag[rng.integers(nsrc), :] = 1e3
    return mag * np.where(np.arange(nsrc) % 2 == 0, 1.0, -1.0)[:, None]


# ------------------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("kind", ["solved", "adversarial"])
@pytest.mark.parametrize("nsrc,ndst", SHAPES)
def test_combine_matches_the_fp64_combination(nsrc, ndst, kind):
    W = solved_weights(nsrc, ndst) if kind == "solved" else adversarial_weights(nsrc, ndst, 100 * nsrc + ndst)
    gen = torch.Generator().manual_seed(7 * nsrc + ndst)
    for numel in SIZES + (ODD_VIEW,):
        odd = numel == ODD_VIEW                                              # one source and one target start 4 bytes off: scalar path
        cpu = torch.randn(nsrc, numel, generator=gen)
        srcs = [cpu[s].to(DEV) for s in range(nsrc)]
        if odd:
            sbuf = torch.zeros(numel + 8, device=DEV)
            sbuf[1:1 + numel].copy_(cpu[nsrc // 2])
            srcs[nsrc // 2] = sbuf[1:1 + numel]
        slot = (numel + 64 + 63) // 64 * 64                                  # every target sits in one guarded arena, 32 elements in
        arena = torch.full((ndst * slot,), GUARD, device=DEV)
        offs = [t * slot + 32 + (1 if odd and t == ndst - 1 else 0) for t in range(ndst)]
        dsts = [arena[o:o + numel] for o in offs]
        aligned = [t.data_ptr() % 16 == 0 for t in srcs + dsts]
        assert all(aligned) != odd and sum(not a for a in aligned) == (2 if odd else 0)
        combine(srcs, dsts, W, numel)
        got = arena.cpu().numpy()
        keep = np.ones(arena.numel(), dtype=bool)
        for o in offs:
            keep[o:o + numel] = False
        bound_check(np.stack([got[o:o + numel] for o in offs]), cpu.numpy(), W, f"{kind} nsrc={nsrc} ndst={ndst} numel={numel}")
        assert np.all(got[keep] == GUARD), "the kernel wrote outside a target"
        for s in range(nsrc):                                                # the sources are read only
            assert torch.equal(srcs[s].cpu(), cpu[s])


# ------------------------------------------------------------------------------------------------------------ 2. determinism
def test_runs_and_target_groupings_are_bit_identical():
    nsrc, ndst, numel = 40, 11, 70001
    gen = torch.Generator().manual_seed(3)
    srcs = [torch.randn(numel, generator=gen).to(DEV) for _ in range(nsrc)]
    W = adversarial_weights(nsrc, ndst, 5)
    run = lambda groups: _grouped(srcs, W, numel, groups)
    a = run([range(0, 8), range(8, 11)])
    b = run([range(0, 8), range(8, 11)])
    c = run([[t] for t in range(ndst)])
    d = run([range(0, 3), range(3, 11)])
    for t in range(ndst):
        assert torch.equal(a[t], b[t]), f"target {t}: two runs differ"
        assert torch.equal(a[t], c[t]), f"target {t}: groups (8, 3) differ from one target per launch"
        assert torch.equal(a[t], d[t]), f"target {t}: groups (8, 3) differ from (3, 8)"
    assert not torch.equal(a[0], a[1])


def _grouped(srcs, W, numel, groups):
    out = [torch.zeros(numel, device=DEV) for _ in range(W.shape[1])]
    for g in groups:
        g = list(g)
        combine(srcs, [out[t] for t in g], W[:, g], numel)
    return out


# ------------------------------------------------------------------------------------------------------------ 3. end to end, bag
class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def make_bag(seed):
    """(module on the device, CPU fp32 master copies): the SIZES tensors plus one view at an odd element offset."""
    gen = torch.Generator().manual_seed(seed)
    cpu = [torch.randn(n, generator=gen) for n in SIZES] + [torch.randn(ODD_VIEW, generator=gen)]
    buf = torch.zeros(ODD_VIEW + 8, device=DEV)
    bag = Bag([c.to(DEV) for c in cpu[:-1]] + [buf[1:1 + ODD_VIEW]])
    with torch.no_grad():
        bag.ps[-1].copy_(cpu[-1])
    return bag, cpu, gen


def perturb(bag, cpu, gen, scale=0.02):
    with torch.no_grad():
        for p, c in zip(bag.ps, cpu):
            c.add_(scale * torch.randn(c.shape, generator=gen))
            p.copy_(c)


def views_of(ema, k):
    return list(ema.profile_state_dict(k).values())


def test_reconstruction_from_snapshots_of_a_parameter_bag(tmp_path):
    from hdmoe_hip import posthoc
    from hdmoe_hip.ema import WeightEMA
    bag, cpu, gen = make_bag(21)
    a, b = WeightEMA(bag, sigma_rels=(0.05, 0.10)), WeightEMA(bag, sigma_rels=(0.075,))
    for t in range(1, 1001):
        perturb(bag, cpu, gen)
        a.update()
        b.update()
        if t % 50 == 0:
            a.save_snapshot(tmp_path / f"ema_{t:08d}.pt")
    rec = posthoc.reconstruct(bag, tmp_path, sigma_rels=[0.05, 0.075, 0.10])
    assert isinstance(rec, posthoc.ReconstructedEMA) and rec.step == 1000 and rec.sigma_rels == [0.05, 0.075, 0.10]
    assert rec.weights.shape == (40, 3) and rec.fit_error.shape == (3,) and rec.fit_error[0] == rec.fit_error[2] == 0.0
    assert 0.0 < rec.fit_error[1] < 0.05 and list(rec.profile_state_dict(1)) == a.names
    for k_rec, k_a in ((0, 0), (2, 1)):                                      # tracked targets: the saved profile itself, bit for bit
        for v, e in zip(views_of(rec, k_rec), views_of(a, k_a)):
            assert torch.equal(v, e)
    states = posthoc.load_sources(tmp_path)
    saved = [(st, k) for st in states for k in range(2)]
    err = near = 0.0
    for i, name in enumerate(a.names):
        xs = np.stack([st["profiles"][k][name].numpy().reshape(-1) for st, k in saved])
        got = views_of(rec, 1)[i].cpu().numpy().reshape(-1)
        bound_check(got[None], xs, rec.weights[:, 1:2], f"bag tensor {name}")
        live = views_of(b, 0)[i].cpu().numpy().astype(np.float64)
        err = max(err, float(np.abs(got - live).max()))
        near_i = [float(np.abs(views_of(a, k)[i].cpu().numpy().astype(np.float64) - live).max()) for k in range(2)]
        near = max(near, min(near_i))
    print(f"sigma_rel 0.075 at step 1000: reconstruction vs live profile max err {err:.3e}, nearer tracked profile {near:.3e}, "
          f"ratio {near / err:.0f}x, fit_error {rec.fit_error[1]:.3e}")
    assert near >= 10.0 * err


# ------------------------------------------------------------------------------------------------------------ 4. real model
def _real_model():
    from models import model_config2
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    mk = lambda: model_config2.preconditioned_HDMOEM(**g["cfg"])
    model = mk()
    model.load_state_dict(g["state"])
    return g, mk, model.to(DEV).eval()


def _forward(model, g):
    with torch.no_grad():
        out = model(x=g["x"].to(DEV), sigma=g["sigma"].to(DEV), text_emb=g["text"].to(DEV), Unet_router_mask=g["unet_mask"].to(DEV),
                    Vit_router_mask=g["vit_mask"].to(DEV), zeta=0.0, return_log_var=True, **g["extra"])
    return out["denoised"].detach().clone()


def _loaded_from_profile(g, mk, rec, k):
    m2 = mk()
    m2.load_state_dict(g["state"])                                         # buffers; every parameter is overwritten below
    m2 = m2.to(DEV).eval()
    res = m2.load_state_dict(rec.profile_state_dict(k), strict=False)
    assert not res.unexpected_keys and all(n not in dict(m2.named_parameters()) for n in res.missing_keys)
    return m2


def _same(a, b, run_to_run, what):
    """Equality up to the run-to-run difference of the same computation measured in the test (bitwise when that is zero)."""
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), what
    if run_to_run == 0.0:
        assert torch.equal(a, b), f"{what}: max diff {float((a - b).abs().max()):.3e}, run-to-run 0"
    else:
        d = float((a - b).abs().max())
        assert d <= run_to_run, f"{what}: max diff {d:.3e} > run-to-run {run_to_run:.3e}"


SIX = [0.04, 0.05, 0.075, 0.12, 0.18, 0.25]


def _reconstructed(model, tmp_path, steps=3):
    """Six targets from three snapshots of a WeightEMA over a few perturbed steps."""
    from hdmoe_hip import posthoc
    from hdmoe_hip.ema import WeightEMA
    ema = WeightEMA(model, sigma_rels=(0.05, 0.25))
    gen = torch.Generator(device=DEV).manual_seed(11)
    for t in range(1, steps + 1):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.05 * torch.randn(p.shape, device=DEV, generator=gen))
        ema.update()
        ema.save_snapshot(tmp_path / f"ema_{t:08d}.pt")
    rec = posthoc.reconstruct(model, tmp_path, sigma_rels=SIX)
    assert rec.nprofiles == 6 and rec.step == steps and rec.weights.shape == (2 * steps, 6)
    for k_rec, k_ema in ((1, 0), (5, 1)):                                    # the tracked ones come back bit for bit
        for v, e in zip(rec.profile_state_dict(k_rec).values(), ema.profile_state_dict(k_ema).values()):
            assert torch.equal(v, e)
    return rec


def test_swapped_exchanges_and_restores_every_one_of_six_targets(tmp_path):
    g, mk, model = _real_model()
    rec = _reconstructed(model, tmp_path)
    assert not hasattr(rec, "update")
    raw = {n: p.detach().clone() for n, p in model.named_parameters()}
    out_raw = _forward(model, g)
    rr = float((_forward(model, g) - out_raw).abs().max())                 # run-to-run difference of this forward
    outs = []
    for k in range(6):
        prof = {n: v.clone() for n, v in rec.profile_state_dict(k).items()}
        assert list(prof) == list(raw) and any(not torch.equal(prof[n], raw[n]) for n in raw)
        m2 = _loaded_from_profile(g, mk, rec, k)
        ref_out = _forward(m2, g)                                            # a fresh model's first forward ...
        ref_warm = _forward(m2, g)                                           # ... and its later ones, which may differ from the first
        rr_k = max(rr, float((ref_warm - ref_out).abs().max()))              # run-to-run difference of the forward compared against
        rr_warm = float((_forward(m2, g) - ref_warm).abs().max())
        with rec.swapped(k):
            for n, p in model.named_parameters():
                assert torch.equal(p.detach(), prof[n]), (k, n)
            out_sw = _forward(model, g)
            out_sw_again = _forward(model, g)
            with pytest.raises(RuntimeError):
                with rec.swapped(k):
                    pass
            with pytest.raises(RuntimeError):
                rec.profile_state_dict(k)
        dd = lambda a, b: float((a - b).abs().max())
        print(f"target {k}: forward inside swapped() vs a model loaded from the profile: first forwards {dd(out_sw, ref_out):.3e} "
              f"(run-to-run {rr_k:.3e}, raw model {rr:.3e}), later forwards {dd(out_sw_again, ref_warm):.3e} (run-to-run {rr_warm:.3e}), "
              f"max |out| {float(ref_out.abs().max()):.3e}")
        _same(out_sw, ref_out, rr_k, f"forward inside swapped({k}) vs a model loaded from the profile")
        _same(out_sw_again, ref_warm, rr_warm, f"second forward inside swapped({k}) vs the second of a model loaded from the profile")
        assert not torch.equal(out_sw, out_raw)
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), raw[n]), (k, n)
        for n, v in rec.profile_state_dict(k).items():
            assert torch.equal(v, prof[n]), (k, n)
        outs.append(out_sw)
    assert all(not torch.equal(outs[i], outs[j]) for i in range(6) for j in range(i))
    _same(_forward(model, g), out_raw, rr, "forward after the contexts")
    m2 = mk().to(DEV)
    rec.copy_to(m2, 4)
    for (n, p), v in zip(m2.named_parameters(), rec.profile_state_dict(4).values()):
        assert torch.equal(p.detach(), v), n
    with pytest.raises(ValueError):
        rec.swapped(6).__enter__()


def test_sampler_graph_notices_the_swap_of_a_reconstructed_profile(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils"))
    from EDM_sampler import EDM_Sampler
    g, mk, model = _real_model()
    rec = _reconstructed(model, tmp_path)
    k = 4                                                                   # in the second group of four
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    text = g["text"][:2].to(DEV)
    s = EDM_Sampler(model, model, num_solve_steps=4, use_graph=True)
    out_raw = s.sample(noise, text, -1.2, 1.6).clone()
    rr = float((s.sample(noise, text, -1.2, 1.6) - out_raw).abs().max())
    m2 = _loaded_from_profile(g, mk, rec, k)
    s2 = EDM_Sampler(m2, m2, num_solve_steps=4, use_graph=True)
    ref_out = s2.sample(noise, text, -1.2, 1.6).clone()
    rr = max(rr, float((s2.sample(noise, text, -1.2, 1.6) - ref_out).abs().max()))   # ... and of the sampler compared against
    with rec.swapped(k):
        out_sw = s.sample(noise, text, -1.2, 1.6).clone()
    _same(out_sw, ref_out, rr, f"graph sampler inside swapped({k}) vs a fresh model and sampler loaded from the profile")
    assert not torch.equal(out_sw, out_raw)
    _same(s.sample(noise, text, -1.2, 1.6), out_raw, rr, "graph sampler after the context")


# ------------------------------------------------------------------------------------------------------------ 5. trainer
def test_trainer_writes_snapshots_that_reconstruct(tmp_path):
    """Tiny configuration of tests/test_ema_gpu.py::_trainer_roundtrip, bf16 expert arithmetic like the other Trainer tests."""
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    try:
        _trainer_snapshots(tmp_path)
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)


def _trainer_snapshots(tmp_path):
    from Utils import configs, training
    from hdmoe_hip import posthoc
    from hdmoe_hip.ema import SNAPSHOT_FORMAT, WeightEMA
    from models import model_config2
    over = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
                VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8)
    mcfg = dict(configs.model_configs, **over, total_steps=10, save_dir=str(tmp_path))
    torch.manual_seed(0)
    model = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg)).to(DEV)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("out_gain"):
                p.fill_(0.5)                                               # (zero-initialised: nothing would reach the experts' gradients)
    srel = (0.05, 0.10)
    ema = WeightEMA(model, sigma_rels=srel)
    snap_dir = tmp_path / "snaps"
    tr = training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, configs.zeta_configs, ema=ema,
                          ema_snapshot_every=2, ema_snapshot_dir=str(snap_dir))
    gen = torch.Generator(device=DEV).manual_seed(1)
    batches = [(0.5 * torch.randn(6, 4, 16, 16, device=DEV, generator=gen), torch.randn(6, 5, 32, device=DEV, generator=gen)) for _ in range(7)]
    training.train_steps(tr, batches[:6])
    assert ema.step == 6
    assert sorted(os.listdir(snap_dir)) == ["ema_00000002.pt", "ema_00000004.pt", "ema_00000006.pt"]
    files = {}
    for step in (2, 4, 6):
        st = torch.load(snap_dir / f"ema_{step:08d}.pt", map_location="cpu", weights_only=False)
        assert st["step"] == step and st["format"] == SNAPSHOT_FORMAT and st["mode"] == "power" and st["sigma_rels"] == list(srel)
        assert set(st) == {"step", "mode", "sigma_rels", "gammas", "betas", "profiles", "format"} and list(st["profiles"][0]) == ema.names
        files[step] = st
    assert any(not torch.equal(files[2]["profiles"][1][n], files[4]["profiles"][1][n]) for n in ema.names)
    rec = posthoc.reconstruct(model, snap_dir, sigma_rels=[0.10], step=4)
    assert rec.step == 4 and rec.fit_error[0] == 0.0
    for n, v in rec.profile_state_dict(0).items():
        assert torch.equal(v.cpu(), files[4]["profiles"][1][n]), n
    training.train_steps(tr, batches[6:])                                   # step 7: no snapshot of its own
    assert ema.step == 7 and len(os.listdir(snap_dir)) == 3
    path = training.save_checkpoint(model, tr.optimizer, 7, 0.5, {"model_configs": mcfg}, "ckpt_ema.pt", ema=ema)
    rec = posthoc.reconstruct(model, [snap_dir, path], sigma_rels=[0.05, 0.075])
    assert rec.step == 7 and rec.weights.shape == (8, 2) and rec.fit_error[0] == 0.0 and rec.fit_error[1] > 0.0
    for v, e in zip(rec.profile_state_dict(0).values(), ema.profile_state_dict(0).values()):
        assert torch.equal(v, e)
    with pytest.raises(RuntimeError):
        with ema.swapped(0):
            ema.save_snapshot(tmp_path / "inside.pt")
    assert not os.path.exists(tmp_path / "inside.pt")
