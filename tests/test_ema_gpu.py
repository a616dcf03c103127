"""GPU tests of the fused weight EMA (hdmoe_hip/ema.py over csrc/ema.hip).

The reference project has no EMA, so the yardstick is the fp64 recursion e_t = e_{t-1} + a_t (p_t - e_{t-1}) written out below, with
a_t = 1 - (1 - 1/t)^(gamma + 1) (power profile; a_1 = 1) or a_t = 1 - beta (constant decay).  The tolerance is not a constant: next to
the fp64 recursion the same sequence runs as an fp32 ``torch.Tensor.lerp_`` chain on the CPU (weight computed in fp64, rounded to fp32),
and the kernel's maximum error may be at most twice that chain's maximum error plus one fp32 ulp of the largest |e| -- the factor 2
covers fma contraction and a different rounding of a.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 4095, 4096, 4097, 70001)
ODD_VIEW = 5003                                     # elements of the parameter that is a view one element into a larger buffer


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    hdmoe_hip.set_compute_dtype(torch.float32)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


def _weight(mode, coef, t):
    if mode == "constant":
        return 1.0 - coef
    return 1.0 if t <= 1 else -math.expm1((coef + 1.0) * math.log1p(-1.0 / t))


class Recursion:
    """fp64 recursion and the fp32 lerp_ chain over a sequence of CPU fp32 parameter snapshots, for every profile."""

    def __init__(self, init, mode, coefs):
        self.mode, self.coefs, self.t = mode, list(coefs), 0
        self.e64 = [[p.double().clone() for p in init] for _ in self.coefs]
        self.e32 = [[p.float().clone() for p in init] for _ in self.coefs]

    def step(self, ps):
        self.t += 1
        for k, c in enumerate(self.coefs):
            a = _weight(self.mode, c, self.t)
            a32 = float(np.float32(a))
            for i, p in enumerate(ps):
                if a == 1.0:
                    self.e64[k][i] = p.double().clone()
                else:
                    self.e64[k][i] += a * (p.double() - self.e64[k][i])
                self.e32[k][i].lerp_(p.float(), a32)

    def errors(self, k, views):
        """(kernel max error, lerp_ chain max error, one fp32 ulp of the largest |e|) of profile k."""
        kern = max(float((v.detach().cpu().double() - e).abs().max()) for v, e in zip(views, self.e64[k]))
        chain = max(float((c.double() - e).abs().max()) for c, e in zip(self.e32[k], self.e64[k]))
        emax = max(float(e.abs().max()) for e in self.e64[k])
        return kern, chain, float(np.spacing(np.float32(emax)))

    def check(self, k, views, what):
        kern, chain, ulp = self.errors(k, views)
        msg = f"{what}, profile {k}, t = {self.t}: kernel max err {kern:.3e}, fp32 lerp_ chain max err {chain:.3e}, ulp(max|e|) {ulp:.3e}"
        print(msg)
        assert kern <= 2.0 * chain + ulp, msg


class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def make_bag(seed):
    """(module on the device, CPU fp32 master copies): the SIZES tensors plus one view at an odd element offset (scalar path)."""
    gen = torch.Generator().manual_seed(seed)
    cpu = [torch.randn(n, generator=gen) for n in SIZES] + [torch.randn(ODD_VIEW, generator=gen)]
    buf = torch.zeros(ODD_VIEW + 8, device=DEV)
    dev_t = [c.to(DEV) for c in cpu[:-1]] + [buf[1:1 + ODD_VIEW]]
    bag = Bag(dev_t)
    with torch.no_grad():
        bag.ps[-1].copy_(cpu[-1])
    assert bag.ps[-1].data_ptr() % 16 != 0 and all(p.data_ptr() % 16 == 0 for p in list(bag.ps)[:-1])
    return bag, cpu, gen


def perturb(bag, cpu, gen, scale=0.02):
    with torch.no_grad():
        for p, c in zip(bag.ps, cpu):
            c.add_(scale * torch.randn(c.shape, generator=gen))
            p.copy_(c)


def views_of(ema, k):
    return list(ema.profile_state_dict(k).values())


# ------------------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("mode", ["power", "constant"])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_update_matches_the_fp64_recursion(K, mode):
    from hdmoe_hip.ema import WeightEMA, sigma_rel_to_gamma
    bag, cpu, gen = make_bag(10 + K)
    if mode == "power":
        srel = [0.05, 0.10, 0.15, 0.25][:K]
        ema = WeightEMA(bag, sigma_rels=srel)
        coefs = [sigma_rel_to_gamma(s) for s in srel]
    else:
        coefs = [0.999, 0.99, 0.9, 0.5][:K]
        ema = WeightEMA(bag, betas=coefs)
    ref = Recursion(cpu, mode, coefs)
    for t in range(200):
        perturb(bag, cpu, gen)
        ema.update()
        ref.step(cpu)
        if t in (0, 1, 49):
            for k in range(K):
                ref.check(k, views_of(ema, k), f"K={K} {mode}")
    assert ema.step == 200
    for k in range(K):
        ref.check(k, views_of(ema, k), f"K={K} {mode}")
    for p, c in zip(bag.ps, cpu):                                       # the update reads the parameters only
        assert torch.equal(p.detach().cpu(), c)


# ------------------------------------------------------------------------------------------------------------ 2. exactness
def test_first_update_copies_and_a_constant_parameter_is_a_fixed_point():
    from hdmoe_hip.ema import WeightEMA
    bag, cpu, gen = make_bag(3)
    ema = WeightEMA(bag, sigma_rels=(0.05, 0.10, 0.25))
    perturb(bag, cpu, gen, scale=1.0)                                   # p changed since construction
    ema.update()
    for k in range(3):
        for v, p in zip(views_of(ema, k), bag.ps):
            assert torch.equal(v, p.detach())
    for _ in range(50):
        ema.update()
    assert ema.step == 51
    for k in range(3):
        for v, p in zip(views_of(ema, k), bag.ps):
            assert torch.equal(v, p.detach())


# ------------------------------------------------------------------------------------------------------------ 3. determinism
def test_two_objects_on_the_same_sequence_are_bit_identical():
    from hdmoe_hip.ema import WeightEMA
    bag, cpu, gen = make_bag(5)
    a, b = WeightEMA(bag, sigma_rels=(0.05, 0.10)), WeightEMA(bag, sigma_rels=(0.05, 0.10))
    for _ in range(20):
        perturb(bag, cpu, gen)
        a.update()
        b.update()
    assert a.step == b.step == 20
    for k in range(2):
        for va, vb in zip(views_of(a, k), views_of(b, k)):
            assert torch.equal(va, vb)
        assert not torch.equal(views_of(a, k)[-2], bag.ps[-2].detach())


# ------------------------------------------------------------------------------------------------------------ 4. graph capture
def _opt_setup(seed):
    from hdmoe_hip.ema import WeightEMA
    from hdmoe_hip.optim import FusedAdamW
    torch.manual_seed(seed)
    m = torch.nn.ModuleList([torch.nn.Linear(37, 129), torch.nn.Linear(129, 70)]).to(DEV)
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    return m, FusedAdamW(m.parameters(), lr=1e-2), WeightEMA(m, sigma_rels=(0.05, 0.10))


def test_captured_step_and_update_replay_like_eager_calls():
    (ma, oa, ea), (mb, ob, eb) = _opt_setup(7), _opt_setup(7)
    for o, e in ((oa, ea), (ob, eb)):                                   # first call builds the tables (host work, outside the capture)
        o.step(); e.update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # one stream, no parallel branches
        oa.step(); ea.update()
    for _ in range(5):
        graph.replay()
        ob.step(); eb.update()
    torch.cuda.synchronize()
    assert ea.step == eb.step == 6
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
    for k in range(2):
        for va, vb in zip(views_of(ea, k), views_of(eb, k)):
            assert torch.equal(va, vb)
        assert not torch.equal(views_of(ea, k)[0], next(ma.parameters()).detach())


# ------------------------------------------------------------------------------------------------------------ 5. skipped expert
def test_expert_skipped_by_the_optimizer_is_still_averaged():
    from hdmoe_hip.ema import WeightEMA, sigma_rel_to_gamma
    from hdmoe_hip.optim import FusedAdamW
    torch.manual_seed(3)
    experts = torch.nn.ModuleList([torch.nn.Linear(5, 7) for _ in range(3)]).to(DEV)
    opt = FusedAdamW(experts.parameters(), lr=1e-2, weight_decay=0.1)
    opt.track_expert_usage([experts])
    usage = torch.zeros(3, device=DEV)
    object.__setattr__(experts, "_hdmoe_usage", usage)
    srel = (0.05, 0.25)
    ema = WeightEMA(experts, sigma_rels=srel)
    snap = lambda: [p.detach().cpu().clone() for p in experts.parameters()]
    ref = Recursion(snap(), "power", [sigma_rel_to_gamma(s) for s in srel])
    e1 = [i for i, (n, _) in enumerate(experts.named_parameters()) if n.startswith("1.")]
    assert len(e1) == 2
    # 30 steps with samples for expert 1, then 4 without: by then a_t is small enough (0.45 and 0.05 at t = 31) that the averages
    # are still far from the parameters, so "moves every step" is a fair demand of all four steps
    plan = [(4, 3, 2), (1, 3, 1), (2, 5, 5)] * 10 + [(2, 0, 1), (3, 0, 3), (1, 0, 1), (2, 0, 2)]
    for it, used in enumerate(plan):
        usage.copy_(torch.tensor(used, dtype=torch.float32))
        for e in range(3):
            for p in experts[e].parameters():
                p.grad = torch.randn_like(p) if used[e] else torch.zeros_like(p)
        before_p = snap()
        before_e = [[v.clone() for v in views_of(ema, k)] for k in range(2)]
        opt.step()
        ema.update()
        now = snap()
        ref.step(now)
        for i in e1:
            assert torch.equal(now[i], before_p[i]) == (used[1] == 0), (it, i)         # phase 2: expert 1 stands still ...
            for k in range(2):
                assert not torch.equal(views_of(ema, k)[i], before_e[k][i]), (it, i, k)   # ... and its average moves every step
        if it >= 29:
            for k in range(2):
                ref.check(k, views_of(ema, k), f"skipped expert, step {it}")
    assert ema.step == 34


# ------------------------------------------------------------------------------------------------------------ 6./7. swap, sampler
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


def _averaged(model, steps=3):
    """A WeightEMA whose profiles differ from the raw parameters: a few perturbed steps."""
    from hdmoe_hip.ema import WeightEMA
    ema = WeightEMA(model, sigma_rels=(0.05, 0.25))
    gen = torch.Generator(device=DEV).manual_seed(11)
    for _ in range(steps):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.05 * torch.randn(p.shape, device=DEV, generator=gen))
        ema.update()
    return ema


def _loaded_from_profile(g, mk, ema, k):
    m2 = mk()
    m2.load_state_dict(g["state"])                                         # buffers; every parameter is overwritten below
    m2 = m2.to(DEV).eval()
    res = m2.load_state_dict(ema.profile_state_dict(k), strict=False)
    assert not res.unexpected_keys and all(n not in dict(m2.named_parameters()) for n in res.missing_keys)
    return m2


def _same(a, b, run_to_run, what):
    """Equality up to the run-to-run difference of the same computation measured in the test (bitwise when that is zero)."""
    if run_to_run == 0.0:
        assert torch.equal(a, b), f"{what}: max diff {float((a - b).abs().max()):.3e}, run-to-run 0"
    else:
        d = float((a - b).abs().max())
        assert d <= run_to_run, f"{what}: max diff {d:.3e} > run-to-run {run_to_run:.3e}"


@pytest.mark.parametrize("k", [0, 1])
def test_swapped_context_exchanges_and_restores(k):
    g, mk, model = _real_model()
    ema = _averaged(model)
    raw = {n: p.detach().clone() for n, p in model.named_parameters()}
    prof = {n: v.clone() for n, v in ema.profile_state_dict(k).items()}
    assert list(prof) == [n for n, _ in model.named_parameters()] and set(prof) <= set(model.state_dict())
    assert any(not torch.equal(prof[n], raw[n]) for n in raw)
    out_raw = _forward(model, g)
    rr = float((_forward(model, g) - out_raw).abs().max())                 # run-to-run difference of this forward
    ref_out = _forward(_loaded_from_profile(g, mk, ema, k), g)
    with ema.swapped(k):
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), prof[n]), n
        out_sw = _forward(model, g)
        with pytest.raises(RuntimeError):
            ema.update()
        with pytest.raises(RuntimeError):
            with ema.swapped(k):
                pass
    _same(out_sw, ref_out, rr, "forward inside swapped() vs a model loaded from the profile")
    assert not torch.equal(out_sw, out_raw)
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), raw[n]), n
    for n, v in ema.profile_state_dict(k).items():
        assert torch.equal(v, prof[n]), n
    _same(_forward(model, g), out_raw, rr, "forward after the context")
    ema.update()                                                           # allowed again


def test_sampler_graph_notices_the_swap():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils"))
    from EDM_sampler import EDM_Sampler
    g, mk, model = _real_model()
    ema = _averaged(model)
    noise = torch.randn(2, 4, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    text = g["text"][:2].to(DEV)
    s = EDM_Sampler(model, model, num_solve_steps=4, use_graph=True)
    out_raw = s.sample(noise, text, -1.2, 1.6).clone()
    rr = float((s.sample(noise, text, -1.2, 1.6) - out_raw).abs().max())
    m2 = _loaded_from_profile(g, mk, ema, 0)
    ref_out = EDM_Sampler(m2, m2, num_solve_steps=4, use_graph=True).sample(noise, text, -1.2, 1.6).clone()
    with ema.swapped(0):
        out_sw = s.sample(noise, text, -1.2, 1.6).clone()
    _same(out_sw, ref_out, rr, "graph sampler inside swapped(0) vs a fresh model and sampler loaded from profile 0")
    assert not torch.equal(out_sw, out_raw)
    _same(s.sample(noise, text, -1.2, 1.6), out_raw, rr, "graph sampler after the context")


# ------------------------------------------------------------------------------------------------------------ 8. trainer, checkpoint
def test_trainer_hook_and_checkpoint_roundtrip(tmp_path):
    """Tiny configuration of tests/test_host_abi.py::test_checkpoint_dictionary_layout, bf16 expert arithmetic like the other Trainer tests
    (parameters and averages are fp32 either way)."""
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    try:
        _trainer_roundtrip(tmp_path)
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)


def _trainer_roundtrip(tmp_path):
    from Utils import configs, training
    from hdmoe_hip.ema import WeightEMA, sigma_rel_to_gamma
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
    names = [n for n, _ in model.named_parameters()]
    assert ema.names == names
    snap = lambda: [p.detach().cpu().clone() for p in model.parameters()]
    ref = Recursion(snap(), "power", [sigma_rel_to_gamma(s) for s in srel])
    tr = training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, configs.zeta_configs, ema=ema)
    gen = torch.Generator(device=DEV).manual_seed(1)
    batches = [(0.5 * torch.randn(6, 4, 16, 16, device=DEV, generator=gen), torch.randn(6, 5, 32, device=DEV, generator=gen)) for _ in range(4)]
    snaps = []
    training.train_steps(tr, batches, on_step=lambda s, r: snaps.append(snap()))
    assert ema.step == 4 and len(snaps) == 4
    assert any(not torch.equal(a, b) for a, b in zip(snaps[0], snaps[-1]))
    for s in snaps:
        ref.step(s)
    for k in range(2):
        ref.check(k, views_of(ema, k), "trainer")
    path = training.save_checkpoint(model, tr.optimizer, 4, 0.5, {"model_configs": mcfg}, "ckpt_ema.pt", ema=ema)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"step", "model_state_dict", "optimizer_state_dict", "mse", "config", "ema_state_dict"}
    es = ck["ema_state_dict"]
    assert set(es) == {"step", "mode", "sigma_rels", "gammas", "betas", "profiles"} and es["step"] == 4 and es["mode"] == "power"
    assert es["betas"] is None and es["sigma_rels"] == list(srel) and len(es["profiles"]) == 2 and list(es["profiles"][0]) == names
    model2 = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg)).to(DEV)
    opt2 = training.build_optimizer(model2, configs.optim_configs)
    ema2 = WeightEMA(model2, sigma_rels=srel)
    training.load_checkpoint(path, model2, opt2, map_location=DEV, ema=ema2)
    assert ema2.step == 4
    for _ in range(2):                                                     # as loaded, then after one further update on both
        for k in range(2):
            for a, b in zip(views_of(ema, k), views_of(ema2, k)):
                assert torch.equal(a, b)
        ema.update(); ema2.update()
    assert ema.step == ema2.step == 6
    bad = dict(es, profiles=[{("x" + n): v for n, v in p.items()} for p in es["profiles"]])
    with pytest.raises(KeyError):
        ema2.load_state_dict(bad)
    path = training.save_checkpoint(model, tr.optimizer, 4, 0.5, {"model_configs": mcfg}, "ckpt_plain.pt")
    assert set(torch.load(path, map_location="cpu", weights_only=False)) == {"step", "model_state_dict", "optimizer_state_dict", "mse", "config"}
    training.load_checkpoint(path, model2, opt2, map_location=DEV, ema=ema2)   # a file without an EMA leaves it alone
    assert ema2.step == 6
