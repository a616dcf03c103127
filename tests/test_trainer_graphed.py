"""Trainer(device_inputs=True) and Trainer(graphed=True): the staged hipGraph replay behind the public training loop, its inputs made on the
device per step, zeta live under replay, the optimizer side, resume, the error paths, and the untouched default path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x0BADC0FFEE123457
B = 6


def _model(module_id):
    """BASELINE config 2 at its real width with the recipe's weights, train() mode without randomness (every dropout p = 0), as in
    test_staged_step_matches_plain_backward / test_bench_path_parity._setup."""
    from Utils import configs
    from models import model_config1, model_config2
    from oracle.recipe import fill_state
    mod = model_config1 if module_id == 1 else model_config2
    model = mod.preconditioned_HDMOEM(**configs.model_kwargs(**configs.BASELINE_CONFIGS[2]["over"]))
    model.load_state_dict(fill_state(model.state_dict(), 5))
    model = model.to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model


def _batch(b=B):
    from oracle.recipe import make_inputs
    inp = make_inputs(b, 4, 32, 4, 77, 768, 5)
    return inp["x0"].to(DEV), inp["text"].to(DEV)


def _configs(max_zeta, zeta_steps):
    from Utils import configs
    mcfg = dict(configs.model_configs, top_k=2, total_steps=4)
    mask = dict(configs.mask_configs, step_size=0.5)            # bandwidth 0.3 at steps 0-1, 0.55 at steps 2-3, 0.8 from step 4
    zeta = dict(configs.zeta_configs, total_schedule_steps=zeta_steps, max_zeta=max_zeta, min_zeta=0.0, warmup_ratio=0.0)
    return mcfg, mask, zeta


def _trainer(module_id, max_zeta, zeta_steps, **kw):
    from Utils import configs, training
    mcfg, mask, zeta = _configs(max_zeta, zeta_steps)
    tr = training.Trainer(_model(module_id), mcfg, configs.optim_configs, configs.loss_configs, mask, zeta, **kw)
    tr.usage_seen = []                                          # the routed-row counters each optimizer step read
    inner = tr.optimizer.step

    def step(*a, **k):
        tr.usage_seen.append(tr.buckets.usage.clone())
        return inner(*a, **k)

    tr.optimizer.step = step
    return tr


def _follow(dst, src):
    """dst's model starts its step from src's current weights."""
    from hdmoe_hip import bank
    dst.model.load_state_dict(src.model.state_dict())
    bank.note_weights_changed()


def _follow_after_build(dst, src):
    """The capture's warm-up runs renormalise src's weights in place (train-mode weight prepare) before the first replay: dst copies the
    weights again right behind the build, so that the first step, too, starts from identical weights on both sides."""
    inner = src._build_staged

    def build(*a, **k):
        inner(*a, **k)
        _follow(dst, src)

    src._build_staged = build


def _inputs(tr):
    return {k: v.clone() for k, v in tr.inputs.buf.items()}


# ------------------------------------------------------------------------------------------------------------------ arithmetic per step
ARITH = [(2, torch.bfloat16, 1e-3, 1e-2), (2, torch.float32, 1e-5, 2e-4), (1, torch.bfloat16, 1e-3, 1e-2)]


@pytest.mark.parametrize("module_id,dtype,ltol,gtol", ARITH, ids=["config2-bf16", "config2-fp32", "config1-bf16"])
def test_graphed_step_matches_the_eager_step(module_id, dtype, ltol, gtol):
    """Zeta 0, no dropout: the replayed step and the eager step over the same device-made inputs, from the same weights, four steps.  The
    bounds are those of test_staged_step_matches_plain_backward.  Both sides run the weight-bank path (as there, where the eager
    reference runs twice before it is read): the eager trainer takes two steps first and is set back to step 0."""
    import hdmoe_hip
    from hdmoe_hip import graph as hgraph
    hdmoe_hip.set_compute_dtype(dtype)
    try:
        lat, text = _batch()
        G = _trainer(module_id, 0.0, 4, graphed=True, seed=SEED)
        E = _trainer(module_id, 0.0, 4, device_inputs=True, seed=SEED)
        assert G.device_inputs and G.graphed and E.device_inputs and not E.graphed
        for _ in range(2):
            E.train_step(lat, text)
        E.step_idx = 0
        E.usage_seen.clear()
        _follow_after_build(E, G)
        for step in range(4):
            _follow(E, G)
            rg = G.train_step(lat, text)
            if step == 0:
                want = hgraph.StagedStep.ORDER_R + ["unet_bwd2", "unet_bwd1", "unet_bwd0", "vcomb_bwd", "vr_bwd"]
                if module_id == 1:                              # the ten-graph order (+ the split U-Net / ViT-router sections)
                    assert sorted(G._staged.graphs) == sorted(want)
                assert hgraph.current() is None
            lg = rg["loss"]["loss"].detach().clone()
            gg = {n: p.grad.detach().clone() for n, p in G.model.named_parameters() if p.grad is not None}
            re_ = E.train_step(lat, text)
            torch.cuda.synchronize()
            le = re_["loss"]["loss"].detach()
            print(f"step {step}: loss graphed {float(lg):.7g} eager {float(le):.7g}")
            assert abs(float(lg) - float(le)) <= ltol * abs(float(le)) + 1e-6
            for k in ("sigma", "x", "unet_mask", "vit_mask", "zeta", "src"):
                assert torch.equal(G.inputs.buf[k], E.inputs.buf[k]), k
            bad, worst = [], 0.0
            for n, p in E.model.named_parameters():
                if p.grad is not None:
                    scale = float(p.grad.abs().max())
                    err = float((gg[n] - p.grad).abs().max())
                    worst = max(worst, err / (scale + 1e-30))
                    if err > gtol * scale + 1e-7:
                        bad.append((n, err, scale))
            print(f"step {step}: worst gradient error / max|ref| = {worst:.3e} over {len(gg)} tensors")
            assert not bad, bad[:5]
            assert len(gg) > 400
            # the optimizer saw this step's routing only (the capture's warm-up forwards were cleared): the eager step's counts
            assert torch.equal(G.usage_seen[step], E.usage_seen[step]), (step, G.usage_seen[step], E.usage_seen[step])
            if step == 0:
                assert float(G.buckets.usage.abs().sum()) == 0.0
                net, used = G.model.net, G.usage_seen[0]
                assert float(used.sum()) > 0
                off = 0
                for lst in (net.Unet_experts, net.VIT_experts):
                    for e, expert in enumerate(lst):            # an expert without a routed row was skipped by the update
                        cnt = float(G.optimizer.state[next(expert.parameters())]["step"])
                        assert cnt == (1.0 if float(used[off + e]) > 0 else 0.0), (e, cnt, used)
                    off += len(lst)
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------------ inputs, zeta, optimizer
@pytest.fixture(scope="module")
def live_run():
    """Five steps of a graphed trainer whose zeta falls 2.0, 1.5, 0.5, 0, 0; beside it an eager device-input trainer with the same
    configuration (its own weights), and a zeta-0 eager trainer that starts every step from the graphed trainer's weights."""
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    try:
        lat, text = _batch()
        G = _trainer(2, 2.0, 3, graphed=True, seed=SEED)
        E = _trainer(2, 2.0, 3, device_inputs=True, seed=SEED)
        R = _trainer(2, 0.0, 3, device_inputs=True, seed=SEED)
        before = {n: p.detach().clone() for n, p in G.model.named_parameters()}
        _follow_after_build(R, G)
        rec = dict(G=G, lat=lat, text=text, g_in=[], e_in=[], noise=[], zeta_host=[], before=before, after3=None, sched3=None, rstep3=None)
        for step in range(5):
            _follow(R, G)
            rec["zeta_host"].append(G.zeta_sched.get_zeta(step))
            rg = G.train_step(lat, text)
            raw_g = rg["out_model"]["Unet_raw"].detach().clone()
            rec["g_in"].append(_inputs(G))
            E.train_step(lat, text)
            rec["e_in"].append(_inputs(E))
            rr = R.train_step(lat, text)
            rec["noise"].append((raw_g - rr["out_model"]["Unet_raw"].detach()).clone())
            for k in ("sigma", "x", "unet_mask", "vit_mask"):
                assert torch.equal(R.inputs.buf[k], G.inputs.buf[k]), k
            if step == 2:                                       # K = 3 steps done
                rec["after3"] = {n: p.detach().clone() for n, p in G.model.named_parameters()}
                rec["sched3"] = G.scheduler.last_epoch
                rec["rstep3"] = float(G.optimizer.state[next(G.model.net.Unet_router.parameters())]["step"])
        torch.cuda.synchronize()
        yield rec
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)


def test_inputs_per_step_match_the_eager_device_inputs(live_run):
    g_in, e_in = live_run["g_in"], live_run["e_in"]
    for step in range(4):
        for k in ("sigma", "x", "unet_mask", "vit_mask", "zeta", "src"):
            assert torch.equal(g_in[step][k], e_in[step][k]), (step, k)
        assert float(g_in[step]["zeta"]) == float(torch.tensor(live_run["zeta_host"][step], dtype=torch.float32))
    for a in range(4):
        for b in range(a + 1, 4):
            for k in ("sigma", "x", "zeta"):
                assert not torch.equal(g_in[a][k], g_in[b][k]), (a, b, k)
    assert live_run["zeta_host"][:4] == [2.0, pytest.approx(1.5), pytest.approx(0.5), 0.0]
    # the bandwidth grows at step 2 and again at step 4.  Sigma is new every step, so "non-decreasing" is read on one sigma: the mask of
    # step s is the torch generator's at step s, and its rows are at least as wide as the same sigma gives under the step-0 bandwidth
    G = live_run["G"]
    for k, gen in (("unet_mask", G.unet_mask_gen), ("vit_mask", G.vit_mask_gen)):
        bws = [gen.bandwidth_scheduler(s) for s in range(5)]
        assert bws[0] == bws[1] < bws[2] == bws[3] < bws[4]
        grew = 0
        for s in range(5):
            got = g_in[s][k]
            assert torch.equal(got, gen(g_in[s]["sigma"], s)), (k, s)
            narrow = gen(g_in[s]["sigma"], 0)
            assert bool((got.sum(1) >= narrow.sum(1)).all()) and bool((got >= narrow).all()), (k, s)
            assert bool((got.sum(1) >= 1).all())
            grew += int(got.sum() > narrow.sum())
        print(k, "row sums per step:", [g_in[s][k].sum(1).tolist() for s in range(5)])
        assert grew >= 1


def test_zeta_is_live_under_replay(live_run):
    """The router's logit noise = Unet_raw minus the zeta-0 run on the same inputs and weights: there while zeta > 0, exactly zero at
    zeta 0.  A capture that baked its zeta (2.0 at the capture) fails the last two steps."""
    for step, (zeta, noise) in enumerate(zip(live_run["zeta_host"], live_run["noise"])):
        fin = noise[torch.isfinite(noise)]                      # masked experts carry the same -inf on both sides
        print(f"step {step}: zeta {zeta}, max |logit noise| {float(fin.abs().max()):.4g}")
        if zeta > 0:
            assert float(fin.abs().max()) > 1e-3 * zeta
        else:
            assert float(fin.abs().max()) == 0.0


def test_optimizer_side_after_three_graphed_steps(live_run):
    assert live_run["rstep3"] == 3.0
    assert live_run["sched3"] == 3
    moved = [n for n, p in live_run["after3"].items() if not torch.equal(p, live_run["before"][n])]
    assert any("Unet_experts" in n for n in moved) and any("vit_router" in n for n in moved) and any("cross_attn" in n for n in moved)


def test_resume_regenerates_the_inputs_of_a_step(live_run):
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    try:
        T = _trainer(2, 2.0, 3, graphed=True, seed=SEED)
        T.step_idx = 2
        T.train_step(live_run["lat"], live_run["text"])
        torch.cuda.synchronize()
        assert T.step_idx == 3
        for k, v in live_run["g_in"][2].items():
            assert torch.equal(T.inputs.buf[k], v), k
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)


def test_shape_change_and_cpu_latents_raise(live_run):
    from Utils import configs, training
    G = live_run["G"]
    lat5, text5 = _batch(5)
    idx, snap = G.step_idx, _inputs(G)
    with pytest.raises(ValueError):
        G.train_step(lat5, text5)
    torch.cuda.synchronize()
    assert G.step_idx == idx and all(torch.equal(G.inputs.buf[k], v) for k, v in snap.items())      # before any device work
    mcfg, mask, zeta = _configs(0.0, 4)
    T = training.Trainer(G.model, mcfg, configs.optim_configs, configs.loss_configs, mask, zeta, graphed=True, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.train_step(live_run["lat"].cpu(), live_run["text"].cpu())


# ------------------------------------------------------------------------------------------------------------------ defaults untouched
def test_default_trainer_keeps_torchs_generator_and_never_calls_the_new_entries(monkeypatch):
    import hdmoe_hip
    from hdmoe_hip import ops
    from Utils import configs, training
    from models import model_config2
    assert hasattr(ops, "train_inputs")
    names = []
    inner = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), inner(name, *a))[1])
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    try:
        over = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
                    VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8, top_k=2)
        mcfg = dict(configs.model_configs, **over, total_steps=10)
        torch.manual_seed(0)
        model = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg)).to(DEV).train()
        tr = training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, configs.zeta_configs)
        assert not tr.device_inputs and not tr.graphed and tr.inputs is None
        g = torch.Generator(device=DEV).manual_seed(1)
        lat, text = 0.5 * torch.randn(8, 4, 16, 16, device=DEV, generator=g), torch.randn(8, 5, 32, device=DEV, generator=g)
        torch.cuda.manual_seed(1234)
        res = tr.train_step(lat, text)
        state = torch.cuda.get_rng_state(DEV)
        sigma = res["sigma"].clone()
        assert "hdmoe_randn" in names and "hdmoe_randn_ds" not in names and "hdmoe_train_inputs" not in names
        # the parent's draws, in its order: sample_sigma_hybrid (randn, rand, randperm), then the noise
        torch.cuda.manual_seed(1234)
        n_ln = int(8 * (1 - 0.5))
        ln = (torch.randn([n_ln, 1, 1, 1], device=DEV) * configs.mask_configs["p_std"] + configs.mask_configs["p_mean"]).exp()
        u = torch.rand([8 - n_ln, 1, 1, 1], device=DEV)
        perm = torch.randperm(8, device=DEV)
        torch.randn_like(lat)
        assert torch.equal(torch.cuda.get_rng_state(DEV), state)
        import math
        lu = (u * (math.log(mcfg["sigma_max"]) - math.log(mcfg["sigma_min"])) + math.log(mcfg["sigma_min"])).exp()
        assert torch.equal(sigma, torch.cat([ln, lu], dim=0).clamp(mcfg["sigma_min"], mcfg["sigma_max"])[perm])
    finally:
        hdmoe_hip.set_compute_dtype(torch.float32)
