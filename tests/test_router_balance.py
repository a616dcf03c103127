"""The routers' selection bias through the model, the sampler, the evaluator and the Trainer (eager and graphed), on the small config-2
model and dataset of test_evaluator.py / test_latent_dataset.py (helpers copied so that the file stands alone).

What a step must satisfy is recomputed on the host from what the step itself reports: the bias behind step s equals the update rule
applied to the bias behind step s - 1 and step s's ``load`` / ``target`` (rate and bias_max dyadic: every fp32 operation is exact, the
comparison is bit for bit), and ``load`` / ``target`` equal the integer reference over the step's own router masks -- sum(load) is
sum_b min(k, a_b), which is B * k where no mask bites."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TINY = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
            VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8, top_k=2)
TSEED = 0x0BADC0FFEE123457
N, B, E, K = 10, 4, 4, 2
SHIFT = 20
RATE, BIAS_MAX = 0.125, 0.25
ROUTERS = ("net.Unet_router", "net.vit_router")


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model


def _dataset():
    from Utils.utils import LatentDataset
    g = torch.Generator(device=DEV).manual_seed(3)
    mean = 0.5 * torch.randn(N, 4, 16, 16, device=DEV, generator=g)
    std = 0.1 + torch.rand(N, 4, 16, 16, device=DEV, generator=g)
    text = torch.randn(N, 5, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    return LatentDataset(mean, std, scale=1.0, flip=0.5, text=text)


def _cfgs():
    from Utils import configs
    mcfg = dict(configs.model_configs, **TINY, total_steps=10)
    zeta = dict(configs.zeta_configs, total_schedule_steps=4, max_zeta=0.0, min_zeta=0.0, warmup_ratio=0.0)
    return configs, mcfg, zeta


def _model(train=False):
    from models import model_config2
    configs, mcfg, _ = _cfgs()
    torch.manual_seed(0)
    model = _no_dropout(model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg)).to(DEV))
    return model.train() if train else model.eval()


def _trainer(model=None, **kw):
    from Utils import training
    configs, mcfg, zeta = _cfgs()
    model = _model(train=True) if model is None else model
    return training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, zeta,
                            dataset=_dataset(), batch_size=B, seed=TSEED, **kw)


def _forward_inputs():
    g = torch.Generator(device=DEV).manual_seed(11)
    x = 0.5 * torch.randn(B, 4, 16, 16, device=DEV, generator=g)
    sigma = torch.tensor([0.05, 0.4, 2.0, 30.0], device=DEV).view(B, 1, 1, 1)
    text = torch.randn(B, 5, 32, device=DEV, generator=g)
    um = torch.tensor([[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 0], [1, 1, 0, 1]], dtype=torch.float32, device=DEV)
    vm = torch.ones(B, E, device=DEV)
    return dict(x=x, sigma=sigma, text_emb=text, Unet_router_mask=um, Vit_router_mask=vm, zeta=0.0, return_log_var=True,
                transition_point=-1.2, softness=1.6)


def _logged(fn):
    """(fn(), the C-ABI entry points it called)."""
    from hdmoe_hip import _lib
    _lib.CALL_LOG = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [name for name, _ in _lib.CALL_LOG]
    finally:
        _lib.CALL_LOG = None


def _same_bits(a, b, path="out"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, path
        assert torch.equal(a.detach().contiguous().view(torch.uint8), b.detach().contiguous().view(torch.uint8)), path
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for key in a:
            _same_bits(a[key], b[key], f"{path}[{key!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _same_bits(u, v, f"{path}[{i}]")
    else:
        assert a == b, path


# ------------------------------------------------------------------------------------------------------------------ off / on
def test_feature_off_is_the_untouched_model_and_launches_the_plain_head():
    from hdmoe_hip.balance import RouterBalance, balanced_routers
    inp = _forward_inputs()
    plain = _model()                                             # never saw the feature
    off = _model()
    tr = _trainer(off.train())                                   # balance_rate=None: the Trainer enables nothing
    off.eval()
    assert tr.balance is None and balanced_routers(off) == [] and tr.buckets._balanced == []
    with torch.no_grad():
        plain(**inp), off(**inp)                                 # (what only a model's first forward launches stays out of the logs)
        ref, names_ref = _logged(lambda: plain(**inp))
        got, names = _logged(lambda: off(**inp))
    _same_bits(ref, got)
    assert names == names_ref and names.count("hdmoe_router_head_fwd") == 2
    assert "hdmoe_router_head_bias_fwd" not in names and "hdmoe_balance_bias_update" not in names
    # ... and switched on, with the bias still zero, the new head returns the same bits
    on = _model()
    keys = list(on.state_dict())
    RouterBalance(on, RATE, BIAS_MAX)
    assert [n for n, _ in balanced_routers(on)] == list(ROUTERS)
    assert list(on.state_dict()) == keys                         # feature on: the state_dict keys are unchanged
    on.load_state_dict(plain.state_dict())                       # strict
    with torch.no_grad():
        on(**inp)
        got_on, names_on = _logged(lambda: on(**inp))
    _same_bits(ref, got_on)
    assert names_on.count("hdmoe_router_head_bias_fwd") == 2 and "hdmoe_router_head_fwd" not in names_on
    assert [n for n in names_on if n != "hdmoe_router_head_bias_fwd"] == [n for n in names if n != "hdmoe_router_head_fwd"]


def test_a_large_negative_bias_keeps_an_expert_unrouted():
    import models.model_components as mc
    torch.manual_seed(5)
    r = mc.Router(in_channels=4, time_dim=6, top_k=2, num_experts=5).to(DEV).eval()
    x, te = torch.randn(64, 4, 8, 8, device=DEV), torch.randn(64, 6, device=DEV)
    mask = (torch.rand(64, 5, device=DEV) < 0.7).float()
    mask[:, 1] = 1.0                                             # expert 1 always allowed ...
    mask[:8, [0, 2]] = 1.0                                       # ... beside at least two others on most rows,
    mask[8:12] = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0], device=DEV)   # with exactly one other on these,
    mask[12:16] = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0], device=DEV)  # and alone on these
    with torch.no_grad():
        s0, p0, l0 = r(x, te, mask, 0.0)
        assert int((s0[mask.sum(1) >= 4, 1] > 0).sum()) > 0      # without a bias expert 1 is in use beside three or more others
        r.enable_balance()
        r.balance_bias[1] = -1.0e4
        s1, p1, l1 = r(x, te, mask, 0.0)
        s2, p2, _ = r(x, te, None, 0.0)
    others = mask.sum(1) - 1
    assert bool((s1[others >= 2, 1] == 0).all()) and int((others >= 2).sum()) > 32       # never while k others are allowed
    assert bool((s1[8:12, 1] > 0).all()) and bool((s1[8:12, 3] > 0).all())                    # the second pick where only one other is
    assert bool((s1[12:16, 1] == 1).all())                       # the only allowed expert: routed, at weight 1
    assert bool((s2[:, 1] == 0).all()) and bool(((s2 > 0).sum(1) == 2).all())
    assert torch.equal(p0, p1) and torch.equal(l0, l1)           # gate probabilities and logits: untouched by the bias
    assert bool(torch.isfinite(s1).all()) and bool((s1.sum(1) - 1).abs().max() < 1e-6)


def test_inference_leaves_the_accumulators_at_zero():
    from hdmoe_hip.balance import RouterBalance
    from Utils.EDM_sampler import EDM_Sampler
    from Utils.evaluation import Evaluator
    configs, mcfg, _ = _cfgs()
    model = _model()
    bal = RouterBalance(model, RATE, BIAS_MAX)
    for i, (_, r) in enumerate(bal.routers):
        r.balance_bias.copy_(torch.tensor([0.25, -0.25, 0.125, -0.125], device=DEV) * (1 - 2 * i))
    inp = _forward_inputs()
    s = EDM_Sampler(model, model, num_solve_steps=2)
    with torch.no_grad():
        d, names = _logged(lambda: s.denoise(inp["x"], inp["sigma"], inp["text_emb"], -1.2, 1.6))
    assert bool(torch.isfinite(d).all()) and names.count("hdmoe_router_head_bias_fwd") == 2       # it routes with the bias ...
    ev = Evaluator(model, mcfg, configs.mask_configs, _dataset(), B, levels=2, rounds=1, seed=7, graphed=False)
    res = ev.evaluate()
    model.train()
    with torch.no_grad():
        model(**inp)
    torch.cuda.synchronize()
    assert res["n"] > 0
    for _, r in bal.routers:                                     # ... and counts nothing
        assert r.balance_load.tolist() == [0] * E and r.balance_target.tolist() == [0] * E
    model(**inp)                                                 # the same forward with grad enabled, in train mode, does
    torch.cuda.synchronize()
    assert all(int(r.balance_load.sum()) > 0 for _, r in bal.routers)


# ------------------------------------------------------------------------------------------------------------------ the Trainer
def _ref_update(bias, load, target):
    """The update rule in fp32 numpy, in the kernel's order (dyadic RATE / BIAS_MAX / E: exact)."""
    sign = np.array([(t > (l << SHIFT)) - (t < (l << SHIFT)) for l, t in zip(load, target)], dtype=np.float32)
    v = (bias + np.float32(RATE) * sign).astype(np.float32)
    s = np.float32(0)
    for i in range(len(v)):
        s = np.float32(s + v[i])
    v = (v - np.float32(s / np.float32(len(v)))).astype(np.float32)
    return np.clip(v, np.float32(-BIAS_MAX), np.float32(BIAS_MAX)).astype(np.float32)


def _ref_counts(mask, raw, bias):
    """Integer reference of a step's counts from its router mask (B, E), the masked logits the step returned (zeta 0: no noise) and
    the bias the step routed with: fp64 top-k of raw + bias, ties to the lowest index, counted where the mask allows."""
    allowed = mask != 0
    idx = np.argsort(-(raw.astype(np.float64) + bias.astype(np.float64)[None, :]), axis=1, kind="stable")[:, :K]
    load = [0] * E
    for b in range(B):
        for e in idx[b]:
            load[int(e)] += int(allowed[b, int(e)])
    target = [0] * E
    for b in range(B):
        a = int(allowed[b].sum())
        share = 0 if a == 0 else ((min(K, a) << (SHIFT + 1)) + a) // (2 * a)
        for e in range(E):
            if allowed[b, e]:
                target[e] += share
    return load, target, sum(min(K, int(allowed[b].sum())) for b in range(B))


def _snap(res):
    torch.cuda.synchronize()
    return {n: {k: v.detach().cpu().numpy().copy() for k, v in d.items()} for n, d in res["router_balance"].items()}


def _check_steps(tr, steps=4):
    prev = {n: np.zeros(E, np.float32) for n in ROUTERS}
    moved = 0
    for step in range(steps):
        res = tr.train_step()
        now = _snap(res)
        assert tuple(now) == ROUTERS
        for n, mkey, rkey in (("net.Unet_router", "unet_mask", "Unet_raw"), ("net.vit_router", "vit_mask", "vit_raw")):
            got = now[n]
            mask = tr.inputs.buf[mkey].cpu().numpy()
            load, target = [int(v) for v in got["load"]], [int(v) for v in got["target"]]
            want = _ref_update(prev[n], load, target)
            assert np.array_equal(got["bias"].view(np.int32), want.view(np.int32)), (step, n, got["bias"], want)
            raw = res["out_model"][rkey].detach().float().cpu().numpy()
            assert np.array_equal(np.isneginf(raw), mask == 0)
            rl, rt, total = _ref_counts(mask, raw, prev[n])
            assert load == rl and target == rt and sum(load) == total, (step, n, load, rl, target, rt, total)
            if bool((mask != 0).all()):
                assert sum(load) == B * K
            moved += int(not np.array_equal(got["bias"], prev[n]))
            prev[n] = got["bias"]
        for _, r in tr.balance.routers:                          # cleared behind the update
            assert r.balance_load.tolist() == [0] * E and r.balance_target.tolist() == [0] * E
    assert moved >= steps                                        # B * k = 8 rows over 4 experts are rarely even: the bias moves
    return prev


@pytest.mark.parametrize("mode", ["eager", "graphed"])
def test_every_step_follows_the_update_rule(mode):
    tr = _trainer(balance_rate=RATE, balance_bias_max=BIAS_MAX, graphed=mode == "graphed")
    assert tr.balance is not None and len(tr.buckets._balanced) == 2
    addr = [r.balance_bias.data_ptr() for _, r in tr.balance.routers]
    _, names = _logged(lambda: _check_steps(tr, 1))
    assert names.count("hdmoe_balance_bias_update") == 2         # one launch per router and step
    if mode == "eager":
        assert names.count("hdmoe_router_head_bias_fwd") == 2 and "hdmoe_router_head_fwd" not in names
    tr2 = _trainer(balance_rate=RATE, balance_bias_max=BIAS_MAX, graphed=mode == "graphed")
    final = _check_steps(tr2, 4)
    assert addr != [] and all(float(np.abs(b).max()) <= BIAS_MAX for b in final.values())
    assert [r.balance_bias.data_ptr() for _, r in tr.balance.routers] == addr     # updated in place: the captured heads read it by pointer
    if mode == "graphed":
        assert tr2._staged is not None


def test_a_skipped_step_keeps_the_bias_bit_for_bit():
    tr = _trainer(balance_rate=RATE, balance_bias_max=BIAS_MAX, skip_nonfinite=True, device_inputs=True)
    victim = next(tr.model.net.Unet_experts[1].parameters())
    inner = tr.buckets.finish

    def finish(*a, **k):
        out = inner(*a, **k)
        if tr.step_idx == 1:
            victim.grad.view(-1)[0] = float("nan")
        return out

    tr.buckets.finish = finish
    r0 = tr.train_step()
    s0 = _snap(r0)
    assert int(r0["step_ok"]) == 1 and any(np.abs(s0[n]["bias"]).max() > 0 for n in ROUTERS)
    r1 = tr.train_step()
    s1 = _snap(r1)
    assert int(r1["step_ok"]) == 0
    for n in ROUTERS:
        assert np.array_equal(s1[n]["bias"].view(np.int32), s0[n]["bias"].view(np.int32))
        assert int(s1[n]["load"].sum()) > 0                      # the skipped step's counts were copied out ...
    for _, r in tr.balance.routers:                              # ... and cleared: they do not leak into the next decision
        assert r.balance_load.tolist() == [0] * E and r.balance_target.tolist() == [0] * E
    r2 = tr.train_step()
    s2 = _snap(r2)
    assert int(r2["step_ok"]) == 1
    for n in ROUTERS:
        want = _ref_update(s1[n]["bias"], [int(v) for v in s2[n]["load"]], [int(v) for v in s2[n]["target"]])
        assert np.array_equal(s2[n]["bias"].view(np.int32), want.view(np.int32))


def test_resume_restores_both_biases(tmp_path):
    from Utils import training
    configs, mcfg, _ = _cfgs()
    tr = _trainer(balance_rate=RATE, balance_bias_max=BIAS_MAX, device_inputs=True)
    for _ in range(2):
        tr.train_step()
    want = _snap({"router_balance": tr.balance.last()})
    assert all(np.abs(want[n]["bias"]).max() > 0 for n in ROUTERS)
    path = training.save_checkpoint(tr.model, tr.optimizer, tr.step_idx, 0.0, {"model_configs": dict(mcfg, save_dir=str(tmp_path))}, "ck.pt",
                                    balance=tr.balance)
    tr2 = _trainer(balance_rate=RATE, balance_bias_max=BIAS_MAX, device_inputs=True)
    ck = training.load_checkpoint(path, tr2.model, tr2.optimizer, balance=tr2.balance)
    assert "router_balance" in ck
    got = _snap({"router_balance": tr2.balance.last()})
    for n in ROUTERS:
        assert np.array_equal(got[n]["bias"].view(np.int32), want[n]["bias"].view(np.int32))
