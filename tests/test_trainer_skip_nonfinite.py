"""Trainer(skip_nonfinite=True, health_every=n, max_skips_in_a_row=m): a step whose gradients hold a NaN is skipped on the device and
leaves parameters, optimizer state and EMA as they were; the health record names the expert; the default trainer is untouched (and lost).

The model, batch and configs are those of test_trainer_graphed.py (B = 6).  No non-finite value goes through the model's kernels: the test
wraps ``tr.buckets.finish`` and, after the real call, writes one NaN into element 0 of the gradient of a parameter of Unet_experts[1].

Where the reference point of "unchanged" lies.  In train mode the model's forward re-normalises the stored MP_Conv weights in place
(models/model_internals.py, MP_Conv), so the parameters behind a skipped step differ from those behind the step before by exactly that
renormalisation, with or without the guard.  The same wrapper therefore copies the model's state where the poison is planted -- behind
the step's forward and backward, in front of its update -- and the state behind the step is compared byte for byte with that copy; the
optimizer state and the EMA, which no forward touches, are compared with the copies taken behind step 0."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x0BADC0FFEE123457
B = 6
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _bf16():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


def _model():
    """BASELINE config 2 at its real width with the recipe's weights, train() mode without randomness (every dropout p = 0)."""
    from Utils import configs
    from models import model_config2
    from oracle.recipe import fill_state
    model = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(**configs.BASELINE_CONFIGS[2]["over"]))
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
    mask = dict(configs.mask_configs, step_size=0.5)
    zeta = dict(configs.zeta_configs, total_schedule_steps=zeta_steps, max_zeta=max_zeta, min_zeta=0.0, warmup_ratio=0.0)
    return mcfg, mask, zeta


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).clone()


def _model_state(tr):
    return {k: _bytes(v) for k, v in tr.model.state_dict().items()}


def _update_state(tr):
    """Optimizer state and EMA: what no forward touches."""
    out = {}
    for i, p in enumerate(tr._clip_params):
        for k, v in tr.optimizer.state.get(p, {}).items():
            out[f"{k}{i}"] = _bytes(v)
    for k, flat in enumerate(tr.ema._flat):
        out[f"ema{k}"] = _bytes(flat)
    out["ema_step"] = tr.ema._step.clone()
    return out


def _differs(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


def _trainer(poison_steps, **kw):
    """A trainer with a WeightEMA whose `buckets.finish` plants the NaN on `poison_steps` and copies the model's state there."""
    from hdmoe_hip.ema import WeightEMA
    from Utils import configs, training
    mcfg, mask, zeta = _configs(0.0, 4)
    model = _model()
    tr = training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, mask, zeta, seed=SEED, ema=WeightEMA(model), **kw)
    tr.victim = next(model.net.Unet_experts[1].parameters())
    tr.at_poison = {}
    inner = tr.buckets.finish

    def finish(*a, **k):
        out = inner(*a, **k)
        if tr.step_idx in poison_steps:
            tr.victim.grad.view(-1)[0] = NAN
            tr.at_poison[tr.step_idx] = _model_state(tr)
        return out

    tr.buckets.finish = finish
    return tr


def _finite(tr):
    return all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())


@pytest.mark.parametrize("mode", ["device_inputs", "graphed"])
def test_clean_poisoned_clean(mode, tmp_path):
    from graphs.logger import Logger
    from hdmoe_hip.optim import health_groups
    lat, text = _batch()
    observe = mode == "device_inputs"                                    # this mode also reads: health_every=1 with a Logger
    kw = dict(health_every=1, logger=Logger(log_dir=str(tmp_path), run_name="run", log_interval=1)) if observe else {}
    tr = _trainer({1}, skip_nonfinite=True, **{mode: True}, **kw)
    names = health_groups(tr.model)[0]

    r0 = tr.train_step(lat, text)
    assert int(r0["step_ok"]) == 1 and float(r0["grad_norm"]) > 0
    model0, update0 = _model_state(tr), _update_state(tr)
    assert int(tr.ema._step.item()) == 1

    r1 = tr.train_step(lat, text)                                        # the poisoned step
    assert int(r1["step_ok"]) == 0 and tr.step_idx == 2 and tr.scheduler.last_epoch == 2
    assert _differs(update0, _update_state(tr)) == []                    # optimizer state and EMA: as behind step 0
    now = _model_state(tr)
    assert _differs(tr.at_poison[1], now) == []                          # the model: as in front of the skipped update
    print(f"{mode}: {len(_differs(model0, now))} of {len(now)} state tensors re-normalised by the skipped step's forward")
    assert _finite(tr)
    assert float(tr.buckets.usage.abs().sum()) == 0.0

    r2 = tr.train_step(lat, text)
    assert int(r2["step_ok"]) == 1 and _finite(tr) and tr.step_idx == 3
    after = _model_state(tr)
    moved = _differs(now, after)
    assert any("Unet_experts" in k for k in moved) and any("vit_router" in k for k in moved) and any("cross_attn" in k for k in moved)
    assert int(tr.ema._step.item()) == 2
    h = tr.health()
    assert (h["skipped"], h["last_skipped_step"], h["skipped_in_a_row"], h["measured"]) == (1, 1, 0, 3)
    assert h["groups"] == names and h["param"]["total"]["nonfinite"] == 0 and tr.last_health is h

    if observe:
        lines = [json.loads(s) for s in (tmp_path / "run_health.jsonl").read_text().splitlines()]
        assert [r["step"] for r in lines] == [0, 1, 2] and [r["ok"] for r in lines] == [1, 0, 1]
        want = [1 if n == "Unet_experts.1" else 0 for n in names]
        for r in lines:
            assert r["groups"] == names
            assert r["per_group"]["grad_nonfinite"] == (want if r["step"] == 1 else [0] * len(names))
            assert r["per_group"]["weight_nonfinite"] == [0] * len(names)
        assert lines[1]["last_skipped_step"] == 1 and lines[2]["skipped_in_a_row"] == 0 and lines[2]["skipped"] == 1


def test_the_default_trainer_is_untouched_and_lost():
    """What the guard is for: the same poison without it ends in non-finite parameters.  The expert is poisoned on both remaining steps,
    so that one of them is a step in which it was routed (an unrouted expert's tensors are left out of the update)."""
    lat, text = _batch()
    tr = _trainer({1, 2}, device_inputs=True)
    assert tr.skip_nonfinite is False and tr._health is None
    for _ in range(3):
        res = tr.train_step(lat, text)
    torch.cuda.synchronize()
    assert "step_ok" not in res and "grad_norm" not in res and tr._health is None
    assert not _finite(tr)


def test_max_skips_in_a_row_raises_with_the_parameters_intact():
    lat, text = _batch()
    tr = _trainer({0, 1, 2}, device_inputs=True, skip_nonfinite=True, health_every=1, max_skips_in_a_row=2)
    ema0 = [_bytes(f) for f in tr.ema._flat]
    tr.train_step(lat, text)
    assert tr.last_health["skipped_in_a_row"] == 1
    with pytest.raises(RuntimeError, match="in a row"):
        tr.train_step(lat, text)
    assert _differs(tr.at_poison[1], _model_state(tr)) == [] and _finite(tr)     # as in front of the second skipped update
    for p in tr._clip_params:                                            # no update ever ran: counters and moments at zero
        st = tr.optimizer.state.get(p, {})
        assert all(float(v.abs().sum()) == 0.0 for v in st.values())
    assert int(tr.ema._step.item()) == 0 and all(torch.equal(a, _bytes(f)) for a, f in zip(ema0, tr.ema._flat))
